"""fp64 oracle, inputs and derived bounds for the fused RoPE + paged-KV-write (rope_cache.hip's
4-element kernel, 16-byte kernel and its q/k-norm instantiation; the kEpRope epilogue of the GEMV
in gemv_core.h), shared by test_rope_oracle_cpu.py (the oracle on its own, planted errors,
ops/reference.py under the same families) and test_rope_oracle_gpu.py (the HIP kernels).

The oracle is written from the definition and shares no code with ops/reference.py:

  input     bf16 qkv [T, (nh + 2 nkv) D] (q heads | k heads | v heads), or S split-K partials
            (fp32 or bf16) summed in fp32 in split order and rounded to bf16 once
  q/k norm  n = bf16(x rsqrt(mean(x^2) + eps) w) per q / k head, fp64 from the bf16 input
  rotation  fp64, from the fp32 table values (the table is an input): with half = D / 2, i < half,
            a = x[i], b = x[i + half], c = cos[p, i] = table[p, i], s = sin[p, i] =
            table[p, half + i]:  out[i] = a c - b s,  out[i + half] = b c + a s
            q and k use p = clamp(pos, 0, max_pos - 1); q_sink uses
            p = clamp(min(pos, window - 1), 0, max_pos - 1); no table: out = x
  K cache   element (slot, kh, d) at flat index ((blk nkv + kh) bs + off) D + d
  V^T cache element (slot, kh, d) at ((((blk nkv + kh) (bs / 8) + off / 8) D + d) 8 + off % 8
            with blk = slot / bs, off = slot % bs; slot -1 writes nothing; every element that no
            slot addresses keeps its initial value

Bounds (derived here, not tuned against any implementation).  The kernels compute
bf16(fmaf(a, c, -(b s))) in fp32.  t = fl(b s) errs by <= 2^-24 |b s|; the fma rounds once:
|r - (a c - t)| <= 2^-24 |a c - t|.  So the fp32 value r is within d = 2^-23 (|a c| + |b s|) of
the exact e (the 2^-48 term is dropped).  The bf16 rounding adds half a bf16 ulp of r; r may sit
one binade above e, where that half ulp is a whole ulp(e) -- but only when d carried it across
the power of two, and then the excess is below d.  Hence

  plain     |got - e| <= ulp_bf16(e) / 2 + 2^-22 (|a c| + |b s|)

(ops/reference.py's unfused fp32 form -- two products, one subtraction, three roundings of
2^-24 -- meets the same bound.)  With q/k norm the kernel's rsqrtf is approximate and its sum of
squares is an fp32 sum, so a normalised value may land on either bf16 neighbour of n; a and b
move by at most one ulp each:

  normed    ... + |c| ulp_bf16(n_a) + |s| ulp_bf16(n_b)

ulp_bf16(e) = 2^(floor(log2 |e|) - 7), floored at bf16's subnormal step 2^-133.  Where the
result is exactly representable (no table; a table row of cos = 1, sin = 0 on normal-range
inputs; inputs a = 1, b = 0) the bound is 0 and the comparison is of bit patterns.

fp8 (e4m3fn) caches hold byte = e4m3(fp32(v) * fp32(1 / scale)): product in fp32, conversion
round-to-nearest-even, finite values beyond +-448 and +-inf saturate to +-448, NaN stays a NaN
code (byte & 0x7F == 0x7F).  For V, v is the input value; for K it is the bf16 K the SAME
implementation wrote for the same input into a bf16 cache (that run is held to the fp64 bound
separately), so the byte comparison is exact and inherits no rounding ambiguity.

Input families (all tiny):
  coord     qkv[t, col] = the bf16 with a bit pattern unique to (t, col), every finite pattern;
            no table: q, K, V^T are a pure permutation of the input
  coordn    the same over normal-range magnitudes (exponent field 8 .. 247): what a GEMV of a
            one-hot x reproduces exactly, and what S partials of code / S sum to exactly
  coord1    coordn with a table whose every row is cos = 1, sin = 0: the fma is exact
  table     a = 1, b = 0 in every head; cos[p, i] = 2^p (1 + i / 128), sin[p, i] =
            2^-(p + 1) (1 + i / 128): out[i] = cos[pc, i], out[i + half] = sin[pc, i] name the
            table row and column every element used; positions -3, 0, 1, W - 2, W - 1, W,
            max_pos - 1, max_pos, max_pos + 7
  randn, big (1e4 randn), small (1e-3 randn), cancel (b = bf16(a c / s): a c - b s is the
            rounding residue): llama3-scaled table of 4096 rows, positions incl. 0 and 4095
  fp8edge   values that reach the encoder at +-447, +-448, +-463, +-464 (the tie that rounds past
            the top code), +-480, +-1e4, +-3e38, 2^-9 (smallest subnormal), 2^-10 (tie to zero)
            and their bf16 neighbours, +-inf and NaN; scales 1, 0.5, 0.3
"""
import dataclasses
import functools
import zlib
from typing import Optional, Tuple

import numpy as np
import torch

from row_oracle import e4m3_bytes
from distributed_llm_inference import ops
from distributed_llm_inference.ops.reference import build_cos_sin

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
G = 4096                        # guard elements on each side of every output
SENT = -12345.0                 # -12352 as bf16
SENT8 = 0x5A
TABLE_MAX_POS = 24
TABLE_WINDOW = 12
REAL_MAX_POS = 4096
LLAMA3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
          "original_max_position_embeddings": 8192}
EXACT_FAMILIES = ("coord", "coordn", "coord1", "table", "fp8edge", "fp8edge_t")
FP8_EDGE = (447.0, 448.0, 463.0, 464.0, 480.0, 1e4, 3e38, 2.0 ** -9, 2.0 ** -10)


@dataclasses.dataclass(frozen=True)
class Case:
    nh: int
    nkv: int
    D: int
    bs: int
    family: str
    nblocks: int = 3
    T: int = 11
    pad: int = 0                # row stride = width + pad (8: 16-byte kernel, 4: 4-element one)
    sliced: bool = False        # qkv is a column slice of a wider tensor
    window: int = 0             # > 0: q_sink wanted
    norm: bool = False
    parts: Optional[Tuple[int, str]] = None     # (S, 'f32' | 'bf16')
    k_scale: float = 1.0
    v_scale: float = 1.0
    eps: float = 1e-6
    pos_shift: int = 0          # short cases (T < 11): where in the position list they start

    @property
    def width(self):
        return (self.nh + 2 * self.nkv) * self.D

    @property
    def exact(self):
        return self.family in EXACT_FAMILIES

    @property
    def path(self):
        """The rope_cache.hip kernel the launcher picks."""
        if self.norm:
            return "v8norm"
        return "v8" if self.D % 16 == 0 and (self.width + self.pad) % 8 == 0 else "v4"

    def ident(self):
        s = f"{self.family}-h{self.nh}x{self.nkv}-D{self.D}-bs{self.bs}x{self.nblocks}-T{self.T}"
        s += f"-pad{self.pad}" if self.pad else ""
        s += "-slice" if self.sliced else ""
        s += f"-W{self.window}" if self.window else ""
        s += "-norm" if self.norm else ""
        s += f"-S{self.parts[0]}{self.parts[1]}" if self.parts else ""
        s += f"-ks{self.k_scale:g}-vs{self.v_scale:g}" if (self.k_scale, self.v_scale) != (1, 1) \
            else ""
        return s + (f"-p{self.pos_shift}" if self.pos_shift else "")


# ------------------------------------------------------------------------------------- inputs
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(shape, *key):
    return torch.randn(shape, generator=_gen(*key), dtype=torch.float32)


def coord_codes(n: int, normal: bool) -> torch.Tensor:
    """n distinct finite bf16 bit patterns (both signs; exponent field 0 .. 254, or 8 .. 247 when
    ``normal``), in a scrambled order."""
    e0, ne = (8, 240) if normal else (0, 255)
    per_sign = ne * 128
    assert n <= 2 * per_sign <= 65280, n
    i = np.arange(n, dtype=np.int64)
    m = (i // 2 * 7919) % per_sign          # 7919 is prime to 128 * 240 and to 128 * 255
    bits = ((i % 2) << 15) | ((m // 128 + e0) << 7) | (m % 128)
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16)).view(BF)


def slots_for(c: Case) -> torch.Tensor:
    """Slots of the T tokens: the first and last offset of the first and of the last block, all
    eight values of off % 8, several off / 8 groups, every block, one token with slot -1, no
    slot twice, in no monotonic order."""
    bs, nb, ng = c.bs, c.nblocks, c.bs // 8
    pairs = [(0, 0), (nb - 1, bs - 1)]
    pairs += [((1, nb - 1, 0)[r % 3] % nb, 8 * ((5 * r) % ng) + r) for r in range(1, 7)]
    pairs += [(0, bs - 1), (nb - 1, 0)]
    assert len(set(pairs)) == len(pairs) and all(0 <= b < nb and 0 <= o < bs for b, o in pairs)
    slots = [b * bs + o for b, o in pairs]
    slots.insert(4, -1)
    order = (7, 2, 10, 0, 4, 9, 1, 6, 3, 8, 5)
    out = [slots[j] for j in order][c.pos_shift % 3:][:c.T]
    assert len(out) == c.T
    return torch.tensor(out, dtype=torch.int64)


def table_code(D: int) -> torch.Tensor:
    half = D // 2
    p = torch.arange(TABLE_MAX_POS, dtype=torch.float64)[:, None]
    f = 1.0 + torch.arange(half, dtype=torch.float64)[None, :] / 128.0
    return torch.cat([2.0 ** p * f, 2.0 ** -(p + 1) * f], dim=1).float()


@functools.lru_cache(maxsize=None)
def real_table(D: int) -> torch.Tensor:
    return build_cos_sin(D, REAL_MAX_POS, 500000.0, LLAMA3).float().contiguous()


def _positions(c: Case) -> torch.Tensor:
    if c.family == "table":
        W, mp = c.window or TABLE_WINDOW, TABLE_MAX_POS
        p = [-3, 0, 1, W - 2, W - 1, W, mp - 1, mp, mp + 7, 2, 5]
    else:
        W = c.window or 64
        r = torch.randint(0, REAL_MAX_POS, (11,), generator=_gen("pos", c.ident())).tolist()
        p = [0, REAL_MAX_POS - 1, W - 2, W - 1, W, -3, REAL_MAX_POS + 7] + r[:4]
        if c.family == "fp8edge_t":
            p = [0] * 11
    k = c.pos_shift % len(p)
    return torch.tensor((p[k:] + p[:k])[:c.T], dtype=torch.int32)


def edge_values(scale: float, finite_only: bool = False) -> torch.Tensor:
    """bf16 inputs whose scaled value reaches the encoder at the FP8_EDGE points (both signs,
    with both bf16 neighbours), then +-inf and NaN."""
    t = torch.tensor(FP8_EDGE, dtype=torch.float64) * scale
    x = torch.cat([t, -t]).float().to(BF)
    bits = x.view(torch.int16)
    x = torch.cat([x, (bits + 1).view(BF), (bits - 1).view(BF)])
    x = x[torch.isfinite(x.float())]
    if not finite_only:
        x = torch.cat([x, torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=BF)])
    return x


def _fill_heads(x: torch.Tensor, vals: torch.Tensor, lo: int, hi: int, seed: int):
    """vals repeated over columns [lo, hi) of every row, each row starting elsewhere."""
    n = hi - lo
    for t in range(x.shape[0]):
        idx = (torch.arange(n) + 13 * t + seed) % vals.numel()
        x[t, lo:hi] = vals[idx]


@functools.lru_cache(maxsize=8)
def inputs(c: Case) -> dict:
    """The case's CPU tensors: qkv bf16 [T, width] (the sum of ``parts`` when given), positions
    int32, slots int64, cos_sin fp32 or None, q_norm / k_norm.  Cached: treat as read-only."""
    T, W, D, half = c.T, c.width, c.D, c.D // 2
    nqk = c.nh + c.nkv
    d = dict(slots=slots_for(c), cos_sin=None, positions=None)
    fam = c.family
    if fam in ("coord", "coordn", "coord1"):
        normal = fam != "coord" or c.parts is not None
        qkv = coord_codes(T * W, normal).reshape(T, W).clone()
        if fam == "coord1":
            cs = torch.zeros(TABLE_MAX_POS, D)
            cs[:, :half] = 1.0
            d["cos_sin"] = cs
            d["positions"] = (torch.arange(T, dtype=torch.int32) * 5) % TABLE_MAX_POS
    elif fam == "table":
        qkv = torch.zeros(T, W, dtype=BF)
        qkv.view(T, c.nh + 2 * c.nkv, D)[:, :nqk, :half] = 1.0
        qkv[:, nqk * D:] = coord_codes(T * c.nkv * D, True).reshape(T, -1)
        d["cos_sin"], d["positions"] = table_code(D), _positions(c)
    elif fam in ("fp8edge", "fp8edge_t"):
        qkv = torch.ones(T, W, dtype=BF)
        finite = fam == "fp8edge_t"
        _fill_heads(qkv, edge_values(c.k_scale, finite), c.nh * D, nqk * D, 0)
        _fill_heads(qkv, edge_values(c.v_scale, finite), nqk * D, W, 5)
        if finite:      # position 0 of a real table: cos = 1, sin = 0 exactly
            d["cos_sin"], d["positions"] = real_table(D), _positions(c)
            assert bool((d["cos_sin"][0, :half] == 1).all() and (d["cos_sin"][0, half:] == 0).all())
    else:
        g = _randn((T, W), fam, c.ident())
        mul = {"randn": 1.0, "big": 1e4, "small": 1e-3, "cancel": 1.0}[fam]
        qkv = (g * mul).to(BF)
        d["cos_sin"], d["positions"] = real_table(D), _positions(c)
        if fam == "cancel":
            pc = d["positions"].long().clamp(0, REAL_MAX_POS - 1)
            cs = d["cos_sin"][pc].double()
            cc, ss = cs[:, None, :half], cs[:, None, half:]
            h = qkv.view(T, -1, D)[:, :nqk]
            a = h[..., :half].double()
            b = torch.where(ss.abs() > 1e-3, a * cc / ss, h[..., half:].double())
            h[..., half:] = b.clamp(-1e30, 1e30).to(BF)
    if c.norm:
        d["q_norm"] = (1.0 + 0.2 * _randn((D,), "qn", D)).to(BF)
        d["k_norm"] = (0.5 + 0.2 * _randn((D,), "kn", D)).to(BF)
    if c.parts is not None:
        S, pdt = c.parts
        dt = BF if pdt == "bf16" else torch.float32
        if c.exact:             # exact for S a power of two and normal-range codes
            assert S & (S - 1) == 0
            parts = (qkv.float() / S).to(dt)[None].expand(S, T, W)
        else:
            parts = qkv.float()[None] / S + 0.05 * _randn((S, T, W), "pn", c.ident())
        if c.pad:
            parts = torch.cat([parts, torch.full((S, T, c.pad), 7.0)], dim=2)
        d["parts"] = parts.to(dt).contiguous()
        acc = d["parts"][0, :, :W].float()
        for k in range(1, S):
            acc = acc + d["parts"][k, :, :W].float()
        qkv = acc.to(BF)
        if c.exact:
            assert torch.equal(qkv.view(torch.int16), (d["parts"][0, :, :W].float() * S).to(BF)
                               .view(torch.int16))
    d["qkv"] = qkv.contiguous()
    return d


# ------------------------------------------------------------------------------------- oracle
def ulp_bf16(e: torch.Tensor) -> torch.Tensor:
    _, ex = torch.frexp(e.abs().double())
    return torch.pow(2.0, (ex - 8).clamp(min=-133).double())


def _rot(X, cs, normed, ulpX, mutate):
    """X fp64 [T, H, D], cs fp32 [T, D] -> (exact, bound)."""
    half = X.shape[-1] // 2
    a, b = X[..., :half], X[..., half:]
    c, s = cs[:, None, :half].double(), cs[:, None, half:].double()
    if mutate == "sin_neg":
        s = -s
    if mutate == "partner4":
        b = torch.roll(b, 4, dims=-1)
    lo, hi = a * c - b * s, b * c + a * s
    e = torch.cat([lo, hi], dim=-1)
    m = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], dim=-1)
    bound = ulp_bf16(e) / 2 + 2.0 ** -22 * m
    if normed:
        ua, ub = ulpX[..., :half], ulpX[..., half:]
        bound = bound + torch.cat([c.abs() * ua + s.abs() * ub, c.abs() * ub + s.abs() * ua], -1)
    return e, bound


def oracle(c: Case, inp: dict, mutate: Optional[str] = None) -> dict:
    """Per token: q, qs (None without window), k as fp64 [T, heads, D] with bounds bq, bqs, bk
    (all 0 for the exact families), and v bf16 [T, nkv, D]."""
    T, D, nqk = c.T, c.D, c.nh + c.nkv
    H = inp["qkv"].view(T, c.nh + 2 * c.nkv, D)
    X = H[:, :nqk].double()
    ulpX = None
    if c.norm:
        w = torch.cat([inp["q_norm"].double()[None].expand(c.nh, D),
                       inp["k_norm"].double()[None].expand(c.nkv, D)])
        n = X * torch.rsqrt((X * X).mean(-1, keepdim=True) + float(np.float32(c.eps))) * w
        X = n.to(BF).double()
        ulpX = ulp_bf16(X)
    cs_all = inp["cos_sin"]
    if cs_all is None:
        z = torch.zeros_like(X)
        out = dict(q=X[:, :c.nh], bq=z[:, :c.nh], k=X[:, c.nh:], bk=z[:, c.nh:], qs=None, bqs=None)
        if c.window:
            out.update(qs=X[:, :c.nh], bqs=z[:, :c.nh])
    else:
        mp = cs_all.shape[0]
        pos = inp["positions"].long()
        if mutate == "pos+1":
            pos = pos + 1
        pc = pos.clamp(0, mp - 1)
        e, bnd = _rot(X, cs_all[pc], c.norm, ulpX, mutate)
        out = dict(q=e[:, :c.nh], bq=bnd[:, :c.nh], k=e[:, c.nh:], bk=bnd[:, c.nh:], qs=None,
                   bqs=None)
        if c.window:
            ps = torch.minimum(pos, torch.tensor(c.window - 1)).clamp(0, mp - 1)
            es, bs_ = _rot(X[:, :c.nh], cs_all[ps], c.norm, None if ulpX is None
                           else ulpX[:, :c.nh], mutate)
            out.update(qs=es, bqs=bs_)
    if c.exact:
        for n_ in ("bq", "bk", "bqs"):
            if out[n_] is not None:
                out[n_] = torch.zeros_like(out[n_])
    out["v"] = H[:, nqk:].contiguous()
    return out


def k_index(c: Case, slots: torch.Tensor):
    """(token rows, flat K-cache indices [n, nkv, D]) of the written tokens."""
    rows = (slots >= 0).nonzero().flatten()
    s = slots[rows]
    blk, off = (s // c.bs)[:, None, None], (s % c.bs)[:, None, None]
    kh, d = torch.arange(c.nkv)[None, :, None], torch.arange(c.D)[None, None, :]
    return rows, ((blk * c.nkv + kh) * c.bs + off) * c.D + d


def v_index(c: Case, slots: torch.Tensor):
    rows = (slots >= 0).nonzero().flatten()
    s = slots[rows]
    blk, off = (s // c.bs)[:, None, None], (s % c.bs)[:, None, None]
    kh, d = torch.arange(c.nkv)[None, :, None], torch.arange(c.D)[None, None, :]
    return rows, (((blk * c.nkv + kh) * (c.bs // 8) + off // 8) * c.D + d) * 8 + off % 8


def scatter(init: torch.Tensor, rows, idx, vals: torch.Tensor) -> torch.Tensor:
    img = init.clone().reshape(-1)
    img[idx.reshape(-1)] = vals[rows].reshape(-1).to(img.dtype)
    return img.reshape(init.shape)


def k_shape(c: Case):
    return (c.nblocks, c.nkv, c.bs, c.D)


def v_shape(c: Case):
    return (c.nblocks, c.nkv, c.bs // 8, c.D, 8)


def fp8_bytes(v: torch.Tensor, scale: float) -> torch.Tensor:
    """uint8 e4m3(fp32(v) * fp32(1 / scale)); NaN -> 0x7F (compare NaN codes with is_nan_code)."""
    inv = torch.tensor(float(np.float32(1.0 / scale)), dtype=torch.float32)
    x = v.float() * inv
    b = e4m3_bytes(torch.nan_to_num(x.double(), nan=0.0, posinf=448.0, neginf=-448.0))
    return torch.where(torch.isnan(x), torch.tensor(0x7F, dtype=torch.uint8), b)


def expected(c: Case, inp: dict, k_bf16: Optional[torch.Tensor] = None,
             mutate: Optional[str] = None) -> dict:
    """The expected outputs.  bf16 caches (``k_bf16`` None): q / qs / K as fp64 with bound
    images (bound 0 off the written slots and for the exact families), V bit-exact.  fp8 caches:
    K bytes from ``k_bf16`` -- the bf16 K cache image the implementation under test wrote for
    the same input -- and V bytes from the input."""
    o = oracle(c, inp, mutate)
    slots = inp["slots"]
    rows, ki = k_index(c, slots)
    _, vi = v_index(c, slots)
    exp = dict(q=o["q"], bq=o["bq"], qs=o["qs"], bqs=o["bqs"])
    if k_bf16 is None:
        k0 = torch.full(k_shape(c), SENT, dtype=BF).double()
        exp["k"] = scatter(k0, rows, ki, o["k"])
        exp["bk"] = scatter(torch.zeros(k_shape(c), dtype=torch.float64), rows, ki, o["bk"])
        exp["v"] = scatter(torch.full(v_shape(c), SENT, dtype=BF), rows, vi, o["v"])
    else:
        written = scatter(torch.zeros(k_shape(c), dtype=torch.bool), rows, ki,
                          torch.ones(c.T, c.nkv, c.D, dtype=torch.bool))
        exp["k8"] = torch.where(written, fp8_bytes(k_bf16, c.k_scale),
                                torch.tensor(SENT8, dtype=torch.uint8))
        exp["v8"] = scatter(torch.full(v_shape(c), SENT8, dtype=torch.uint8), rows, vi,
                            fp8_bytes(o["v"], c.v_scale))
    return exp


# --------------------------------------------------------------------------------- evaluation
@dataclasses.dataclass
class Verdict:
    ratios: dict = dataclasses.field(default_factory=dict)     # output -> largest err / bound
    problems: list = dataclasses.field(default_factory=list)

    @property
    def ratio(self):
        return max(self.ratios.values(), default=0.0)

    @property
    def ok(self):
        return self.ratio <= 1.0 and not self.problems


def _bounded(v: Verdict, what: str, got: torch.Tensor, e: torch.Tensor, bound: torch.Tensor):
    """Where bound > 0: |got - e| <= bound.  Where bound == 0: the bit pattern of bf16(e) (any
    NaN for NaN)."""
    want = e.to(BF)
    same = (got.view(torch.int16) == want.view(torch.int16)) | (got.isnan() & want.isnan())
    err = (got.double() - e).abs()
    q = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                    torch.where(same, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    q = torch.nan_to_num(q, nan=float("inf"))
    q = torch.where(same & ((bound == 0) | want.isnan() | want.isinf()), torch.zeros_like(q), q)
    m = float(q.max()) if q.numel() else 0.0
    v.ratios[what] = max(v.ratios.get(what, 0.0), m)
    if m > 1.0:
        i = np.unravel_index(int(q.argmax()), q.shape)
        v.problems.append(f"{what}: {int((q > 1).sum())} elements out of bound, worst {m:.3g}x "
                          f"at {tuple(int(j) for j in i)}: got {float(got[i]):.9g} want "
                          f"{float(e[i]):.9g} (bound {float(bound[i]):.3g})")


def is_nan_code(b: torch.Tensor) -> torch.Tensor:
    return (b & 0x7F) == 0x7F


def _bytes_equal(v: Verdict, what: str, got: torch.Tensor, want: torch.Tensor):
    ok = (got == want) | (is_nan_code(got) & is_nan_code(want))
    v.ratios[what] = max(v.ratios.get(what, 0.0), 0.0 if bool(ok.all()) else float("inf"))
    if not bool(ok.all()):
        i = tuple(int(j) for j in (~ok).nonzero()[0])
        v.problems.append(f"{what}: {int((~ok).sum())} bytes differ, first at {i}: got "
                          f"0x{int(got[i]):02X} want 0x{int(want[i]):02X}")


def evaluate(c: Case, exp: dict, out: dict) -> Verdict:
    """``out``: CPU tensors q, qs (or None), k, v (fp8 caches as uint8) and ``guards`` (a list of
    problems found around the outputs)."""
    v = Verdict(problems=list(out.get("guards", ())))
    _bounded(v, "q", out["q"], exp["q"], exp["bq"])
    if c.window:
        _bounded(v, "q_sink", out["qs"], exp["qs"], exp["bqs"])
    if "k" in exp:
        _bounded(v, "K", out["k"], exp["k"], exp["bk"])
        _bounded(v, "V", out["v"], exp["v"].double(), torch.zeros(v_shape(c), dtype=torch.float64))
    else:
        _bytes_equal(v, "K8", out["k"], exp["k8"])
        _bytes_equal(v, "V8", out["v"], exp["v8"])
    return v


def ideal_out(c: Case, inp: dict, mutate: Optional[str] = None) -> dict:
    """An implementation that rounds the oracle's exact values to bf16 (bf16 caches)."""
    e = expected(c, inp, mutate=mutate)
    return dict(q=e["q"].to(BF), qs=None if e["qs"] is None else e["qs"].to(BF),
                k=e["k"].to(BF), v=e["v"].clone(), guards=[])


# ------------------------------------------------------------------------------------ running
def _guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    fill = SENT8 if dtype == torch.uint8 else SENT
    buf = torch.full((G + n + G,), fill, dtype=dtype, device=dev)
    return buf, buf[G:G + n].view(*shape)


def _guard_problems(bufs: dict) -> list:
    out = []
    for what, (buf, n) in bufs.items():
        fill = torch.tensor(SENT8 if buf.dtype == torch.uint8 else SENT, dtype=buf.dtype)
        b = buf.cpu()
        if not bool((b[:G] == fill).all()):
            out.append(f"{what}: write before the output")
        if not bool((b[G + n:] == fill).all()):
            out.append(f"{what}: write after the output")
    return out


def device_inputs(c: Case, inp: dict, dev, native_parts: bool):
    """(qkv argument, positions, slots, cos_sin, q_norm, k_norm) on ``dev``.  The table sits in
    an allocation one row longer than max_pos."""
    to = lambda t: None if t is None else t.to(dev)
    if c.parts is not None and native_parts:
        qkv = ops.SplitKPartials(inp["parts"].to(dev))
    else:
        T, W = c.T, c.width
        lead = 16 if c.sliced else 0
        wide = torch.full((T, lead + W + c.pad + (24 if c.sliced else 0)), 3.0, dtype=BF,
                          device=dev)
        wide[:, lead:lead + W] = inp["qkv"].to(dev)
        qkv = wide[:, lead:lead + W]
        if not c.sliced and c.pad == 0:
            qkv = qkv.contiguous()
    cs = inp["cos_sin"]
    if cs is not None:
        big = torch.zeros(cs.shape[0] + 1, cs.shape[1], dtype=torch.float32, device=dev)
        big[:-1] = cs.to(dev)
        cs = big[:-1]
    return qkv, to(inp["positions"]), to(inp["slots"]), cs, to(inp.get("q_norm")), \
        to(inp.get("k_norm"))


def run_ops(c: Case, inp: dict, dev, fp8: bool) -> dict:
    """The case through ``ops.rope_cache`` with its tensors on ``dev`` (CPU: ops/reference.py;
    split-K partials are pre-summed there, the CPU front-end has no partials path), outputs and
    caches sentinel-filled and guarded on both sides.  Returns CPU tensors."""
    on_gpu = torch.device(dev).type != "cpu"
    qkv, pos, slots, cs, qn, kn = device_inputs(c, inp, dev, on_gpu)
    cdt = torch.uint8 if fp8 else BF
    kbuf, k = _guarded(k_shape(c), cdt, dev)
    vbuf, v = _guarded(v_shape(c), cdt, dev)
    qbuf, q = _guarded((c.T, c.nh, c.D), BF, dev)
    sbuf, qs = _guarded((c.T, c.nh, c.D), BF, dev)
    kc, vc = (k.view(F8), v.view(F8)) if fp8 else (k, v)
    ops.rope_cache(qkv, pos, slots, cs, c.nh, c.nkv, c.D, kc, vc, window=c.window,
                   want_sink=c.window > 0, q_out=q, q_sink_out=qs if c.window else None,
                   k_scale=c.k_scale, v_scale=c.v_scale, q_norm=qn, k_norm=kn, norm_eps=c.eps)
    if on_gpu:
        torch.cuda.synchronize()
    guards = _guard_problems(dict(K=(kbuf, k.numel()), V=(vbuf, v.numel()), q=(qbuf, q.numel()),
                                  q_sink=(sbuf, qs.numel())))
    if not c.window and not bool((qs.cpu() == torch.tensor(SENT, dtype=BF)).all()):
        guards.append("q_sink written without a window")
    return dict(q=q.cpu(), qs=qs.cpu() if c.window else None, k=k.cpu(), v=v.cpu(), guards=guards)


def check_both(c: Case, dev) -> dict:
    """bf16 caches against the fp64 bound, then fp8 caches against the byte images made from
    that run's K.  Returns {'bf16': Verdict, 'fp8': Verdict}."""
    inp = inputs(c)
    out = run_ops(c, inp, dev, False)
    vb = evaluate(c, expected(c, inp), out)
    out8 = run_ops(c, inp, dev, True)
    v8 = evaluate(c, expected(c, inp, k_bf16=out["k"]), out8)
    return dict(bf16=vb, fp8=v8)


# -------------------------------------------------------------------------------- case matrix
#        nh nkv   D   bs  nb pad sliced
GEOS = ((4, 2, 8, 8, 4, 0, False),          # 4-element kernel, one workgroup
        (4, 2, 32, 16, 3, 8, True),
        (9, 3, 48, 8, 4, 0, False),         # gpr = 3; q|k|v in workgroup 1
        (9, 3, 64, 64, 3, 4, False),        # odd row stride: 4-element kernel
        (14, 2, 80, 16, 4, 0, False),       # gpr = 5; q|k boundary mid-workgroup
        (14, 2, 128, 256, 3, 0, True),
        (12, 12, 96, 64, 3, 8, False),      # gpr = 6; v_lo > 0
        (12, 12, 64, 16, 4, 0, True),
        (12, 12, 80, 64, 3, 4, False),      # odd row stride: v_lo > 0 in the 4-element kernel
        (32, 8, 64, 64, 3, 0, False),
        (32, 8, 32, 256, 3, 4, False),
        (4, 2, 256, 8, 3, 0, False))


def _geo(i, family, **kw):
    nh, nkv, D, bs, nb, pad, sl = GEOS[i]
    return Case(nh, nkv, D, bs, family, nblocks=nb, pad=pad, sliced=sl, **kw)


def cases():
    out = []
    for i in range(len(GEOS)):
        out.append(_geo(i, "coord", window=(0, 64)[i % 2]))
        out.append(_geo(i, "coord1", window=(64, 0)[i % 2]))
    out += [_geo(3, "coord", T=1), _geo(6, "coord1", T=1, window=5), _geo(8, "coord", T=1),
            _geo(11, "coord1", T=1)]
    for i in (0, 2, 4, 5, 6, 10, 11):
        out.append(_geo(i, "table", window=(TABLE_WINDOW, 0)[i % 4 == 0]))
    out.append(_geo(7, "table", T=1, window=TABLE_WINDOW))
    for i, fam, kw in ((1, "randn", dict(window=64)), (2, "big", {}), (4, "small", dict(window=64)),
                       (5, "cancel", dict(window=64)), (6, "randn", {}), (8, "cancel", {}),
                       (9, "big", dict(window=64)), (11, "small", {}), (0, "randn", {})):
        out.append(_geo(i, fam, **kw))
    # q/k norm: D = 32, 64, 128, 256 (two loop trips around the butterfly)
    out += [_geo(1, "randn", norm=True), _geo(7, "randn", norm=True, window=64),
            _geo(9, "big", norm=True, eps=1e-5), _geo(5, "small", norm=True, window=64),
            _geo(11, "randn", norm=True, window=64), _geo(11, "cancel", norm=True, T=1)]
    for ks, vs in ((1.0, 1.0), (0.5, 0.5), (0.3, 0.3), (0.3, 1.0)):
        out += [_geo(1, "fp8edge", k_scale=ks, v_scale=vs),
                _geo(4, "fp8edge", k_scale=ks, v_scale=vs),
                _geo(6, "fp8edge_t", k_scale=ks, v_scale=vs)]
    for S in (1, 8):
        for pdt in ("f32", "bf16"):
            out += [_geo(6 if S == 1 else 2, "coord", parts=(S, pdt)),
                    _geo(3 if S == 1 else 8, "coord1", parts=(S, pdt), window=64)]
    out += [_geo(6, "randn", parts=(3, "f32"), window=64), _geo(4, "randn", parts=(3, "f32")),
            _geo(7, "randn", parts=(3, "f32"), norm=True)]
    assert len({c.ident() for c in out}) == len(out)
    return out


def gemv_cases():
    """The GEMV epilogue: M = T in {1, 2} rows (no q_sink there).  The table family's position
    list is walked in steps of two, so that every clamp is met."""
    out = []
    scales = (1.0, 0.5, 0.3)
    i = 0
    for nh, nkv, D in ((4, 2, 32), (9, 3, 64), (14, 2, 128)):
        for bs in (16, 64):
            g = dict(nh=nh, nkv=nkv, D=D, bs=bs)
            out += [Case(family="coordn", T=2, pos_shift=i, **g),
                    Case(family="coord1", T=1 + i % 2, pos_shift=i + 1, **g),
                    Case(family="table", T=2, pos_shift=2 * i, **g),
                    Case(family="table", T=1 + i % 2, pos_shift=(2 * i + 5) % 11, **g),
                    Case(family="fp8edge", T=1, k_scale=scales[i % 3], v_scale=scales[i % 3], **g),
                    Case(family="fp8edge_t", T=2, k_scale=scales[(i + 1) % 3],
                         v_scale=scales[(i + 2) % 3], **g)]
            i += 1
    return out


def ids(cs):
    return [c.ident() for c in cs]
