"""Exact-product cases, fp64 oracles, derived bounds and a tile emulator for the dense GEMM family
(csrc/kernels/gemm_tile.hip, gemm4.hip, gemv.hip and the split-K reduce), shared by
test_gemm_oracle_cpu.py (the cases' own conditions, the CPU branches of ops, mutations) and
test_gemm_exact_gpu.py (the HIP kernels, on guarded outputs).

Exact cases.  Operands are sparse small integers (codes of the operand format) and every scale is
a power of two, so every product is an integer multiple of one power of two ``u`` and
``max(|x| @ |w|^T) / u < 2^24``: every product and every partial sum, in any order, is exact in
fp32.  For the tile kernels every output (and every split-K partial) is also exactly
representable in bf16, so the kernel's result equals the fp64 product BIT FOR BIT whatever its
lane maps and summation order -- as long as they are the right ones.  The GEMV weight cases carry
every magnitude code of their format (e4m3: multiples of 2^-9), so their outputs are held to the
weaker but still order-free form: the fp32 sum is exact, the result is the fp64 product rounded
once to bf16.  The builders assert these conditions and lower the density until they hold.
No symmetry hides a mistake: all rows of an operand differ, no row or k index is all zero, and
the power-of-two scales differ between neighbours (r ^ 1), between rows / channels 16 apart (the
rows one MFMA lane owns) and between neighbouring MX k-blocks.

Real-valued cases.  bf16 / fp8 / int8 codes from fixed seeds, fp64 oracle ``o`` of the
dequantised product, and per element

    |y - o| <= 2^-8 (1 + 2^-6) |o| + c 2^-24 S,     S = sum_k |a_k| |b_k|   (scales included)

The first term is the final bf16 rounding (half an ulp at the low edge of a binade, with room for
the fp32 error of the epilogue's scale multiplies).  The second is the fp32 accumulation: a sum of
K terms in ANY order errs by at most (K - 1) 2^-24 S.

  MFMA tile kernels (gemm_tile, gemm4, + splitk_reduce): c = 2 K.  Twice the worst case of any
      summation order, because the MFMA's internal rounding is unspecified.
  GEMVs: c = the longest chain of dependent fp32 roundings an output passes through.  A lane owns
      one 16-byte weight vector per k-step and accumulates it with v_dot2c_f32_bf16 (two products
      per instruction: counted as 2 roundings, its internal rounding being unspecified), then the
      64 lanes are summed by a 6-level butterfly, the scales are multiplied in (<= 2) and the
      bias is added (1):
        skinny_gemm        8 bf16 / vector, 512 k per step:   c = 8 ceil(K / 512) + 9
        skinny_gemm_fp8   16 bytes / vector, 1024 k per step: c = 16 ceil(K / 1024) + 9
        skinny_gemm_fp4   32 nibbles / vector, 2048 k / step: c = 32 ceil(K / 2048) + 9
      (all K / 64 + 9 at multiples of the step.)
  skinny_gemm_int8: the kernel biases every weight byte to unsigned and computes
      sum_k x_k (q_k + 128) - 128 sum_k x_k, both sums in fp32, subtracted per lane.  What it
      accumulates is therefore not |x| |q| but |x| (q + 128) <= |x| (|q| + 128), plus the
      correction's 128 |x|: together at most 2 |x| (|q| + 128).  Its contract is the WEAKER
          S_int8 = ws sum_k |x_k| (|q_k| + 128),      c = 2 (16 ceil(K / 1024) + 10)
      (one more rounding for the subtraction; the factor 2 is the second sum).  For a zero-mean
      x the two terms stay small; for x with a mean (family ``offset``) the bound is dominated by
      128 ws sum |x| whatever the weights are -- an all-zero weight row gives |y| up to that
      term's rounding error instead of 0.

SwiGLU epilogues: gate and up are the exact integers (|gate| <= 40), the expected value is
silu(g) * u in fp64 under row_oracle's silu bound, and the fused epilogue must still equal the
unfused ``bf16 store -> ops.swiglu_interleaved`` path bit for bit.

The emulator (:func:`emulate_tile`, :func:`emulate_gemv`) forms the product through the
documented decomposition -- 256 x 256 tiles, 128-byte k-tiles, ``kps = ceil(kt / splits)``, the
XCD block remap, the grouped tile order, scales in the epilogue, the outlier term in split 0,
``swiglu_interleave`` pairing -- and takes a named fault.  It exists for the CPU self-test: every
fault in ``TILE_FAULTS`` / ``GEMV_FAULTS`` must be rejected by the checker on the case named
there (test_gemm_oracle_cpu.py prints the table).
"""
import dataclasses
import zlib
from typing import Optional

import torch

from distributed_llm_inference import ops
from row_oracle import silu_bound, silu_mul_oracle

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
G = 4096          # guard elements on each side of every output
SENT_BYTE = 0xA5  # guard fill (bf16 0xA5A5, fp32 0xA5A5A5A5: finite, never a result here)
KB = {"bf16": 64, "fp8": 128, "int8": 128, "mx": 128}   # elements of one 128-byte k-tile


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def e_row(r):
    """Power-of-two exponent pattern in {-1, 0, 1}: differs between r and r ^ 1 and r, r + 16."""
    return (r + r // 16) % 3 - 1


def e_col(n):
    return (n + n // 16 + 1) % 3 - 1


def is_bf16(t: torch.Tensor) -> bool:
    return bool((t.to(BF).double() == t).all())


def granule(t: torch.Tensor) -> float:
    """Largest power of two every element of ``t`` is an integer multiple of."""
    for q in range(-8, 40):
        s = t * 2.0 ** q
        if bool((s == s.round()).all()):
            return 2.0 ** -q
    raise AssertionError("operand is not on a power-of-two grid")


def sparse_ints(shape, p, key, vals=(1,)):
    """fp64 [R, C]: +-vals with probability p, else 0; every column and every row is non-zero
    somewhere (coverage of every k index / no dead row)."""
    g = _gen("sparse", shape, key)
    R, C = shape
    mag = torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), shape, generator=g)]
    sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    t = (torch.rand(shape, generator=g) < p).double() * mag * sgn
    c = torch.arange(C)
    r = (c * 7 + 3) % R
    t[r, c] = torch.where(t[r, c] == 0, sgn[r, c], t[r, c])
    r = torch.arange(R)
    c = (r * 5 + 1) % C
    t[r, c] = torch.where(t[r, c] == 0, sgn[r, c], t[r, c])
    return t


def assert_asymmetric(t: torch.Tensor, what: str):
    assert bool((t != 0).any(1).all()), f"{what}: an all-zero row"
    assert bool((t != 0).any(0).all()), f"{what}: a k index that is zero in every row"
    assert torch.unique(t, dim=0).shape[0] == t.shape[0], f"{what}: two equal rows"


# ===================================================================================== tile cases
@dataclasses.dataclass
class TileCase:
    """One product of the tile kernels.  ``araw`` [M, K] / ``braw`` [N, K]: the operand codes as
    fp64; ``sa`` [M] / ``sb`` [N]: epilogue scales (1 for bf16, whose scales sit in ``braw``);
    ``emx`` [M, K / 128]: MX exponents (precision ``mx``); ``xo`` [M, J] / ``wo`` [N, J]: bf16
    outlier operands (int8), of which the kernel multiplies ``ceil(live / 32) * 32`` columns when
    ``dynamic`` (the rest holds garbage) and all J otherwise."""
    name: str
    prec: str
    araw: torch.Tensor
    braw: torch.Tensor
    sa: torch.Tensor
    sb: torch.Tensor
    emx: Optional[torch.Tensor] = None
    xo: Optional[torch.Tensor] = None
    wo: Optional[torch.Tensor] = None
    live: int = 0
    dynamic: bool = False
    exact: bool = True

    @property
    def M(self):
        return self.araw.shape[0]

    @property
    def N(self):
        return self.braw.shape[0]

    @property
    def K(self):
        return self.araw.shape[1]

    @property
    def kt(self):
        return self.K // KB[self.prec]

    def a_deq(self, emx=None):
        a = self.araw * self.sa[:, None]
        e = self.emx if emx is None else emx
        if e is not None:
            a = a * torch.exp2(e.double()).repeat_interleave(128, 1)
        return a

    def b_deq(self):
        return self.braw * self.sb[:, None]

    def jl(self):
        """Outlier columns the epilogue multiplies."""
        if self.xo is None:
            return 0
        J = self.xo.shape[1]
        return min(J, (self.live + 31) // 32 * 32) if self.dynamic else J

    def outlier_term(self):
        if self.xo is None or self.jl() == 0:
            return 0.0
        j = self.jl()
        return self.xo[:, :j] @ self.wo[:, :j].t()


def split_ranges(kt: int, splits: int):
    """k-tile range [lo, hi) of every split: ``kps = ceil(kt / splits)`` (launch_tile)."""
    kps = -(-kt // splits)
    assert (splits - 1) * kps < kt, "every split owns at least one k-tile"
    return [(s * kps, min(kt, (s + 1) * kps)) for s in range(splits)]


def split_sums(c: TileCase, splits: int) -> torch.Tensor:
    """fp64 [S, M, N]: the exact partial product of every split, the outlier term in split 0."""
    a, b, kb = c.a_deq(), c.b_deq(), KB[c.prec]
    parts = torch.stack([a[:, lo * kb:hi * kb] @ b[:, lo * kb:hi * kb].t()
                         for lo, hi in split_ranges(c.kt, splits)])
    parts[0] += c.outlier_term()
    return parts


def oracle(c: TileCase) -> torch.Tensor:
    return c.a_deq() @ c.b_deq().t() + c.outlier_term()


def abs_sum(c: TileCase) -> torch.Tensor:
    s = c.a_deq().abs() @ c.b_deq().abs().t()
    if c.jl():
        s = s + c.xo[:, :c.jl()].abs() @ c.wo[:, :c.jl()].abs().t()
    return s


def swiglu_oracle(p: torch.Tensor):
    """(gate, up, silu(gate) * up) in fp64 from a product whose columns follow swiglu_interleave:
    tile-local column = wave (4) x pair (2) x {gate, up} x 16 lanes."""
    M, n2 = p.shape
    v = p.reshape(M, n2 // 256, 4, 2, 2, 16)
    g, u = v[..., 0, :].reshape(M, n2 // 2), v[..., 1, :].reshape(M, n2 // 2)
    return g, u, silu_mul_oracle(g, u)


def assert_exact(c: TileCase, splits=(1,), gate40: bool = False):
    """The conditions of an exact case (module docstring), on the CPU."""
    u = granule(c.a_deq()) * granule(c.b_deq())
    s = abs_sum(c)
    assert float(s.max()) / u < 2 ** 24, (c.name, "a partial sum may be inexact in fp32")
    o = oracle(c)
    assert is_bf16(o), (c.name, "an output is not a bf16 value")
    for sp in splits:
        if sp > 1:
            assert is_bf16(split_sums(c, sp)), (c.name, sp, "a split-K partial is not a bf16 value")
    assert bool((o != 0).any()), c.name
    assert_asymmetric(c.araw, c.name + " x")
    assert_asymmetric(c.braw, c.name + " w")
    if c.prec != "bf16":
        assert bool((c.sa[:-1] != c.sa[1:]).all() or c.M == 1 or c.prec == "mx"), c.name
        assert bool((c.sb[:-1] != c.sb[1:]).all()), c.name
    if c.emx is not None:
        e = c.emx
        assert bool((e[:-1] != e[1:]).all()) and (e.shape[1] == 1 or bool((e[:, :-1] != e[:, 1:]).all()))
    if gate40:
        g, _, _ = swiglu_oracle(o)
        assert float(g.abs().max()) <= 40, (c.name, "|gate| > 40")


_X_VALS = {"bf16": (1,), "fp8": (1, 1, 1, 2), "int8": (1, 1, 1, 2), "mx": (1, 1, 1, 2)}
_W_VALS = {"bf16": (1,), "fp8": (1, 1, 1, 2, 3, 4), "int8": (1, 1, 2, 3), "mx": (1, 1, 1, 2, 4)}
_TILE_CACHE = {}


def tile_case(prec: str, M: int, N: int, kt: int, splits=(1,), J: int = 0, live: int = 0,
              dynamic: bool = False, gate40: bool = False) -> TileCase:
    """The exact case of one shape, built once: the densest of a fixed ladder that meets
    :func:`assert_exact` (the CPU assertion decides)."""
    key = (prec, M, N, kt, tuple(splits), J, live, dynamic, gate40)
    if key in _TILE_CACHE:
        return _TILE_CACHE[key]
    K = kt * KB[prec]
    name = f"{prec}-M{M}-N{N}-kt{kt}" + (f"-J{J}-live{live}{'d' if dynamic else ''}" if J else "")
    err = None
    for p in (1 / 6, 1 / 12, 1 / 24, 1 / 48, 1 / 96, 1 / 192):
        # SwiGLU cases stay ternary: |gate| <= 40 after scales of up to 2^2
        araw = sparse_ints((M, K), p, (key, "x"), (1,) if gate40 else _X_VALS[prec])
        braw = sparse_ints((N, K), p, (key, "w"), (1,) if gate40 else _W_VALS[prec])
        r, n = torch.arange(M), torch.arange(N)
        sa, sb = torch.ones(M, dtype=torch.float64), torch.exp2(e_col(n).double())
        emx = None
        if prec == "bf16":
            braw, sb = braw * sb[:, None], torch.ones(N, dtype=torch.float64)
        elif prec == "mx":
            kb = torch.arange(kt)
            emx = (r[:, None] + r[:, None] // 16 + 2 * kb[None, :]) % 3 - 1
        else:
            sa = torch.exp2(e_row(r).double())
        if prec == "int8" and not J and not gate40:   # +-127 in both operands, against ternary columns of the other
            braw[n % 9 == 4, 11] = -127.0
            braw[n % 9 == 2, 11] = 127.0
            araw[:, 11] = araw[:, 11].clamp(-1, 1)
            if M > 1:   # rows that carry +-127 stay out of the weights' +-127 column
                braw[:, 5] = braw[:, 5].clamp(-1, 1)
                big = r % 7 == 0
                araw[big, 5] = torch.where(r[big] % 2 == 0, 127.0, -127.0).double()
                araw[big, 11] = 0.0
                araw[1, 11] = 1.0
        c = TileCase(name, prec, araw, braw, sa, sb, emx)
        if J:
            c.xo = sparse_ints((M, J), 0.2, (key, "xo"), (1, 2))
            c.wo = sparse_ints((N, J), 0.2, (key, "wo"), (1,))
            c.live, c.dynamic = live, dynamic
            c.xo[:, live:] = 0.0
            c.wo[:, live:] = 0.0
            if dynamic and c.jl() < J:   # stale columns of an earlier product: must be ignored
                c.xo[:, c.jl():] = 7777.0
                c.wo[:, c.jl():] = -3.0
        try:
            assert_exact(c, splits, gate40)
        except AssertionError as e:
            err = e
            continue
        _TILE_CACHE[key] = c
        return c
    raise AssertionError(f"no density makes {name} exact: {err}")


# ------------------------------------------------------------------------------ real-valued cases
TILE_FAMILIES = ("gauss", "positive", "spike", "scale_spread")
_AMP = {"bf16": 1.0, "fp8": 1.0, "int8": 30.0, "mx": 1.0}


def _codes(v: torch.Tensor, prec: str) -> torch.Tensor:
    """fp32 values -> the nearest code of the operand format, as fp64."""
    if prec == "bf16":
        return v.to(BF).double()
    if prec == "int8":
        return v.round().clamp(-127, 127).double()
    return v.clamp(-448, 448).to(F8).double()


def _family(fam: str, R: int, K: int, prec: str, key, kb: int, rows_are_weights: bool):
    g = torch.randn((R, K), generator=_gen("fam", fam, R, K, prec, key), dtype=torch.float32)
    amp = _AMP[prec]
    if fam == "positive":
        v = g.abs() * amp
    elif fam == "spike":
        v = g * (1.0 if prec == "int8" else 1e-3)
        r = torch.arange(R)
        kt, ch = K // kb, kb // 8
        # across the rows every k-tile and every 16-byte chunk of a k-tile receives a spike
        k = (r % kt) * kb + ((r + r // kt) % 8) * ch + r % ch
        v[r, k] = torch.where(r % 2 == 0, 300.0, -300.0)
    else:
        v = g * amp
    if prec == "bf16" and rows_are_weights and fam != "spike":
        v = v / K ** 0.5
    return _codes(v, prec)


def real_tile_case(prec: str, fam: str, M: int, N: int, kt: int) -> TileCase:
    key = ("real", prec, fam, M, N, kt)
    if key in _TILE_CACHE:
        return _TILE_CACHE[key]
    K, kb = kt * KB[prec], KB[prec]
    araw = _family(fam, M, K, prec, "x", kb, False)
    braw = _family(fam, N, K, prec, "w", kb, True)
    g = _gen("scales", key)
    spread = fam == "scale_spread"

    def scales(n):
        if spread:
            return torch.exp2(torch.randint(-6, 7, (n,), generator=g).float()) * \
                (1 + 0.25 * torch.rand(n, generator=g))
        return (0.5 + torch.rand(n, generator=g)) / 16.0
    one = torch.ones
    sa = one(M, dtype=torch.float64) if prec in ("bf16", "mx") else scales(M).float().double()
    sb = one(N, dtype=torch.float64) if prec == "bf16" else scales(N).float().double()
    emx = None
    if prec == "mx":
        lo, hi = (-6, 7) if spread else (-1, 2)
        emx = torch.randint(lo, hi, (M, kt), generator=g)
    if prec == "bf16" and spread:   # the spread sits in the operands themselves
        araw = _codes((araw * scales(M)[:, None].double()).float(), prec)
        braw = _codes((braw * scales(N)[:, None].double()).float(), prec)
    c = TileCase(f"{prec}-{fam}-M{M}-N{N}-kt{kt}", prec, araw, braw, sa, sb, emx, exact=False)
    _TILE_CACHE[key] = c
    return c


def tile_bound(c: TileCase) -> torch.Tensor:
    """The per-element bound of a real-valued tile case (c = 2 K)."""
    return 2.0 ** -8 * (1 + 2.0 ** -6) * oracle(c).abs() + 2 * c.K * 2.0 ** -24 * abs_sum(c)


# ------------------------------------------------------------------------------- device operands
def mx_pack(emx: torch.Tensor) -> torch.Tensor:
    """e8m0 bytes in gemm_tile.hip's mx_off layout; pad rows of the last 64-row block hold 127."""
    M, kt = emx.shape
    nb = (M + 63) // 64
    sc = torch.full((kt, nb * 64), 127, dtype=torch.uint8)
    r = torch.arange(M)
    sc[:, (r // 64) * 64 + (r % 16) * 4 + (r % 64) // 16] = (emx + 127).to(torch.uint8).t()
    return sc.view(-1)


def tile_operands(c: TileCase, dev) -> dict:
    """The tensors the kernels take, on ``dev``."""
    f32 = lambda t: t.float().contiguous().to(dev)   # noqa: E731
    if c.prec == "bf16":
        d = dict(a=c.araw.to(BF), b=c.braw.to(BF))
        assert bool((d["a"].double() == c.araw).all() and (d["b"].double() == c.braw).all())
    elif c.prec == "int8":
        d = dict(a=c.araw.to(torch.int8), b=c.braw.to(torch.int8), sa=f32(c.sa), sb=f32(c.sb))
    else:
        d = dict(a=c.araw.float().to(F8), b=c.braw.float().to(F8), sb=f32(c.sb))
        assert bool((d["a"].double() == c.araw).all() and (d["b"].double() == c.braw).all())
        if c.prec == "fp8":
            d["sa"] = f32(c.sa)
        else:
            d["a_mx"] = mx_pack(c.emx).to(dev)
    d["a"], d["b"] = d["a"].contiguous().to(dev), d["b"].contiguous().to(dev)
    if c.xo is not None:
        d["xo"], d["wo"] = c.xo.to(BF).contiguous().to(dev), c.wo.to(BF).contiguous().to(dev)
        if c.dynamic:
            d["cnt"] = torch.tensor([c.live], dtype=torch.int32, device=dev)
    return d


def guarded(shape, dtype, dev):
    """(buffer, view): the view is the output, G sentinel elements lie on each side of it."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(G + n + G, dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(SENT_BYTE)
    return buf, buf[G:G + n].view(*shape)


def guard_ok(buf: torch.Tensor, n: int) -> bool:
    b = buf.view(torch.uint8).cpu()
    e = buf.element_size()
    return bool((b[:G * e] == SENT_BYTE).all() and (b[(G + n) * e:] == SENT_BYTE).all())


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ============================================================================== the tile emulator
def remap(b: int, n: int, off_by_one: bool = False) -> int:
    """gemm_tile.hip's XCD block remap: physical block b of an n-block grid -> logical id.
    ``off_by_one``: the count of XCDs that run one more block is one short."""
    x, q, r = b & 7, n >> 3, n & 7
    if off_by_one:
        r = max(r - 1, 0)
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (b >> 3)


def grouped_tile(tile: int, tiles_m: int, tiles_n: int, GM: int = 8, ragged_fault: bool = False):
    """(tm, tn) of the grouped tile order: groups of up to GM M-tiles x all N panels."""
    gper = GM * tiles_n
    grp, grem = tile // gper, tile % gper
    gm = GM if ragged_fault else min(GM, tiles_m - grp * GM)
    return grp * GM + grem % gm, grem // gm


TILE_FAULTS = {
    # fault: (case builder arguments, splits, epilogue) on which the checker must reject it
    "drop_last_ktile": (("bf16", 65, 256, 5, (2,)), 2, 0),
    "start_one_ktile_early": (("fp8", 65, 256, 7, (3,)), 3, 1),
    "swap_chunks_in_a": (("bf16", 65, 256, 2), 1, 0),
    "ktile_offset_a_only": (("int8", 65, 256, 5, (2,)), 2, 4),
    "a_scale_row_xor_1": (("fp8", 300, 256, 1), 1, 0),
    "b_scale_chan_xor_1": (("fp8", 65, 256, 1), 1, 0),
    "b_scale_chan_plus_16": (("int8", 65, 256, 2), 1, 0),
    "mx_scale_next_kblock": (("mx", 65, 256, 2), 1, 0),
    "mx_scale_row_xor_1": (("mx", 257, 256, 1), 1, 0),
    "mx_pad_row_scale": (("fp8", 65, 256, 1, (1,), 0, 0, False, True), 1, 3),
    "ragged_group_tm_tn": (("bf16", 2309, 512, 1), 1, 0),
    "remap_remainder_off_by_one": (("bf16", 300, 256, 5, (5,)), 5, 1),
    "outlier_in_every_split": (("int8", 65, 256, 3, (3,), 32, 3, False), 3, 1),
    "dead_outlier_chunk": (("int8", 65, 256, 1, (1,), 64, 3, True), 1, 0),
    "swap_gate_up_one_pair": (("bf16", 65, 256, 1, (1,), 0, 0, False, True), 1, 2),
    "store_row_m": (("bf16", 65, 256, 1), 1, 0),
}


def emulate_tile(c: TileCase, splits: int = 1, epi: int = 0, fault: Optional[str] = None) -> dict:
    """The kernels' result through the documented decomposition, in fp64 and rounded where the
    kernel rounds.  Returns ``out`` (epilogue 0 / 2: bf16 [M, N] / [M, N / 2]; 1: fp32 and 4:
    bf16 partials [S, M, N]; 3: e4m3 bytes) with ``sc`` (epilogue 3) and ``guard`` (False when
    something was stored outside the output)."""
    M, N, kb, kt = c.M, c.N, KB[c.prec], c.kt
    tiles_m, tiles_n = (M + 255) // 256, N // 256
    tiles = tiles_m * tiles_n
    kps = -(-kt // splits)
    grid = tiles * splits
    parts = torch.full((splits, M + 1, N), float("nan"), dtype=torch.float64)   # row M: guard
    a_codes = c.araw
    if fault == "swap_chunks_in_a":   # 16-byte chunks 0 and 1 of every k-tile, A only
        ch = kb // 8
        a_codes = c.araw.clone().view(M, kt, 8, ch)
        a_codes[:, :, [0, 1]] = a_codes[:, :, [1, 0]]
        a_codes = a_codes.reshape(M, c.K)
    emx = c.emx
    if emx is not None:
        if fault == "mx_scale_next_kblock":
            emx = emx.roll(-1, 1)
        if fault == "mx_scale_row_xor_1":
            emx = emx[(torch.arange(M) ^ 1).clamp(max=M - 1)]
        a_codes = a_codes * torch.exp2(emx.double()).repeat_interleave(128, 1)
    for b in range(grid):
        lid = remap(b, grid, fault == "remap_remainder_off_by_one")
        if lid >= grid:
            continue
        tile, split = lid % tiles, lid // tiles
        tm, tn = grouped_tile(tile, tiles_m, tiles_n, 8, fault == "ragged_group_tm_tn")
        if tm >= tiles_m or tn >= tiles_n:
            continue
        m0, n0 = tm * 256, tn * 256
        kt0 = split * kps
        T = min(kps, kt - kt0)
        if fault == "drop_last_ktile" and split == splits - 1:
            T -= 1
        if fault == "start_one_ktile_early" and split > 0:
            kt0, T = kt0 - 1, T + 1
        ktb = 0 if fault == "ktile_offset_a_only" else kt0
        rows = (m0 + torch.arange(256)).clamp(max=M - 1)   # rows past M: computed, never stored
        cols = n0 + torch.arange(256)
        acc = a_codes[rows, kt0 * kb:(kt0 + T) * kb] @ c.braw[cols, ktb * kb:(ktb + T) * kb].t()
        srow = (rows ^ 1).clamp(max=M - 1) if fault == "a_scale_row_xor_1" else rows
        scol = cols
        if fault == "b_scale_chan_xor_1":
            scol = cols ^ 1
        if fault == "b_scale_chan_plus_16":
            scol = (cols + 16) % N
        acc = acc * c.sb[scol][None, :] * c.sa[srow][:, None]
        if c.xo is not None and (split == 0 or fault == "outlier_in_every_split"):
            j = c.xo.shape[1] if fault == "dead_outlier_chunk" else c.jl()
            if j:
                acc = acc + c.xo[rows, :j] @ c.wo[cols, :j].t()
        nrow = min(256, M - m0)
        parts[split, m0:m0 + nrow, n0:n0 + 256] = acc[:nrow]
        if fault == "store_row_m" and m0 + nrow == M:
            parts[split, M, n0:n0 + 256] = acc[nrow - 1]
    res = {"guard": bool(torch.isnan(parts[:, M]).all())}
    parts = parts[:, :M]
    if epi == 1:
        res["out"] = parts.float()
    elif epi == 4:
        res["out"] = parts.float().to(BF)
    else:
        y = parts.sum(0).float().to(BF)   # fp32 sum (exact here), one bf16 rounding
        if epi == 0:
            res["out"] = y
        else:
            v = y.double().reshape(M, N // 256, 4, 2, 2, 16)
            if fault == "swap_gate_up_one_pair":
                v = v.clone()
                v[:, 0, 0, 0] = v[:, 0, 0, 0].flip(1)
            h = silu_mul_oracle(v[..., 0, :], v[..., 1, :]).reshape(M, N // 2).float().to(BF)
            if epi == 2:
                res["out"] = h
            else:
                q = ops.mx_quantize(h)
                sc = q.sc.clone()
                if fault == "mx_pad_row_scale":
                    nb = (M + 63) // 64
                    r = torch.arange(M, nb * 64)
                    sc.view(-1, nb * 64)[:, (r // 64) * 64 + (r % 16) * 4 + (r % 64) // 16] = 0
                res["out"], res["sc"] = q.q.view(torch.uint8), sc
    return res


def check_tile(c: TileCase, res: dict, splits: int = 1, epi: int = 0) -> list:
    """Problems of a result (``emulate_tile``'s dict, or the same made from a kernel's outputs)
    against the fp64 oracle: bit-equal for an exact case, the bound for a real-valued one."""
    bad = []
    if not res.get("guard", True):
        bad.append("a store outside the output")
    out = res["out"].cpu()
    if epi in (1, 4):
        want = split_sums(c, splits)
    else:
        want = oracle(c)
    if epi in (0, 1, 4):
        if tuple(out.shape) != tuple(want.shape):
            return bad + [f"shape {tuple(out.shape)} != {tuple(want.shape)}"]
        if c.exact:
            w = want.float() if epi == 1 else want.float().to(BF)
            n = int((bits(out) != bits(w)).sum())
            if n or not bool(torch.isfinite(out.float()).all()):
                bad.append(f"{n} elements differ from the exact product")
        else:
            y = out.double().sum(0) if epi in (1, 4) else out.double()
            o = oracle(c)
            bound = tile_bound(c)
            if epi == 4:   # one more bf16 rounding per partial
                bound = bound + 2.0 ** -8 * split_sums(c, splits).abs().sum(0)
            q = torch.nan_to_num((y - o).abs() / bound, nan=float("inf"))
            res["ratio"] = float(q.max())
            if res["ratio"] > 1.0:
                bad.append(f"err / bound = {res['ratio']:.3g}")
    else:
        g, u, o = swiglu_oracle(want)
        if epi == 2:
            h = out.double()
        else:   # MX fp8 bytes + scales: against the reference quantiser of the exact h's bf16
            h = ops.MxFp8(out.view(F8), res["sc"].cpu()).dequantize().double()
            ref = ops.mx_quantize(silu_mul_oracle(g, u).float().to(BF))
            nb = (c.M + 63) // 64
            r = torch.arange(c.M, nb * 64)
            pad = (r // 64) * 64 + (r % 16) * 4 + (r % 64) // 16
            if not bool((res["sc"].cpu().view(-1, nb * 64)[:, pad] == 127).all()):
                bad.append("a pad-row scale is not 127")
            if res["sc"].numel() != ref.sc.numel():
                bad.append("scale buffer size")
        if tuple(h.shape) != tuple(o.shape):
            return bad + [f"shape {tuple(h.shape)} != {tuple(o.shape)}"]
        # e4m3 keeps 3 mantissa bits: half an ulp is 2^-4 relative; half a subnormal step
        # is 2^-10 of a block scale that is below amax / 224
        bound = silu_bound(o) if epi == 2 else (
            (2.0 ** -4 + 2.0 ** -7) * o.abs()
            + 2.0 ** -17 * o.abs().view(c.M, -1, 128).amax(-1).repeat_interleave(128, 1) + 1e-38)
        q = torch.nan_to_num(torch.where(h == o, 0.0, (h - o).abs() / bound), nan=float("inf"))
        if float(q.max()) > 1.0:
            bad.append(f"silu(gate) * up: err / bound = {float(q.max()):.3g}")
    return bad


# =========================================================================================== GEMV
GEMV_FORMATS = ("bf16", "fp8", "fp8x", "int8", "fp4")   # fp8x: fp8 rows as well
GEMV_MIN_K = {"bf16": 8, "fp8": 16, "fp8x": 16, "int8": 16, "fp4": 32}
GEMV_GROUP = {"bf16": 2048, "fp8": 4096, "fp8x": 4096, "int8": 4096, "fp4": 4096}   # one unrolled group
GEMV_VEC = {"bf16": 8, "fp8": 16, "fp8x": 16, "int8": 16, "fp4": 32}
GEMV_STEP = {"bf16": 512, "fp8": 1024, "fp8x": 1024, "int8": 1024, "fp4": 2048}
GEMV_MAX_M = {"bf16": 4, "fp8": 2, "fp8x": 2, "int8": 2, "fp4": 2}
E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)


def gemv_ks(fmt: str):
    g = GEMV_GROUP[fmt]
    return (GEMV_MIN_K[fmt], g, g + GEMV_VEC[fmt], 8192)


def gemv_c(fmt: str, K: int) -> int:
    """Chain length of the module docstring."""
    n = GEMV_VEC[fmt] * -(-K // GEMV_STEP[fmt])
    return 2 * (n + 10) if fmt == "int8" else n + 9


@dataclasses.dataclass
class GemvCase:
    """``xraw`` [M, K] / ``xs`` [M]: row codes and scales (scales 1 unless fp8x); ``wraw`` [N, K]
    the weight codes' VALUES (fp4: block scales included), ``ws`` [N] row scales; ``bias`` [N].
    ``dev``: the tensors the kernel takes (CPU)."""
    name: str
    fmt: str
    xraw: torch.Tensor
    xs: torch.Tensor
    wraw: torch.Tensor
    ws: torch.Tensor
    bias: Optional[torch.Tensor]
    dev: dict
    swiglu: bool = False
    exact: bool = True

    @property
    def M(self):
        return self.xraw.shape[0]

    @property
    def N(self):
        return self.wraw.shape[0]

    @property
    def K(self):
        return self.xraw.shape[1]

    def x_deq(self):
        return self.xraw * self.xs[:, None]

    def w_deq(self):
        return self.wraw * self.ws[:, None]


def gemv_oracle(c: GemvCase) -> torch.Tensor:
    return c.x_deq() @ c.w_deq().t() + (c.bias if c.bias is not None else 0.0)


def gemv_abs_sum(c: GemvCase) -> torch.Tensor:
    w = c.wraw.abs() + 128.0 if c.fmt == "int8" else c.wraw.abs()
    s = c.x_deq().abs() @ (w * c.ws[:, None].abs()).t()
    return s + (c.bias.abs() if c.bias is not None else 0.0)


def gemv_bound(c: GemvCase) -> torch.Tensor:
    return (2.0 ** -8 * (1 + 2.0 ** -6) * gemv_oracle(c).abs()
            + gemv_c(c.fmt, c.K) * 2.0 ** -24 * gemv_abs_sum(c))


def gemv_swiglu_rows(N: int):
    """(gate rows, up rows) of the GEMV SwiGLU epilogue: output column o takes weight row
    32 (o // 16) + o % 16 as its gate and the row 16 further as its up (gemv_core.h)."""
    o = torch.arange(N // 2)
    g = 32 * (o // 16) + o % 16
    return g, g + 16


def _gemv_weights(fmt: str, N: int, K: int, key, real=None, plant: bool = True):
    """(wraw values fp64, ws fp64, device tensors)."""
    g = _gen("gemv-w", fmt, N, K, key)
    n = torch.arange(N)
    ws = torch.exp2(e_col(n).double()) if real is None else real["ws"]
    if fmt == "bf16":
        w = sparse_ints((N, K), 0.5, (key, "w")) * ws[:, None] if real is None else real["w"]
        return w, torch.ones(N, dtype=torch.float64), dict(w=w.to(BF))
    if fmt in ("fp8", "fp8x"):
        if real is None and not plant:   # SwiGLU: integer codes, so gate and up are bf16 values
            w8 = sparse_ints((N, K), 0.5, (key, "w"), (1, 1, 2, 4)).float().to(F8)
        elif real is None:   # every magnitude code up to 4.0, and each larger one planted once
            byte = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
            byte = (byte & 0x80) | ((byte & 0x7F) % 0x49)
            flat = byte.view(-1)
            if flat.numel() >= 4096 and plant:
                pos = torch.randperm(flat.numel(), generator=g)[:0x7F - 0x49]
                flat[pos] = torch.arange(0x49, 0x7F, dtype=torch.uint8) | (flat[pos] & 0x80)
            w8 = byte.view(F8)
        else:
            w8 = real["w"].clamp(-448, 448).float().to(F8)
        return w8.float().double(), ws, dict(w=w8, ws=ws.float())
    if fmt == "int8":
        if real is None:
            w = sparse_ints((N, K), 0.5, (key, "w"), (1, 1, 2))
            if plant:
                w[n % 3 == 1, (n[n % 3 == 1] * 5) % K] = 127.0
                w[n % 3 == 2, (n[n % 3 == 2] * 5) % K] = -127.0
        else:
            w = real["w"].round().clamp(-127, 127).double()
        return w, ws, dict(w=w.to(torch.int8), ws=ws.float())
    # fp4: every nibble code, block scales 2^-1 .. 2^1 that differ between neighbouring blocks
    if real is None:
        code = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
        blk = torch.arange(K // 32)
        eb = (n[:, None] + n[:, None] // 16 + 2 * blk[None, :]) % 3 - 1
    else:
        pk, sc = ops.quantize_weight_mxfp4(real["w"].float())
        code = torch.stack([pk & 0xF, pk >> 4], -1).reshape(N, K)
        eb = sc.to(torch.int32) - 127
    w = E2M1[code.long()] * torch.exp2(eb.double()).repeat_interleave(32, 1)
    packed = (code.view(N, K // 2, 2)[..., 0] | (code.view(N, K // 2, 2)[..., 1] << 4)).contiguous()
    return w, torch.ones(N, dtype=torch.float64), dict(w=packed, ws=(eb + 127).to(torch.uint8))


_GEMV_CACHE = {}


def gemv_case(fmt: str, M: int, N: int, K: int, bias: bool = False, swiglu: bool = False,
              nonneg_x: bool = False) -> GemvCase:
    """An exact GEMV case: integer rows, format codes as weights, power-of-two scales, integer
    bias.  ``nonneg_x``: all x >= 0 (the int8 kernel's 128 sum x term is large and must cancel
    exactly).  ``swiglu``: sparse enough that |gate| <= 40."""
    key = (fmt, M, N, K, bias, swiglu, nonneg_x)
    if key in _GEMV_CACHE:
        return _GEMV_CACHE[key]
    err = None
    for p in ((1 / 24, 1 / 96, 1 / 384, 1 / 1536, 1 / 6144) if swiglu else (0.5, 1 / 8, 1 / 32)):
        x = sparse_ints((M, K), p, (key, "x"), (1,) if swiglu else (1, 1, 2))
        if nonneg_x:
            x = x.abs()
        xs = torch.ones(M, dtype=torch.float64)
        dev = {}
        if fmt == "fp8x":
            xs = torch.exp2(e_row(torch.arange(M)).double() + 1)
            dev["xs"] = xs.float()
            dev["x"] = x.float().to(F8)
        else:
            dev["x"] = x.to(BF)
        wraw, ws, wd = _gemv_weights(fmt, N, K, key, plant=not swiglu)
        if swiglu:   # thin the weights too: the gate is a sum over K
            keep = torch.rand((N, K), generator=_gen(key, "keep")) < 4 * p
            if fmt in ("bf16", "int8"):
                wraw = wraw * keep
                wd["w"] = wraw.to(wd["w"].dtype)
            elif fmt == "fp4":
                code = torch.stack([wd["w"] & 0xF, wd["w"] >> 4], -1).reshape(N, K) * keep
                wd["w"] = (code.view(N, K // 2, 2)[..., 0] | (code.view(N, K // 2, 2)[..., 1] << 4)).contiguous()
                wraw = wraw * keep
            else:
                wd["w"] = (wd["w"].view(torch.uint8) * keep).view(F8)
                wraw = wraw * keep
        dev.update(wd)
        b = None
        if bias:
            b = ((torch.arange(N) * 5) % 13 - 6).double()
            dev["bias"] = b.to(BF)
        c = GemvCase(f"gemv-{fmt}-M{M}-N{N}-K{K}" + ("-b" if bias else "") + ("-sw" if swiglu else "")
                     + ("-pos" if nonneg_x else ""), fmt, x, xs, wraw, ws, b, dev, swiglu)
        try:
            u = granule(c.x_deq()) * granule(c.w_deq())
            lim = gemv_abs_sum(c).max() if fmt != "int8" else \
                (c.xraw.abs() @ (c.wraw + 128).t()).max() + 128 * c.xraw.abs().sum(1).max()
            assert float(lim) / u < 2 ** 24, "a partial sum may be inexact in fp32"
            assert bool((x != 0).any(0).all()) and bool((x != 0).any(1).all())
            assert M == 1 or torch.unique(x, dim=0).shape[0] == M
            if swiglu:
                gr, _ = gemv_swiglu_rows(N)
                assert float(gemv_oracle(c)[:, gr].abs().max()) <= 40, "|gate| > 40"
                assert is_bf16(gemv_oracle(c)), "gate or up is not a bf16 value"
        except AssertionError as e:
            err = e
            continue
        _GEMV_CACHE[key] = c
        return c
    raise AssertionError(f"no density makes gemv {key} exact: {err}")


GEMV_FAMILIES = ("gauss", "positive", "spike", "scale_spread")


def real_gemv_case(fmt: str, fam: str, M: int, N: int, K: int, bias: bool = True) -> GemvCase:
    key = ("real", fmt, fam, M, N, K, bias)
    if key in _GEMV_CACHE:
        return _GEMV_CACHE[key]
    g = _gen("gemv-real", key)
    gx = torch.randn((M, K), generator=g)
    gw = torch.randn((N, K), generator=g)
    amp = 30.0 if fmt == "int8" else 1.0
    if fam == "positive":
        gx, gw = gx.abs(), gw.abs()
    if fam == "spike":
        r, n = torch.arange(M), torch.arange(N)
        gx, gw = gx * 1e-3, gw * (1.0 / amp if fmt == "int8" else 1e-3)
        gx[r, (r * 521 + 7) % K] = 300.0
        gw[n, (n * 1031 + K - 1) % K] = -300.0 / (1.0 if fmt != "int8" else 300.0 / 127.0) / amp
    if fam == "offset":
        gx = 3.0 + 0.1 * gx
        gw = (gw * 1.2) / amp
        gw[N // 2] = 0.0
    gw = gw * amp
    spread = fam == "scale_spread"
    ws = (torch.exp2(torch.randint(-6, 7, (N,), generator=g).float()) if spread
          else (0.5 + torch.rand(N, generator=g)) / 64).float().double()
    xs = torch.ones(M, dtype=torch.float64)
    dev = {}
    if fmt == "fp8x":
        xs = (torch.exp2(torch.randint(-6, 7, (M,), generator=g).float()) if spread
              else 0.5 + torch.rand(M, generator=g)).float().double()
        dev["x"], dev["xs"] = gx.clamp(-448, 448).to(F8), xs.float()
        x = dev["x"].float().double()
    else:
        if spread:
            gx = gx * torch.exp2(torch.randint(-6, 7, (M, 1), generator=g).float())
        dev["x"] = gx.to(BF)
        x = dev["x"].double()
    if fmt in ("bf16", "fp4"):
        gw = gw * ws[:, None].float() / (K ** 0.5 if fmt == "bf16" else 1.0)
    if fmt == "bf16":
        gw = gw.to(BF).double()
    wraw, ws, wd = _gemv_weights(fmt, N, K, key, real=dict(w=gw, ws=ws))
    dev.update(wd)
    b = None
    if bias:
        dev["bias"] = torch.randn(N, generator=g).to(BF)
        b = dev["bias"].double()
    c = GemvCase(f"gemv-{fmt}-{fam}-M{M}-N{N}-K{K}", fmt, x, xs, wraw, ws, b, dev, exact=False)
    _GEMV_CACHE[key] = c
    return c


GEMV_FAULTS = {
    # fault: arguments of gemv_case on which the checker must reject it
    "drop_last_partial_kstep": ("bf16", 1, 7, 2056, False),
    "store_row_1_of_last_wave_at_odd_n": ("fp8", 2, 7, 16, False),
    "sum_x_of_row_0_for_row_1": ("int8", 2, 8, 4112, False, False, True),
    "bias_from_n_minus_1": ("fp4", 1, 9, 32, True),
}


def emulate_gemv(c: GemvCase, fault: Optional[str] = None) -> dict:
    """A wave per 2 weight rows, lanes stride K by one vector per k-step, zero-filled past K."""
    x, w = c.x_deq(), c.w_deq()
    K = c.K
    if fault == "drop_last_partial_kstep":
        K = K // GEMV_STEP[c.fmt] * GEMV_STEP[c.fmt]
    if c.fmt == "int8":   # the offset trick, with the kernel's grouping
        acc = x[:, :K] @ (c.wraw[:, :K] + 128).t()
        sx = x[:, :K].sum(1)
        if fault == "sum_x_of_row_0_for_row_1":
            sx = sx[[0] * c.M]
        y = (acc - 128 * sx[:, None]) * c.ws[None, :]
    else:
        y = x[:, :K] @ w[:, :K].t()
    if c.bias is not None:
        y = y + (c.bias.roll(1) if fault == "bias_from_n_minus_1" else c.bias)
    out = torch.full((c.M, c.N + 1), float("nan"), dtype=torch.float64)   # column N: guard
    out[:, :c.N] = y
    if fault == "store_row_1_of_last_wave_at_odd_n" and c.N % 2:
        out[:, c.N] = y[:, c.N - 1]
    res = {"guard": bool(torch.isnan(out[:, c.N]).all())}
    y = out[:, :c.N].float().to(BF)
    if c.swiglu:
        gr, ur = gemv_swiglu_rows(c.N)
        y = silu_mul_oracle(y[:, gr].double(), y[:, ur].double()).float().to(BF)
    res["out"] = y
    return res


def check_gemv(c: GemvCase, res: dict) -> list:
    bad = []
    if not res.get("guard", True):
        bad.append("a store outside the output")
    y = res["out"].cpu()
    o = gemv_oracle(c)
    if c.swiglu:
        gr, ur = gemv_swiglu_rows(c.N)
        assert c.exact
        o = silu_mul_oracle(o[:, gr], o[:, ur])
        if tuple(y.shape) != tuple(o.shape):
            return bad + ["shape"]
        q = torch.nan_to_num(torch.where(y.double() == o, 0.0, (y.double() - o).abs() / silu_bound(o)),
                             nan=float("inf"))
        if float(q.max()) > 1.0:
            bad.append(f"silu(gate) * up: err / bound = {float(q.max()):.3g}")
        return bad
    if tuple(y.shape) != tuple(o.shape):
        return bad + [f"shape {tuple(y.shape)} != {tuple(o.shape)}"]
    if c.exact:
        n = int((bits(y) != bits(o.to(BF))).sum())
        if n:
            bad.append(f"{n} elements differ from the exact product rounded to bf16")
    else:
        q = torch.nan_to_num((y.double() - o).abs() / gemv_bound(c), nan=float("inf"))
        res["ratio"] = float(q.max())
        if res["ratio"] > 1.0:
            bad.append(f"err / bound = {res['ratio']:.3g}")
    return bad


def run_gemv_ops(c: GemvCase, dev="cpu") -> torch.Tensor:
    """The case through the public ops entry points (the CPU branches on ``dev`` = cpu)."""
    d = {k: v.to(dev) for k, v in c.dev.items()}
    b = d.get("bias")
    if c.fmt == "bf16":
        return ops.skinny_gemm(d["x"], d["w"], b, swiglu=c.swiglu)
    if c.fmt in ("fp8", "fp8x"):
        return ops.skinny_gemm_fp8(d["x"], d["w"], d["ws"], d.get("xs"), b, swiglu=c.swiglu)
    if c.fmt == "int8":
        return ops.skinny_gemm_int8(d["x"], d["w"], d["ws"], b, swiglu=c.swiglu)
    return ops.skinny_gemm_fp4(d["x"], d["w"], d["ws"], b, swiglu=c.swiglu)


# ================================================================================== split-K reduce
def reduce_case(splits: int, MN: int):
    """(fp32 parts [S, 1, MN], exact bf16 sum): integers whose sum is a bf16 value."""
    g = _gen("reduce", splits, MN)
    parts = torch.randint(-15, 16, (splits, 1, MN), generator=g).float()
    i = torch.arange(MN)
    parts[0, 0] += ((i * 7 + i // 8) % 5).float() - 2   # position-dependent: a shifted read shows
    want = parts.double().sum(0)
    assert is_bf16(want) and float(parts.abs().sum(0).max()) < 2 ** 24
    return parts, want.to(BF)


# ================================================================= the shapes both test files use
TILE_PRECS = ("bf16", "fp8", "int8", "mx")
TILE_MS = (1, 65, 256, 257, 300)      # 65 / 257 / 300 end inside a 64-row MX scale block
TILE_NS = (256, 768)
TILE_KTS = (1, 2, 3, 5)
# (M, N, k-tiles, splits): 3 + 2, 3 + 3 + 1 and 8 x 1 k-tiles; tiles * splits = 3, 10, 21 (no
# multiple of 8: the XCD remap's remainder path), 16 and 4 (a partial M tile)
SPLIT_SPECS = ((65, 256, 7, 3), (65, 1280, 5, 2), (1, 1792, 7, 3), (300, 256, 8, 8), (257, 256, 5, 2))
LONG_KT = {"bf16": 128, "fp8": 64, "int8": 64, "mx": 64}    # M = 1, N = 256, K = 8192
GROUPED_MS = (2309, 2049)             # tiles_m = 10 / 9: the ragged group holds 2 / 1 M-tiles
MX_MAX_KPS = (65, 256, 64)            # the largest legal k-tiles per split, once
# (J, live columns, dynamic cnt)
OUTLIER_COMBOS = ((32, 0, False), (32, 3, False), (32, 0, True), (32, 3, True), (64, 3, False),
                  (64, 33, False), (64, 0, True), (64, 3, True), (64, 33, True))
OUTLIER_MS = (65, 300)
SWIGLU_SPECS = ((65, 512, 2), (300, 512, 1))   # (M, 2I, k-tiles)
REAL_MS, REAL_KTS, REAL_SPLITS = (65, 300), (5, 64), (1, 3)
GEMV_NS = (1, 2, 7, 8, 9, 33)
GEMV_SWIGLU_NS = (32, 96)
REDUCE_SPECS = ((1, 8), (2, 8), (8, 8), (1, 2056), (2, 2056), (8, 2056), (2, 4096 * 256 * 8 + 8))


def exact_tile_specs(prec: str):
    """Arguments of :func:`tile_case` for every exact case of one precision."""
    out = [(prec, M, N, kt) for M in TILE_MS for N in TILE_NS for kt in TILE_KTS]
    out += [(prec, M, N, kt, (sp,)) for M, N, kt, sp in SPLIT_SPECS]
    out.append((prec, 1, 256, LONG_KT[prec]))
    if prec in ("bf16", "fp8"):
        out += [(prec, M, 512, 1) for M in GROUPED_MS]
    if prec == "mx":
        out.append((prec,) + MX_MAX_KPS)
    else:
        out += [(prec, M, N, kt, (1,), 0, 0, False, True) for M, N, kt in SWIGLU_SPECS]
    if prec == "int8":
        out += [(prec, M, 256, 3, (3,), J, live, dyn, True)
                for M in OUTLIER_MS for J, live, dyn in OUTLIER_COMBOS]
    return out


def exact_gemv_specs(fmt: str):
    """Arguments of :func:`gemv_case` for every exact case of one format."""
    out = [(fmt, M, N, K, b) for N in GEMV_NS for K in gemv_ks(fmt)
           for M in range(1, GEMV_MAX_M[fmt] + 1) for b in (False, True)]
    out += [(fmt, M, N, K, False, True) for N in GEMV_SWIGLU_NS for K in gemv_ks(fmt)[:3]
            for M in (1, 2)]
    if fmt == "int8":
        out += [(fmt, 2, N, K, False, False, True) for N in (7, 8) for K in gemv_ks(fmt)]
    return out


def real_gemv_specs(fmt: str):
    fams = GEMV_FAMILIES + (("offset",) if fmt == "int8" else ())
    ks = (GEMV_GROUP[fmt] + GEMV_VEC[fmt] // 2 * 2 + (8 if fmt == "bf16" else 0), 8192)
    return [(fmt, fam, M, 33, K) for fam in fams for K in (gemv_ks(fmt)[2], 8192)
            for M in (1, GEMV_MAX_M[fmt])] if ks else []
