"""fp64 oracles, inputs and derived bounds for the row-per-workgroup and element-wise kernels
(norm.hip, quant.hip's quant_rowwise / silu_mul_quant / quant_rowwise_int8, activation.hip),
shared by test_row_oracle_cpu.py (ops/reference.py and the CPU paths of ops against the bounds,
mutations) and test_row_kernels_gpu.py (the HIP kernels against the same bounds).

Every oracle returns the UNROUNDED fp64 result ``o``.  The only rounding an oracle performs is
``r = bf16(x + res)`` (one fp32 add of two bf16 values and one rounding: bit-determined) and, for
split-K partials, the fp32 sum in split order rounded to bf16 (the documented contract of
common.h load_row_vecs).  ``eps`` is the fp32 value the launchers receive.

Bounds.  A bf16 rounding errs by at most 2^-8 relative (half an ulp of an 8-bit significand at
the low edge of a binade).  The kernels round once, from fp32 arithmetic whose error is far below
2^-16 relative (sums of <= 16384 terms: <= 64 sequential adds per thread, then a tree):

  rms       |y - o| <= 2^-8 (1 + 2^-8) |o| + 1e-38
  ln        |y - o| <= 2^-8 (1 + 2^-8) |o| + 2^-20 (|(r - mean) rstd w| + |b|)
                       + 2^-16 |w| rstd mean|r|
            (the last term: a thread sums up to 64 values before the tree, so ``mean`` is off by
            up to 2^-18 mean|r|; 4x margin.  It is what a constant row is held to.)
  silu_mul  |y - o| <= 2^-8 (1 + 2^-6) |o| + 1e-38 for gates >= -80; below that the output is
            finite and |y| <= 1e-30 |u|
  gelu      |y - o| <= 2^-8 (1 + 2^-6) |o| + 2^-22 |t|   (fp32 cancellation in 1 + tanh, t < 0)
  add, residual_out: bit-equal to bf16(fp32(a) + fp32(b))
  fp8 rows  scale: |s - s_o| <= 2^-22 s_o where the quantised row is an exact bf16 tensor (amax
            is exact; 4 ulp for a division that may not be correctly rounded), 2^-8 (1 + 2^-6)
            s_o where a bf16 rounding precedes the quantiser (norm, silu_mul);
            values, y = q s: |y - o| <= (2^-4 + 2^-7) |o| + 2^-10 (1 + 2^-6) s_o
            (e4m3: 3 mantissa bits, half an ulp is 2^-4 relative; half a subnormal step is
            2^-10 s); no NaN code; the row's largest element encodes to +-448; an all-zero row
            gives scale 1 and zeros
  codes     where the quantised row is an exact bf16 tensor (fp8) and for int8, every code is
            compared with the fp64 code of x / s_o: a mismatch must be to the adjacent code and
            only where x / s_o is within 2^-20 relative of the midpoint of the two; at most 1%
            of a case may mismatch.

The scale oracle is ``max(amax / 448, FLT_MIN)`` (int8: / 127), 1 for an all-zero row: the floor
keeps 1 / scale finite for rows whose amax is below ~1.3e-36 (family ``denorm``).

Inputs are bf16 from fixed seeds, 6 rows per case (64 at width 8 for the quantisers, where one
tie among 48 codes would already be 2% of the case).  Families: gauss, heavy (g exp(2 g')),
offset (100 + 0.1 g), big (1e4 g), tiny (1e-20 g: eps-dominant), const (ln), spike (1e-3 g and
one +-300 per row, at the positions of spike_elems), zero_row, denorm (1e-37 g times 0.03 .. 3
per row, every fifth element 0), edges (SwiGLU gates at and past the range of exp).
"""
import dataclasses
import functools
import zlib
from typing import Optional, Tuple

import numpy as np
import torch

from distributed_llm_inference import ops

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
FLT_MIN = 2.0 ** -126
ROWS = 6

NORM_WIDTHS = (8, 520, 2056, 5120, 10248, 16384)
QUANT_WIDTHS = (8, 520, 4104, 8200, 28672, 32776, 65544)
EW_WIDTHS = (8, 520, 8000)
EW_BIG = (70, 65536)            # rows x width / 8 > 2048 x 256: the grid-stride loop's 2nd trip
INTERLEAVED_I = (128, 384, 3584)
PARTS_WIDTHS = (520, 10248)
# (threads, VPT) each width list must reach: test_row_oracle_cpu.py asserts these sets
NORM_ARMS = {(64, 1), (128, 1), (256, 2), (256, 4), (256, 8)}
QUANT_ARMS = {(64, 1), (128, 1), (256, 4), (320, 4), (896, 4), (1024, 8), (1024, 16)}


# ------------------------------------------------------------------------------ launcher arms
def _arm(vpt: int, arms) -> Optional[int]:
    return next((a for a in arms if vpt <= a), None)


def norm_threads(hidden: int) -> int:
    """csrc/kernels/norm.hip norm_threads."""
    nvec = hidden // 8
    return min(256, (nvec + 63) // 64 * 64)


def norm_arm(hidden: int):
    """(threads, vectors a thread really holds, VPT instantiated) of norm.hip's launchers
    (NORM_DISPATCH / RMS_LAUNCH_PB); VPT None: rejected."""
    nvec, t = hidden // 8, norm_threads(hidden)
    vpt = (nvec + t - 1) // t
    return t, vpt, _arm(vpt, (1, 2, 4, 8))


def row_threads(nvec: int) -> int:
    """csrc/kernels/quant.hip row_threads."""
    t = ((nvec + 3) // 4 + 63) // 64 * 64
    if t < 256:
        t = min((nvec + 63) // 64 * 64, 256)
    return min(t, 1024)


def quant_arm(K: int):
    """(threads, vectors per thread, VPT instantiated) of quant.hip's launchers."""
    nvec = K // 8
    t = row_threads(nvec)
    vpt = (nvec + t - 1) // t
    return t, vpt, _arm(vpt, (1, 2, 4, 8, 16))


def spike_elems(H: int, threads: int, vpt: int, rows: int = ROWS):
    """One spike position per row: element 0, element H - 1, the last element of lane 63 of wave
    0, the first of wave 1, the last valid vector, a vector in the last slot a thread holds
    (vector index = thread + slot * threads).  Positions the row is too short for fall away;
    the rest are cycled over the rows."""
    nvec = H // 8
    last_slot = (vpt - 1) * threads
    cand = [0, H - 1, 63 * 8 + 7, 64 * 8, (nvec - 1) * 8,
            (last_slot + min(5, nvec - 1 - last_slot)) * 8 + 3]
    cand = list(dict.fromkeys(c for c in cand if 0 <= c < H))
    return [cand[i % len(cand)] for i in range(rows)]


# ------------------------------------------------------------------------------------- inputs
def _randn(shape, *key):
    gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    return torch.randn(shape, generator=gen, dtype=torch.float32)


CONSTS = (3.0, -0.75, 100.0, 1e-3, -1e4, 0.0)
DENORM_ROW = (1.0, 1.0, 0.3, 0.1, 3.0, 0.03)


def family(name: str, H: int, arm, key, rows: int = ROWS) -> torch.Tensor:
    """bf16 [rows, H] of one input family; ``arm`` = (threads, vectors per thread) places the
    spikes."""
    g = _randn((rows, H), name, H, key, 0)
    if name in ("gauss", "zero_row"):
        x = g
        if name == "zero_row":
            x[2] = 0.0
    elif name == "heavy":
        x = g * torch.exp(2.0 * _randn((rows, H), name, H, key, 1))
    elif name == "offset":
        x = 100.0 + 0.1 * g
    elif name == "big":
        x = 1e4 * g
    elif name == "tiny":
        x = 1e-20 * g
    elif name == "const":
        x = torch.tensor([CONSTS[r % len(CONSTS)] for r in range(rows)])[:, None]
        x = x.expand(rows, H).clone()
    elif name == "spike":
        x = 1e-3 * g
        for r, e in enumerate(spike_elems(H, *arm, rows)):
            x[r, e] = 300.0 if r % 2 == 0 else -300.0
    elif name == "denorm":
        f = torch.tensor([DENORM_ROW[r % len(DENORM_ROW)] for r in range(rows)])
        x = (1e-37 * g.double() * f.double()[:, None]).float()
        x[:, ::5] = 0.0
    else:
        raise ValueError(name)
    return x.to(BF)


@dataclasses.dataclass(frozen=True)
class Case:
    kernel: str                     # rms ln silu_mul silu_il gelu add quant silu_mul_quant int8
    H: int                          # row width (I for the SwiGLU kernels)
    family: str = "gauss"
    residual: bool = False
    norm: bool = False              # quant: fused RMSNorm
    eps: float = 1e-5
    wkind: str = "near1"            # 1 + 0.1 g | 'gauss': w, b ~ g
    parts: Optional[Tuple[int, str]] = None     # split-K partials (S, 'f32' | 'bf16')
    mask: bool = False              # int8: outlier columns
    bias: bool = True               # gelu
    rows: int = ROWS

    def ident(self):
        s = f"{self.kernel}-{self.H}-{self.family}"
        s += "-res" if self.residual else ""
        s += "-norm" if self.norm else ""
        s += f"-{self.wkind}" if self.wkind != "near1" else ""
        s += f"-eps{self.eps:g}" if self.kernel in ("rms", "ln") or self.norm else ""
        s += f"-S{self.parts[0]}{self.parts[1]}" if self.parts else ""
        s += "-mask" if self.mask else ""
        s += "" if self.bias else "-nobias"
        return s + (f"-r{self.rows}" if self.rows != ROWS else "")

    @property
    def arm(self):
        t, vpt, _ = norm_arm(self.H) if self.kernel in ("rms", "ln") else quant_arm(self.H)
        return t, vpt


def sum_parts(parts: torch.Tensor) -> torch.Tensor:
    """fp32 sum in split order 0..S-1, rounded to bf16 once (common.h load_row_vecs)."""
    acc = parts[0].float()
    for k in range(1, parts.shape[0]):
        acc = acc + parts[k].float()
    return acc.to(BF)


def bf16_add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (a.float() + b.float()).to(BF)


def il_columns(I: int):
    """(gate column, up column) of every output column of the interleaved SwiGLU row, from the
    comment of activation.hip: output column o = 128 t + 32 w + 16 p + l has its gate at
    256 t + 64 w + 32 p + l and its up 16 columns later."""
    o = np.arange(I)
    t, w, p, l = o // 128, (o % 128) // 32, (o % 32) // 16, o % 16
    gc = 256 * t + 64 * w + 32 * p + l
    return torch.from_numpy(gc), torch.from_numpy(gc + 16)


def il_columns_from_src(I: int):
    """The same map from ops._swiglu_src: interleaved column c holds column src[c] of the fused
    [gate | up] row."""
    src = ops._swiglu_src(2 * I, torch.device("cpu"))
    inv = torch.empty(2 * I, dtype=torch.long)
    inv[src] = torch.arange(2 * I)
    return inv[:I], inv[I:]


# deep and ordinary gates alternate, so that even an 8-wide row has a well-defined scale
GATE_EDGES = (-80.0, 80.0, -88.0, 20.0, -1e4, 0.0, -89.0, 100.0, -84.0, 88.0, -87.5, 1e4,
              -88.5, -20.0, -100.0, -0.0)


@functools.lru_cache(maxsize=4)
def inputs(c: Case) -> dict:
    """The case's tensors (bf16, CPU).  Cached: treat as read-only."""
    k, H, arm = c.kernel, c.H, c.arm
    d = {}
    if k in ("silu_mul", "silu_il", "silu_mul_quant"):
        u = family("gauss" if c.family == "edges" else c.family, H, arm, "up", c.rows)
        g = family("heavy" if c.family == "heavy" else "gauss", H, arm, "gate", c.rows)
        if c.family == "spike":             # the product's spike sits where u's does
            for r, e in enumerate(spike_elems(H, *arm, c.rows)):
                g[r, e] = 4.0
        if c.family == "edges":             # gates at and beyond the range of exp
            ge = torch.tensor(GATE_EDGES, dtype=BF)
            g[:, :min(H, ge.numel())] = ge[:H]
        if k == "silu_il":
            x = torch.empty(c.rows, 2 * H, dtype=BF)
            gc, uc = il_columns(H)
            x[:, gc], x[:, uc] = g, u
        else:
            x = torch.cat([g, u], dim=1)
        d.update(x=x.contiguous(), gate=g, up=u)
        return d
    if c.parts is not None:
        S, pdt = c.parts
        full = family(c.family, H, arm, "parts", c.rows).float()
        p = full[None] / S + 0.05 * _randn((S, c.rows, H), "pn", H, S, pdt)
        d["parts"] = p.to(BF if pdt == "bf16" else torch.float32).contiguous()
        d["x"] = sum_parts(d["parts"])
    else:
        d["x"] = family(c.family, H, arm, "x", c.rows)
    if k == "add":
        d["res"] = family(c.family, H, arm, "b", c.rows)
    if c.residual:
        d["res"] = family("spike" if c.family == "spike" else c.family, H, arm, "res", c.rows)
        if c.family == "spike":             # background only: the sum keeps x's spike
            d["res"] = (1e-3 * _randn((c.rows, H), "sres", H)).to(BF)
    if k in ("rms", "ln") or c.norm:
        gw = _randn((H,), "w", H, c.wkind)
        d["w"] = (gw if c.wkind == "gauss" else 1.0 + 0.1 * gw).to(BF)
    if k == "ln":
        gb = _randn((H,), "b", H, c.wkind)
        d["b"] = (gb if c.wkind == "gauss" else 0.1 * gb).to(BF)
    if k == "gelu" and c.bias:
        d["b"] = _randn((H,), "gb", H).to(BF)
    if k == "int8" and c.mask:
        m = torch.zeros(H, dtype=torch.uint8)
        m[::37] = 1
        m[H - 1] = 1
        # the largest element of every other row sits in a masked column: it must not enter amax
        x = d["x"].clone()
        x[::2, 0] = x.float().abs().amax().item() * 4.0
        d["x"], d["mask"] = x, m
    return d


# ------------------------------------------------------------------------------------ oracles
def eps32(eps: float) -> float:
    return float(np.float32(eps))


def rms_oracle(r, w, eps):
    rd = r.double()
    return rd * torch.rsqrt((rd * rd).mean(-1, keepdim=True) + eps32(eps)) * w.double()


def ln_oracle(r, w, b, eps):
    """(o, bound) of LayerNorm."""
    rd, wd, bd = r.double(), w.double(), b.double()
    mean = rd.mean(-1, keepdim=True)
    var = ((rd - mean) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps32(eps))
    core = (rd - mean) * rstd * wd
    o = core + bd
    bound = (2.0 ** -8 * (1 + 2.0 ** -8) * o.abs() + 2.0 ** -20 * (core.abs() + bd.abs())
             + 2.0 ** -16 * wd.abs() * rstd * rd.abs().mean(-1, keepdim=True))
    return o, bound


def rms_bound(o):
    return 2.0 ** -8 * (1 + 2.0 ** -8) * o.abs() + 1e-38


def silu_mul_oracle(g, u):
    gd = g.double()
    return gd / (1.0 + torch.exp(-gd)) * u.double()


def silu_bound(o):
    return 2.0 ** -8 * (1 + 2.0 ** -6) * o.abs() + 1e-38


def gelu_oracle(x, b):
    """(o, bound)."""
    t = x.double() + (b.double() if b is not None else 0.0)
    k0, k1 = 0.7978845608028654, 0.044715
    o = 0.5 * t * (1.0 + torch.tanh(k0 * (t + k1 * t ** 3)))
    return o, 2.0 ** -8 * (1 + 2.0 ** -6) * o.abs() + 2.0 ** -22 * t.abs()


def scale_oracle(o, qmax: float):
    amax = o.abs().amax(-1)
    return torch.where(amax > 0, (amax / qmax).clamp_min(FLT_MIN), torch.ones_like(amax))


def e4m3_bytes(t: torch.Tensor) -> torch.Tensor:
    """fp64 -> e4m3fn byte, round to nearest even, saturating at +-448 (done in fp64: the
    result is exact in fp32, so the final cast only encodes)."""
    a = t.abs().clamp(max=448.0)
    _, ex = torch.frexp(a)
    step = torch.pow(2.0, ((ex - 1).clamp(min=-6) - 3).double())
    v = (torch.round(a / step) * step).clamp(max=448.0)
    return (torch.copysign(v, t)).float().to(F8).view(torch.uint8)


def f8_value(b: torch.Tensor) -> torch.Tensor:
    return b.view(F8).double()


def _ordinal(b: torch.Tensor) -> torch.Tensor:
    """Signed rank of an e4m3 byte among the finite codes (+-0 -> 0)."""
    m = (b & 0x7F).to(torch.int64)
    return torch.where((b & 0x80) != 0, -m, m)


# --------------------------------------------------------------------------------- evaluation
@dataclasses.dataclass
class Verdict:
    ratio: float = 0.0              # largest err / bound
    share: float = 0.0              # share of mismatching codes
    problems: list = dataclasses.field(default_factory=list)

    @property
    def ok(self):
        return self.ratio <= 1.0 and not self.problems


def _ratio(v: Verdict, what, y, o, bound):
    err = (y.double() - o).abs()
    q = torch.nan_to_num(torch.where(err == 0, err, err / bound), nan=float("inf"))
    m = float(q.max())
    v.ratio = max(v.ratio, m)
    if m > 1.0:
        i = np.unravel_index(int(q.argmax()), q.shape)
        v.problems.append(f"{what}: err {float(err[i]):.4g} > bound {float(bound[i]):.4g} "
                          f"({m:.3g}x) at {tuple(int(j) for j in i)}: got {float(y[i]):.6g} "
                          f"want {float(o[i]):.6g}")


def _bits_equal(v: Verdict, what, a, b):
    if a.shape != b.shape or not torch.equal(a.view(torch.int16), b.view(torch.int16)):
        n = int((a.view(torch.int16) != b.view(torch.int16)).sum()) if a.shape == b.shape else -1
        v.problems.append(f"{what}: not bit-equal ({n} elements differ)")


def _codes(v: Verdict, what, got, want, val, t):
    """Code-by-code: ``got`` / ``want`` integer ranks, ``val(rank)`` their values, t = x / s_o."""
    mis = got != want
    v.share = max(v.share, float(mis.double().mean()))
    if v.share > 0.01:
        v.problems.append(f"{what}: {v.share:.3%} of the codes differ from the fp64 codes (> 1%)")
    if not mis.any():
        return
    g, w, tt = got[mis], want[mis], t[mis]
    if ((g - w).abs() != 1).any():
        i = int(((g - w).abs() != 1).nonzero()[0])
        v.problems.append(f"{what}: code {int(g[i])} where {int(w[i])} is expected "
                          f"(x / s = {float(tt[i]):.9g}): not adjacent")
        return
    mid = (val(g) + val(w)) / 2
    far = (tt - mid).abs() > 2.0 ** -20 * mid.abs()
    if far.any():
        i = int(far.nonzero()[0])
        v.problems.append(f"{what}: code {int(g[i])} where {int(w[i])} is expected and x / s = "
                          f"{float(tt[i]):.9g} is no tie (midpoint {float(mid[i]):.9g})")


def _fp8_rows(v: Verdict, q, s, o, exact: bool):
    """q uint8 [rows, K], s fp32 [rows], o fp64 unrounded; exact: o is an exact bf16 tensor."""
    s = s.reshape(-1).double()
    s_o = scale_oracle(o, 448.0)
    tol = 2.0 ** -22 if exact else 2.0 ** -8 * (1 + 2.0 ** -6)
    _ratio(v, "scale", s, s_o, tol * s_o)
    mag = q & 0x7F
    if (mag == 0x7F).any():
        i = (mag == 0x7F).nonzero()[0].tolist()
        v.problems.append(f"NaN code at {i} ({int((mag == 0x7F).sum())} in all)")
        return
    y = f8_value(q) * s[:, None]
    _ratio(v, "values", y, o, (2.0 ** -4 + 2.0 ** -7) * o.abs()
           + 2.0 ** -10 * (1 + 2.0 ** -6) * s_o[:, None])
    amax = o.abs().amax(-1)
    zero = amax == 0
    if zero.any() and not (bool((s[zero] == 1.0).all()) and bool((mag[zero] == 0).all())):
        v.problems.append("an all-zero row must give scale 1.0 and zero codes")
    full = amax / 448.0 >= FLT_MIN          # rows whose scale is not floored
    top = (o.abs() == amax[:, None]) & full[:, None]
    if not bool((mag[top] == 0x7E).all()):
        v.problems.append("the row's largest element does not encode to +-448")
    if exact:
        t = o / s_o[:, None]
        _codes(v, "fp8 codes", _ordinal(q), _ordinal(e4m3_bytes(t)),
               lambda r: torch.copysign(f8_value(r.abs().to(torch.uint8)), r.double()), t)


def stage_oracle(c: Case, inp: dict):
    """(r, o, exact): the residual sum (or x), the unrounded value the quantiser sees, and
    whether o is an exact bf16 tensor."""
    r = bf16_add(inp["x"], inp["res"]) if c.residual else inp["x"]
    if c.kernel == "silu_mul_quant":
        return r, silu_mul_oracle(inp["gate"], inp["up"]), False
    if c.norm:
        return r, rms_oracle(r, inp["w"], c.eps), False
    return r, r.double(), True


def evaluate(c: Case, out: dict) -> Verdict:
    """``out``: what an implementation produced for ``inputs(c)``, CPU tensors: y (bf16), r (the
    residual sum it wrote), q (uint8 bytes / int8), s (fp32)."""
    v = Verdict()
    inp = inputs(c)
    k = c.kernel
    if c.residual:
        _bits_equal(v, "residual_out", out["r"], bf16_add(inp["x"], inp["res"]))
    if k == "rms":
        r, _, _ = stage_oracle(c, inp)
        o = rms_oracle(r, inp["w"], c.eps)
        _ratio(v, "rms", out["y"], o, rms_bound(o))
    elif k == "ln":
        r, _, _ = stage_oracle(c, inp)
        o, bound = ln_oracle(r, inp["w"], inp["b"], c.eps)
        _ratio(v, "ln", out["y"], o, bound)
    elif k in ("silu_mul", "silu_il"):
        g, u = inp["gate"], inp["up"]
        o = silu_mul_oracle(g, u)
        y = out["y"].double()
        deep = g.double() < -80.0
        _ratio(v, "silu_mul", torch.where(deep, o, y), o, silu_bound(o))
        if not bool(torch.isfinite(y[deep]).all()) or \
                not bool((y[deep].abs() <= 1e-30 * u.double()[deep].abs()).all()):
            v.problems.append("silu_mul: gate < -80 must give a finite |y| <= 1e-30 |u|")
    elif k == "gelu":
        o, bound = gelu_oracle(inp["x"], inp.get("b"))
        _ratio(v, "gelu", out["y"], o, bound)
    elif k == "add":
        _bits_equal(v, "add", out["y"], bf16_add(inp["x"], inp["res"]))
    elif k in ("quant", "silu_mul_quant"):
        _, o, exact = stage_oracle(c, inp)
        _fp8_rows(v, out["q"].view(torch.uint8), out["s"], o, exact)
    elif k == "int8":
        x = inp["x"].double()
        if c.mask:
            x = x * (inp["mask"] == 0).double()
        s_o = scale_oracle(x, 127.0)
        _ratio(v, "scale", out["s"].reshape(-1).double(), s_o, 2.0 ** -22 * s_o)
        q = out["q"].to(torch.int64)
        if c.mask and bool((q[:, inp["mask"] != 0] != 0).any()):
            v.problems.append("int8: a masked column is not 0")
        t = x / s_o[:, None]
        _codes(v, "int8 codes", q, torch.round(t).clamp(-127, 127).to(torch.int64),
               lambda r: r.double(), t)
    else:
        raise ValueError(k)
    return v


# -------------------------------------------------------------------------------- running ops
def run_ops(c: Case, dev, inp: Optional[dict] = None) -> dict:
    """The case through the ``ops`` front-end with its tensors on ``dev`` (CPU: ops/reference.py
    and the CPU paths of ops; split-K partials are pre-summed there, the CPU front-end has no
    partials path).  Returns CPU tensors."""
    inp = inputs(c) if inp is None else inp
    t = {n: (x.to(dev) if torch.is_tensor(x) else x) for n, x in inp.items()}
    on_gpu = torch.device(dev).type != "cpu"
    k = c.kernel
    x = t["x"]
    if c.parts is not None and on_gpu:
        x = ops.SplitKPartials(t["parts"])
    res = t.get("res") if c.residual else None
    r_out = torch.empty_like(res) if res is not None else None
    out = {}
    if k == "rms":
        out["y"], _ = ops.rms_norm(x, t["w"], c.eps, residual=res, residual_out=r_out)
    elif k == "ln":
        out["y"], _ = ops.layer_norm(x, t["w"], t["b"], c.eps, residual=res, residual_out=r_out)
    elif k == "silu_mul":
        out["y"] = ops.silu_mul(x)
    elif k == "silu_il":
        out["y"] = ops.swiglu_interleaved(x)
    elif k == "gelu":
        out["y"] = ops.gelu_bias(x, t.get("b"))
    elif k == "add":
        out["y"] = ops.add(x, t["res"])
    elif k == "quant":
        out["q"], out["s"] = ops.quant_rowwise(x, residual=res, norm_w=t.get("w"), eps=c.eps,
                                               residual_out=r_out)
    elif k == "silu_mul_quant":
        out["q"], out["s"] = ops.silu_mul_quant(x)
    elif k == "int8":
        out["q"], out["s"] = ops.quant_rowwise_int8(x, t.get("mask"))
    if r_out is not None:
        out["r"] = r_out
    return {n: (y.view(torch.uint8) if y.dtype == F8 else y).cpu() for n, y in out.items()}


# -------------------------------------------------------------------------------- case matrix
def _eps(i: int) -> float:
    return (1e-5, 1e-6)[i % 2]


def norm_cases(kind: str):
    out = []
    fams = ("gauss", "heavy", "offset", "big", "tiny", "spike")
    for H in NORM_WIDTHS:
        i = 0
        for fam in fams:
            for res in (False, True):
                out.append(Case(kind, H, fam, residual=res, eps=_eps(i)))
                i += 1
        out.append(Case(kind, H, "tiny", eps=1e-6))
        out.append(Case(kind, H, "tiny", residual=True, eps=1e-5))
        if kind == "ln":
            out.append(Case(kind, H, "const", eps=1e-5))
            out.append(Case(kind, H, "const", wkind="gauss", eps=1e-6))
            out.append(Case(kind, H, "gauss", wkind="gauss", residual=True, eps=1e-5))
            out.append(Case(kind, H, "offset", wkind="gauss", eps=1e-6))
    return out


def parts_cases(kind: str):
    """rms / quant with split-K partials as x."""
    out = []
    for H in PARTS_WIDTHS:
        for S in (1, 8):
            for pdt in ("f32", "bf16"):
                out.append(Case(kind, H, "gauss", parts=(S, pdt), eps=1e-5))
                out.append(Case(kind, H, "gauss", parts=(S, pdt), residual=True,
                                norm=kind == "quant", eps=1e-6))
    return out


def _qrows(H: int) -> int:
    """Rows of a quantiser case: 64 at H = 8, so that one exact tie among the codes is 0.2% of
    the case, not 2%."""
    return 64 if H == 8 else ROWS


def quant_cases():
    out = []
    for H in QUANT_WIDTHS:
        for fam in ("gauss", "heavy", "offset", "big", "tiny", "spike", "zero_row", "denorm"):
            out.append(Case("quant", H, fam, rows=_qrows(H)))
        for i, fam in enumerate(("gauss", "heavy", "tiny", "spike", "zero_row", "offset")):
            out.append(Case("quant", H, fam, norm=True, residual=i % 2 == 0, eps=_eps(i),
                            rows=_qrows(H)))
        out.append(Case("quant", H, "gauss", residual=True, rows=_qrows(H)))
        out.append(Case("quant", H, "denorm", residual=True, rows=_qrows(H)))
    return out


def silu_quant_cases():
    return [Case("silu_mul_quant", H, fam, rows=_qrows(H)) for H in QUANT_WIDTHS
            for fam in ("gauss", "heavy", "tiny", "spike", "zero_row", "edges")]


def int8_cases():
    out = []
    for H in QUANT_WIDTHS:
        for fam in ("gauss", "heavy", "offset", "big", "tiny", "spike", "zero_row", "denorm"):
            out.append(Case("int8", H, fam, rows=_qrows(H)))
        for fam in ("gauss", "spike", "denorm"):
            out.append(Case("int8", H, fam, mask=True, rows=_qrows(H)))
    return out


def elementwise_cases():
    out = []
    for H in EW_WIDTHS:
        for fam in ("gauss", "heavy", "big", "tiny", "edges"):
            out.append(Case("silu_mul", H, fam))
        for fam in ("gauss", "heavy", "offset", "big", "tiny"):
            out.append(Case("gelu", H, fam))
            out.append(Case("add", H, fam))
        out.append(Case("gelu", H, "gauss", bias=False))
    for I in INTERLEAVED_I:
        for fam in ("gauss", "heavy", "edges"):
            out.append(Case("silu_il", I, fam))
    rows, W = EW_BIG
    out += [Case(k, W, "gauss", rows=rows) for k in ("silu_mul", "gelu", "add")]
    return out


def all_cases():
    return (norm_cases("rms") + norm_cases("ln") + parts_cases("rms") + parts_cases("quant")
            + quant_cases() + silu_quant_cases() + int8_cases() + elementwise_cases())


def ids(cases):
    return [c.ident() for c in cases]
