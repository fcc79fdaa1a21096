"""The dense GEMM kernels (gemm_tile.hip, gemm4.hip, gemv.hip, the split-K reduce) against
gemm_oracle.py: exact-product cases bit for bit, real-valued families under their derived
per-element bounds.  Every output -- the fp32 split-K workspace, the bf16 partials and the MX
scale buffer included -- is a view into a buffer with 4096 sentinel elements on each side, which
must survive.  What the cases are and why a wrong kernel fails them: gemm_oracle.py's docstring
and the mutation table of test_gemm_oracle_cpu.py.

The real-valued tests print ``RATIO <kernel> <family> <largest err / bound>`` (pytest -s): a
record of how much room each bound leaves, not a threshold.
"""
import pytest
import torch

from distributed_llm_inference import ops

import gemm_oracle as go

pytestmark = pytest.mark.gpu
BF, F8 = go.BF, go.F8
_DEV = {}


def _operands(c, dev):
    if id(c) not in _DEV:   # the cases live in gemm_oracle's cache: one upload each
        _DEV[id(c)] = go.tile_operands(c, dev)
    return _DEV[id(c)]


def run_tile(c: go.TileCase, dev, splits: int = 1, epi: int = 0, kernel: str = "tile",
             grid: int = 0, var: int = -1) -> dict:
    """One launch on guarded outputs -> the dict gemm_oracle.check_tile takes."""
    nat = ops.native()
    d = _operands(c, dev)
    M, N = c.M, c.N
    bufs = []

    def out_of(shape, dtype):
        buf, view = go.guarded(shape, dtype, dev)
        n = 1
        for s in shape:
            n *= s
        bufs.append((buf, n))
        return view
    sc = None
    if epi == 3:
        out = out_of((M, N // 2), F8)
        sc = out_of((N // 2 // 128 * ((M + 63) // 64) * 64,), torch.uint8)
    elif epi in (1, 4):
        out = out_of((splits, M, N), torch.float32 if epi == 1 else BF)
    else:
        out = out_of((M, N // 2 if epi == 2 else N), BF)
    if kernel == "gemm4":
        nat.gemm4(out, d["a"], d["b"], splits, epi, grid, d.get("sa"), d.get("sb"), var,
                  a_mx=d.get("a_mx"), out_mx=sc)
    else:
        ws, c_out = None, out
        if epi == 1:
            ws, c_out = out.view(-1), torch.empty(M, 0, dtype=BF, device=dev)
        elif epi == 0 and splits > 1:
            ws = out_of((splits * M * N,), torch.float32)
        nat.gemm_tile(c_out, d["a"], d["b"], splits, epi, ws, d.get("sa"), d.get("sb"),
                      d.get("xo"), d.get("wo"), d.get("a_mx"), sc, d.get("cnt"))
    torch.cuda.synchronize()
    res = {"out": out.cpu(), "guard": all(go.guard_ok(b, n) for b, n in bufs), "dev_out": out}
    if sc is not None:
        res["sc"] = sc.cpu()
    if kernel == "tile" and epi == 0 and splits > 1:
        res["workspace"] = ws.view(splits, M, N).cpu()
    return res


def _check(c, res, splits=1, epi=0, what=""):
    bad = go.check_tile(c, res, splits, epi)
    assert not bad, (c.name, what, splits, epi, bad)


def _splits_of(a):
    return a[4][0] if len(a) > 4 else 1


# ================================================================================ gemm_tile, exact
@pytest.mark.parametrize("M", go.TILE_MS)
@pytest.mark.parametrize("prec", go.TILE_PRECS)
def test_gemm_tile_exact(gpu, prec, M):
    """Whole tiles and partial M tiles (65 / 257 / 300 end inside a 64-row MX scale block), one
    to five k-tiles (the prologue alone, both buffers, every tail of the k-loop)."""
    for N in go.TILE_NS:
        for kt in go.TILE_KTS:
            c = go.tile_case(prec, M, N, kt)
            _check(c, run_tile(c, gpu))


@pytest.mark.parametrize("spec", go.SPLIT_SPECS, ids=lambda s: "M%d-N%d-kt%d-s%d" % s)
@pytest.mark.parametrize("prec", go.TILE_PRECS)
def test_gemm_tile_exact_split_k(gpu, prec, spec):
    """3 + 2, 3 + 3 + 1 and 8 x 1 k-tiles; grids of 3, 10 and 21 blocks (the XCD remap's
    remainder path).  Reduced bf16 (and the fp32 workspace it leaves), fp32 partials and bf16
    partials: every split's slab is the exact partial product."""
    M, N, kt, sp = spec
    c = go.tile_case(prec, M, N, kt, (sp,))
    r = run_tile(c, gpu, sp, 0)
    _check(c, r, sp, 0)
    _check(c, {"out": r["workspace"]}, sp, 1, "workspace")
    _check(c, run_tile(c, gpu, sp, 1), sp, 1)
    _check(c, run_tile(c, gpu, sp, 4), sp, 4)


@pytest.mark.parametrize("prec", go.TILE_PRECS)
def test_gemm_tile_exact_long_k(gpu, prec):
    c = go.tile_case(prec, 1, 256, go.LONG_KT[prec])
    assert c.K == 8192
    _check(c, run_tile(c, gpu))


@pytest.mark.parametrize("M", go.GROUPED_MS)
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_gemm_tile_exact_grouped_tile_order(gpu, prec, M):
    """tiles_m = 10 / 9 > 8: the grouped order with a ragged last group of 2 / 1 M-tiles."""
    c = go.tile_case(prec, M, 512, 1)
    _check(c, run_tile(c, gpu))


def test_gemm_tile_exact_mx_largest_k_split(gpu):
    c = go.tile_case("mx", *go.MX_MAX_KPS)
    _check(c, run_tile(c, gpu))


@pytest.mark.parametrize("spec", go.SWIGLU_SPECS, ids=lambda s: "M%d-N%d-kt%d" % s)
@pytest.mark.parametrize("prec", ["bf16", "fp8", "int8"])
def test_gemm_tile_exact_swiglu(gpu, prec, spec):
    """Exact integer gate and up: silu(g) * u under the silu bound, the fused epilogue bit-equal
    to bf16 store -> swiglu_interleaved, and (fp8) the kSwiGLUMx producer's bytes and scales equal
    to ops.mx_quantize of that h, pad rows included."""
    c = go.tile_case(prec, *spec, (1,), 0, 0, False, True)
    y = run_tile(c, gpu)
    _check(c, y)
    h = run_tile(c, gpu, 1, 2)
    _check(c, h, 1, 2)
    assert torch.equal(h["dev_out"], ops.swiglu_interleaved(y["dev_out"].contiguous()))
    if prec == "fp8":
        a = run_tile(c, gpu, 1, 3)
        _check(c, a, 1, 3)
        ref = ops.mx_quantize(h["out"])
        assert torch.equal(a["sc"], ref.sc)
        assert torch.equal(a["out"].view(torch.uint8), ref.q.view(torch.uint8))


@pytest.mark.parametrize("J,live,dyn", go.OUTLIER_COMBOS)
@pytest.mark.parametrize("M", go.OUTLIER_MS)
def test_gemm_tile_exact_int8_outlier_epilogue(gpu, M, J, live, dyn):
    """The bf16 outlier product in the int8 epilogue: 0 / 3 / 33 live columns of J = 32 / 64,
    with the dynamic count (stale columns past the live chunks must be ignored) and without;
    plain store, SwiGLU, and split-K (the term in split 0 only) reduced and as partials."""
    c = go.tile_case("int8", M, 256, 3, (3,), J, live, dyn, True)
    y = run_tile(c, gpu)
    _check(c, y)
    h = run_tile(c, gpu, 1, 2)
    _check(c, h, 1, 2)
    assert torch.equal(h["dev_out"], ops.swiglu_interleaved(y["dev_out"].contiguous()))
    for epi in (0, 1, 4):
        _check(c, run_tile(c, gpu, 3, epi), 3, epi)


# ==================================================================================== gemm4, exact
_G4_RUNS = {"bf16": ((0, -1), (7, -1), (0, 4), (0, 6), (0, 8), (0, 9)),
            "fp8": ((0, -1), (7, -1)), "mx": ((0, -1), (7, -1))}


@pytest.mark.parametrize("prec,grid,var", [(p, g, v) for p, runs in _G4_RUNS.items() for g, v in runs])
def test_gemm4_exact(gpu, prec, grid, var):
    """gemm4 against the exact product itself (not only "equals gemm_tile"): every exact case,
    automatic and 7-block persistent grids, every k-loop schedule; M = 2309 as well."""
    specs = go.exact_tile_specs(prec)
    if prec == "mx":
        specs = specs + [("mx", 2309, 512, 1)]
    for a in specs:
        c = go.tile_case(*a)
        sp = _splits_of(a)
        if sp > 1:
            for epi in (1, 4):
                _check(c, run_tile(c, gpu, sp, epi, "gemm4", grid, var), sp, epi, (grid, var))
            continue
        y = run_tile(c, gpu, 1, 0, "gemm4", grid, var)
        _check(c, y, 1, 0, (grid, var))
        if len(a) > 8:   # SwiGLU cases
            h = run_tile(c, gpu, 1, 2, "gemm4", grid, var)
            _check(c, h, 1, 2, (grid, var))
            assert torch.equal(h["dev_out"], ops.swiglu_interleaved(y["dev_out"].contiguous()))
            if prec == "fp8":
                q = run_tile(c, gpu, 1, 3, "gemm4", grid, var)
                _check(c, q, 1, 3, (grid, var))
                ref = ops.mx_quantize(h["out"])
                assert torch.equal(q["sc"], ref.sc)
                assert torch.equal(q["out"].view(torch.uint8), ref.q.view(torch.uint8))


# ============================================================================ split-K reduce, exact
@pytest.mark.parametrize("splits,MN", go.REDUCE_SPECS)
def test_splitk_reduce_exact(gpu, splits, MN):
    """bf16 of the fp64 sum; the last case makes the grid-stride loop take a second trip."""
    parts, want = go.reduce_case(splits, MN)
    buf, out = go.guarded((1, MN), BF, gpu)
    ops.native().splitk_reduce(out, parts.to(gpu))
    torch.cuda.synchronize()
    assert go.guard_ok(buf, MN)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


# ==================================================================================== GEMVs, exact
def run_gemv(c: go.GemvCase, dev) -> dict:
    nat = ops.native()
    d = {k: v.to(dev) for k, v in c.dev.items()}
    cols = c.N // 2 if c.swiglu else c.N
    buf, out = go.guarded((c.M, cols), BF, dev)
    b = d.get("bias")
    if c.fmt == "bf16":
        nat.skinny_gemm(out, d["x"], d["w"], b, c.swiglu)
    elif c.fmt in ("fp8", "fp8x"):
        nat.skinny_gemm_fp8(out, d["x"], d.get("xs"), d["w"], d["ws"], b, c.swiglu)
    elif c.fmt == "int8":
        nat.skinny_gemm_int8(out, d["x"], d["w"], d["ws"], b, c.swiglu)
    else:
        nat.skinny_gemm_fp4(out, d["x"], d["w"], d["ws"], b, c.swiglu)
    torch.cuda.synchronize()
    return {"out": out.cpu(), "guard": go.guard_ok(buf, c.M * cols)}


@pytest.mark.parametrize("N", go.GEMV_NS)
@pytest.mark.parametrize("fmt", go.GEMV_FORMATS)
def test_gemv_exact(gpu, fmt, N):
    """Odd N (the clamped second row of the last wave), one workgroup's 8 rows and one past it;
    K at the format's minimum, one unrolled group, one vector past it (the k < K zero fill) and
    8192; every M, with and without an integer bias; int8 also with x >= 0."""
    for a in go.exact_gemv_specs(fmt):
        if a[2] != N or (len(a) > 5 and a[5]):
            continue
        c = go.gemv_case(*a)
        bad = go.check_gemv(c, run_gemv(c, gpu))
        assert not bad, (c.name, bad)


@pytest.mark.parametrize("fmt", go.GEMV_FORMATS)
def test_gemv_exact_swiglu(gpu, fmt):
    for a in go.exact_gemv_specs(fmt):
        if len(a) > 5 and a[5]:
            c = go.gemv_case(*a)
            bad = go.check_gemv(c, run_gemv(c, gpu))
            assert not bad, (c.name, bad)


# ================================================================================ real-valued cases
@pytest.mark.parametrize("fam", go.TILE_FAMILIES)
@pytest.mark.parametrize("prec", go.TILE_PRECS)
def test_gemm_tile_real_valued(gpu, prec, fam):
    """Every element within 2^-8 (1 + 2^-6) |o| + 2 K 2^-24 S of the fp64 product."""
    worst = 0.0
    for M in go.REAL_MS:
        for kt in go.REAL_KTS:
            c = go.real_tile_case(prec, fam, M, 256, kt)
            for sp in go.REAL_SPLITS:
                r = run_tile(c, gpu, sp, 0)
                bad = go.check_tile(c, r, sp, 0)
                print(f"RATIO gemm_tile-{prec} {fam} M{M} kt{kt} s{sp} {r.get('ratio', float('nan')):.3f}")
                assert not bad, (c.name, sp, bad)
                worst = max(worst, r["ratio"])
                if prec != "int8":
                    epi = 0 if sp == 1 else 4
                    r4 = run_tile(c, gpu, sp, epi, "gemm4")
                    bad = go.check_tile(c, r4, sp, epi)
                    assert not bad, (c.name, "gemm4", sp, bad)
                    worst = max(worst, r4["ratio"])
    print(f"RATIO gemm_tile/gemm4-{prec} {fam} worst {worst:.3f}")


@pytest.mark.parametrize("fmt", go.GEMV_FORMATS)
def test_gemv_real_valued(gpu, fmt):
    """Every element within 2^-8 (1 + 2^-6) |o| + c 2^-24 S, c the kernel's chain length; the
    int8 kernel under its |q| + 128 contract, family ``offset`` included."""
    worst = {}
    for a in go.real_gemv_specs(fmt):
        c = go.real_gemv_case(*a)
        r = run_gemv(c, gpu)
        bad = go.check_gemv(c, r)
        print(f"RATIO gemv-{fmt} {a[1]} M{c.M} K{c.K} {r.get('ratio', float('nan')):.3f}")
        assert not bad, (c.name, bad)
        worst[a[1]] = max(worst.get(a[1], 0.0), r["ratio"])
    for fam, w in worst.items():
        print(f"RATIO gemv-{fmt} {fam} worst {w:.3f}")
