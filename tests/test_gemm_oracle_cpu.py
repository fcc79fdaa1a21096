"""gemm_oracle.py on the CPU: every case meets its own conditions, the CPU branches of the GEMM
entry points in ops pass the same checks the HIP kernels are held to in test_gemm_exact_gpu.py,
and the checker rejects every fault of the tile / GEMV emulator on a named case -- the evidence
that the GPU tests would fail on a subtly wrong kernel.

Mutation -> case on which it is rejected (gemm_oracle.TILE_FAULTS / GEMV_FAULTS; printed by
test_*_fault_is_rejected with ``-s``):

  drop_last_ktile                    bf16 M65 N256 5 k-tiles, 2 splits, reduced bf16
  start_one_ktile_early              fp8 M65 N256 7 k-tiles, 3 splits, fp32 partials
  swap_chunks_in_a                   bf16 M65 N256 2 k-tiles
  ktile_offset_a_only                int8 M65 N256 5 k-tiles, 2 splits, bf16 partials
  a_scale_row_xor_1                  fp8 M300 N256
  b_scale_chan_xor_1                 fp8 M65 N256
  b_scale_chan_plus_16               int8 M65 N256
  mx_scale_next_kblock               mx M65 N256 2 k-tiles
  mx_scale_row_xor_1                 mx M257 N256
  mx_pad_row_scale                   fp8 M65 N256, SwiGLU -> MX epilogue
  ragged_group_tm_tn                 bf16 M2309 N512 (tiles_m = 10)
  remap_remainder_off_by_one         bf16 M300 N256 5 splits (grid 10)
  outlier_in_every_split             int8 M65 N256 3 splits, J 32, 3 live columns
  dead_outlier_chunk                 int8 M65 N256, J 64, dynamic cnt 3
  swap_gate_up_one_pair              bf16 M65 N256, SwiGLU epilogue
  store_row_m                        bf16 M65 N256 (guard)
  drop_last_partial_kstep            GEMV bf16 M1 N7 K2056
  store_row_1_of_last_wave_at_odd_n  GEMV fp8 M2 N7 K16 (guard)
  sum_x_of_row_0_for_row_1           GEMV int8 M2 N8 K4112, x >= 0
  bias_from_n_minus_1                GEMV fp4 M1 N9 K32
"""
import pytest
import torch

from distributed_llm_inference import ops

import gemm_oracle as go

BF = go.BF


# ------------------------------------------------------------------- 1. the cases' own conditions
@pytest.mark.parametrize("prec", go.TILE_PRECS)
def test_exact_tile_cases_meet_their_conditions(prec):
    """tile_case asserts exactness in fp32, bf16 outputs and partials, asymmetry and k coverage
    while it builds; here also: the tile counts the split cases were chosen for, +-127 among the
    int8 codes, and the CPU emulator (no fault) reproduces every case bit for bit."""
    specs = go.exact_tile_specs(prec)
    grids = set()
    for a in specs:
        c = go.tile_case(*a)
        go.assert_exact(c, a[4] if len(a) > 4 else (1,), len(a) > 8 and a[8])
        if c.prec == "mx":
            assert c.kt // (a[4][0] if len(a) > 4 else 1) <= 64
        for sp in (a[4] if len(a) > 4 else (1,)):
            grids.add((c.M + 255) // 256 * (c.N // 256) * sp)
    assert {3, 10, 21} <= grids
    if prec == "int8":
        for a in specs:
            if len(a) == 4:   # the plain cases carry +-127 in both operands
                c = go.tile_case(*a)
                assert 127 in c.braw and -127 in c.braw
                assert c.M == 1 or (127 in c.araw and -127 in c.araw)
        lives = {(c.xo.shape[1], c.live, c.dynamic) for c in map(lambda a: go.tile_case(*a), specs)
                 if c.xo is not None}
        assert lives == set(go.OUTLIER_COMBOS)


@pytest.mark.parametrize("prec", go.TILE_PRECS)
def test_tile_emulator_without_fault_is_exact(prec):
    for a in go.exact_tile_specs(prec)[::5]:
        c = go.tile_case(*a)
        sp = a[4][0] if len(a) > 4 else 1
        for epi in ((0, 1, 4) if sp > 1 else (0,)):
            assert not go.check_tile(c, go.emulate_tile(c, sp, epi), sp, epi), (c.name, epi)


@pytest.mark.parametrize("fmt", go.GEMV_FORMATS)
def test_exact_gemv_cases_meet_their_conditions(fmt):
    """Every e4m3 / e2m1 magnitude code occurs among the weights of the format's cases."""
    cases = [go.gemv_case(*a) for a in go.exact_gemv_specs(fmt)]
    assert {c.K for c in cases} == set(go.gemv_ks(fmt))
    if fmt in ("fp8", "fp8x"):
        codes = torch.cat([(c.dev["w"].view(torch.uint8) & 0x7F).flatten() for c in cases]).unique()
        assert codes.tolist() == list(range(0x7F))
    if fmt == "fp4":
        codes = torch.cat([torch.cat([c.dev["w"] & 0xF, c.dev["w"] >> 4]).flatten() for c in cases])
        assert codes.unique().numel() == 16
    if fmt == "int8":
        assert any(bool((c.xraw >= 0).all()) and c.K == 8192 for c in cases)
        assert any(127 in c.wraw and -127 in c.wraw for c in cases)


def test_real_valued_families_are_what_they_claim():
    c = go.real_tile_case("fp8", "positive", 65, 256, 5)
    assert bool((c.araw >= 0).all() and (c.braw >= 0).all())
    # S = |o|: the bound is within 1.3x of one bf16 rounding at K = 8192
    c = go.real_tile_case("bf16", "positive", 65, 256, 128)
    assert float((go.tile_bound(c) / (2.0 ** -8 * go.oracle(c).abs())).max()) < 1.3
    c = go.real_tile_case("bf16", "spike", 65, 256, 5)
    k = (c.araw.abs() >= 300).nonzero()[:, 1]
    assert set((k // 64).tolist()) == set(range(5)) and set((k % 64 // 8).tolist()) == set(range(8))
    c = go.real_tile_case("int8", "scale_spread", 300, 256, 5)
    assert float(c.sa.max() / c.sa.min()) >= 2 ** 10 and float(c.sb.max() / c.sb.min()) >= 2 ** 10
    c = go.real_gemv_case("int8", "offset", 2, 33, 8192)
    assert bool((c.wraw[16] == 0).all()) and float((c.wraw.abs() <= 2).double().mean()) > 0.85
    assert float(c.xraw.mean()) > 2.9


# ---------------------------------------------------------------------- 2. the CPU branches of ops
def _ops_tile(c: go.TileCase, swiglu: bool = False):
    d = go.tile_operands(c, "cpu")
    if c.prec == "bf16":
        return ops.gemm_tile(d["a"], d["b"], swiglu=swiglu)
    if c.prec == "fp8":
        return ops.gemm_tile_fp8(d["a"], d["sa"], d["b"], d["sb"], swiglu=swiglu)
    if c.prec == "mx":
        return ops.gemm_tile_fp8_mx(ops.MxFp8(d["a"], d["a_mx"]), d["b"], d["sb"])
    raise AssertionError(c.prec)


@pytest.mark.parametrize("prec", ["bf16", "fp8", "mx"])
def test_cpu_tile_branches_are_exact(prec):
    for a in go.exact_tile_specs(prec)[::3]:
        if len(a) > 5:
            continue
        c = go.tile_case(*a)
        assert not go.check_tile(c, {"out": _ops_tile(c)}), c.name


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_cpu_tile_swiglu_and_mx_producer(prec):
    for M, N, kt in go.SWIGLU_SPECS:
        c = go.tile_case(prec, M, N, kt, (1,), 0, 0, False, True)
        h = _ops_tile(c, swiglu=True)
        assert not go.check_tile(c, {"out": h}, 1, 2), c.name
        assert torch.equal(h, ops.swiglu_interleaved(_ops_tile(c)))     # fused == unfused, bitwise
        if prec == "fp8":
            d = go.tile_operands(c, "cpu")
            a = ops.gemm_tile_fp8(d["a"], d["sa"], d["b"], d["sb"], swiglu=True, mx_out=True)
            assert not go.check_tile(c, {"out": a.q.view(torch.uint8), "sc": a.sc}, 1, 3), c.name


@pytest.mark.parametrize("prec,fam", [(p, f) for p in ("bf16", "fp8", "mx") for f in go.TILE_FAMILIES])
def test_cpu_tile_branches_meet_the_real_valued_bound(prec, fam):
    c = go.real_tile_case(prec, fam, 65, 256, 5)
    res = {"out": _ops_tile(c)}
    assert not go.check_tile(c, res), (c.name, res.get("ratio"))


def test_cpu_llm_int8_linear_is_exact_when_rows_quantise_exactly():
    """Every row carries a +-127, so quant_rowwise_int8's scale is exactly 1 and the int8 codes
    are the row itself; threshold 0 switches the outlier decomposition off."""
    c = go.tile_case("int8", 65, 256, 2)
    x = c.araw.clone()
    x[:, 7] = torch.where(torch.arange(c.M) % 2 == 0, 127.0, -127.0).double()
    y = ops.llm_int8_linear(x.to(BF), c.braw.to(torch.int8), c.sb.float(), threshold=0.0)
    want = x @ c.b_deq().t()
    assert float((x.abs() @ c.b_deq().abs().t()).max()) * 4 < 2 ** 24
    assert torch.equal(y, want.to(BF))


def test_cpu_split_k_partials_materialize_exactly():
    c = go.tile_case("fp8", 65, 256, 7, (3,))
    parts = go.emulate_tile(c, 3, 4)["out"]
    assert not go.check_tile(c, {"out": ops.SplitKPartials(parts).materialize()})


@pytest.mark.parametrize("fmt", go.GEMV_FORMATS)
def test_cpu_gemv_branches(fmt):
    for a in go.exact_gemv_specs(fmt)[::3]:
        c = go.gemv_case(*a)
        assert not go.check_gemv(c, {"out": go.run_gemv_ops(c)}), c.name
    for a in go.real_gemv_specs(fmt):
        c = go.real_gemv_case(*a)
        res = {"out": go.run_gemv_ops(c)}
        assert not go.check_gemv(c, res), (c.name, res.get("ratio"))


def test_cpu_swiglu_interleaved_takes_gemv_widths():
    """32-column groups (16 gate, 16 up): any N % 32 == 0, the GEMV epilogues' widths included."""
    g = torch.Generator().manual_seed(3)
    y = torch.randn(2, 96, generator=g).to(BF)
    gr, ur = go.gemv_swiglu_rows(96)
    want = (torch.nn.functional.silu(y[:, gr].float()) * y[:, ur].float()).to(BF)
    assert torch.equal(ops.swiglu_interleaved(y), want)


def test_reduce_cases():
    for sp, mn in go.REDUCE_SPECS[:-1]:
        parts, want = go.reduce_case(sp, mn)
        assert torch.equal(parts.double().sum(0).to(BF), want)


# ------------------------------------------------------------------------------------ 3. mutations
@pytest.mark.parametrize("fault", sorted(go.TILE_FAULTS))
def test_tile_fault_is_rejected(fault):
    args, sp, epi = go.TILE_FAULTS[fault]
    c = go.tile_case(*args)
    assert not go.check_tile(c, go.emulate_tile(c, sp, epi), sp, epi), "the clean emulator must pass"
    bad = go.check_tile(c, go.emulate_tile(c, sp, epi, fault), sp, epi)
    print(f"{fault:34s} rejected on {c.name} splits {sp} epilogue {epi}: {bad}")
    assert bad, f"{fault} goes unnoticed on {c.name}"


@pytest.mark.parametrize("fault", sorted(go.GEMV_FAULTS))
def test_gemv_fault_is_rejected(fault):
    c = go.gemv_case(*go.GEMV_FAULTS[fault])
    assert not go.check_gemv(c, go.emulate_gemv(c)), "the clean emulator must pass"
    bad = go.check_gemv(c, go.emulate_gemv(c, fault))
    print(f"{fault:34s} rejected on {c.name}: {bad}")
    assert bad, f"{fault} goes unnoticed on {c.name}"


def test_a_fault_without_effect_is_not_counted():
    """The XCD remap is bijective for every grid size, and `x <= r` in place of `x < r` is the
    same map: the checker rejects only what changes the result."""
    for n in (1, 3, 8, 10, 21, 33):
        assert sorted(go.remap(b, n) for b in range(n)) == list(range(n))
    for tiles_m, tiles_n in ((10, 2), (9, 2), (3, 5), (17, 3)):
        seen = {go.grouped_tile(t, tiles_m, tiles_n) for t in range(tiles_m * tiles_n)}
        assert seen == {(m, n) for m in range(tiles_m) for n in range(tiles_n)}
