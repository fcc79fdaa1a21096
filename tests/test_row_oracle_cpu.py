"""tests/row_oracle.py checked without a GPU: its Python copies of the launchers' thread / VPT
choice reach the arms the width lists claim, ops/reference.py and the CPU paths of ops meet every
bound and condition on every case the GPU tests run (which pins the bounds to something real),
and ten deliberately wrong implementations each fail at least one case."""
import pytest
import torch

import row_oracle as ro
from distributed_llm_inference import ops

BF = ro.BF
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------ the oracle
def test_launcher_arm_coverage():
    """The width lists reach exactly the (threads, VPT) instantiations they were chosen for; a
    launcher change that moves an arm makes the lists stale and fails here (the Python copies
    of norm_threads / row_threads must be changed with the launchers)."""
    norm = {(t, V) for t, _, V in map(ro.norm_arm, ro.NORM_WIDTHS)}
    quant = {(t, V) for t, _, V in map(ro.quant_arm, ro.QUANT_WIDTHS)}
    assert norm == ro.NORM_ARMS
    assert quant == ro.QUANT_ARMS
    # non-power-of-two vector counts round up: 3 -> 4, 6 -> 8 (norm), 3 -> 4, 5 -> 8, 9 -> 16
    assert ro.norm_arm(5120)[1:] == (3, 4) and ro.norm_arm(10248)[1:] == (6, 8)
    assert ro.quant_arm(4104)[1:] == (3, 4) and ro.quant_arm(32776)[1:] == (5, 8)
    assert ro.quant_arm(65544)[1:] == (9, 16)
    # one valid lane in the last slot
    assert 2056 // 8 - ro.norm_arm(2056)[0] == 1
    # the first widths past the launchers' limits
    assert ro.norm_arm(16384)[2] == 8 and ro.norm_arm(16392)[2] is None
    assert ro.quant_arm(131072)[2] == 16 and ro.quant_arm(131080)[2] is None
    for rows, W in (ro.EW_BIG,):
        assert rows * W // 8 > 2048 * 256


def test_spike_positions():
    t, vpt, _ = ro.norm_arm(10248)
    e = ro.spike_elems(10248, t, vpt)
    assert e[:5] == [0, 10247, 511, 512, 10240]
    assert e[5] // 8 >= (vpt - 1) * t and e[5] < 10248
    assert set(ro.spike_elems(8, 64, 1)) == {0, 7, 3}
    x = ro.family("spike", 2056, ro.norm_arm(2056)[:2], "t")
    assert (x.float().abs() == 300).sum(-1).tolist() == [1] * ro.ROWS


def test_interleaved_map_two_ways():
    """The column map read off activation.hip's comment equals the one ops._swiglu_src gives."""
    for I in ro.INTERLEAVED_I:
        gc, uc = ro.il_columns(I)
        gs, us = ro.il_columns_from_src(I)
        assert torch.equal(gc, gs) and torch.equal(uc, us)
        assert sorted(gc.tolist() + uc.tolist()) == list(range(2 * I))


def test_e4m3_rounding():
    b = torch.arange(256, dtype=torch.uint8)
    b = b[(b & 0x7F) != 0x7F]
    v = ro.f8_value(b)
    assert torch.equal(ro.e4m3_bytes(v), b)
    # ties go to the even code, anything past 448 saturates, tiny values underflow to 0
    pos = b[(b & 0x80) == 0]
    lo, hi = ro.f8_value(pos[:-1]), ro.f8_value(pos[1:])
    tie = ro.e4m3_bytes((lo + hi) / 2)
    assert bool(((tie & 1) == 0).all())
    assert bool(((tie == pos[:-1]) | (tie == pos[1:])).all())
    assert ro.e4m3_bytes(torch.tensor([1e9, -500.0, 2.0 ** -11, 464.0], dtype=torch.float64)
                         ).tolist() == [0x7E, 0xFE, 0x00, 0x7E]
    x = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * 100
    assert torch.equal(ro.e4m3_bytes(x.float().double()),
                       x.float().clamp(-448, 448).to(ro.F8).view(torch.uint8))


def test_sum_parts_is_sequential():
    p = torch.tensor([1.0, 2.0 ** -24, 2.0 ** -24, -1.0]).reshape(4, 1, 1)
    assert float(ro.sum_parts(p)) == 0.0          # ((1 + e) + e) - 1 in fp32, not 2e


# ------------------------------------------------------------------- the reference vs bounds
GROUPS = [("rms", ro.norm_cases("rms")), ("ln", ro.norm_cases("ln")),
          ("rms-parts", ro.parts_cases("rms")), ("quant-parts", ro.parts_cases("quant")),
          ("quant", ro.quant_cases()), ("silu_mul_quant", ro.silu_quant_cases()),
          ("int8", ro.int8_cases()), ("elementwise", ro.elementwise_cases())]


@pytest.mark.parametrize("name,cases", GROUPS, ids=[g[0] for g in GROUPS])
def test_reference_within_bounds(name, cases):
    worst, share, fails = {}, 0.0, []
    for c in cases:
        v = ro.evaluate(c, ro.run_ops(c, CPU))
        key = (c.kernel, c.family)
        worst[key] = max(worst.get(key, 0.0), v.ratio)
        share = max(share, v.share)
        fails += [f"{c.ident()}: {p}" for p in v.problems]
    for (k, fam), r in sorted(worst.items()):
        print(f"ROW-RATIO cpu {k} {fam} {r:.4f}")
    print(f"ROW-SHARE cpu {name} {share:.2e}")
    assert not fails, "\n".join(fails[:20])


def test_tiny_rows_survive_the_cpu_quantiser():
    """A row of 1e-20 g used to quantise to zeros (amax clamped at 1e-12)."""
    x = ro.family("tiny", 520, (128, 1), "x")
    q, s = ops.quant_rowwise(x)
    assert bool((q.float().abs().amax(-1) == 448).all())
    assert torch.allclose(s.reshape(-1), x.float().abs().amax(-1) / 448, rtol=1e-6, atol=0)


# ----------------------------------------------------------------------------------- mutations
def _truncate(y32):
    return (y32.view(torch.int32) & -65536).view(torch.float32).to(BF)


def _rms_mutant(c, kind):
    inp = ro.inputs(c)
    t, _, V = ro.norm_arm(c.H)
    w = inp["w"].float()
    v, r = inp["x"].float(), None
    if c.residual:
        s32 = v + inp["res"].float()
        r = s32.to(BF)
        v = s32 if kind == "unrounded_residual" else r.float()
    sq = v * v
    if kind == "drop_last_vector":
        sq = sq.clone()
        sq[:, -8:] = 0
    div = t * V * 8 if kind == "divisor" else c.H
    rstd = torch.rsqrt(sq.sum(-1, keepdim=True) / div + (0.0 if kind == "no_eps" else c.eps))
    if kind == "shift_w":
        w = torch.roll(w, 8)
    y32 = v * rstd * w
    return dict(y=_truncate(y32) if kind == "truncate" else y32.to(BF), r=r)


def _ln_mutant(c, kind):
    inp = ro.inputs(c)
    v, r = inp["x"].float(), None
    if c.residual:
        r = ro.bf16_add(inp["x"], inp["res"])
        v = r.float()
    mean = v.mean(-1, keepdim=True)
    d = v if kind == "var_about_0" else v - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + c.eps)
    return dict(y=((v - mean) * rstd * inp["w"].float() + inp["b"].float()).to(BF), r=r)


def _quant_mutant(c, kind):
    x = ro.inputs(c)["x"].float()
    t, vpt, _ = ro.quant_arm(c.H)
    a = x.abs()
    if kind == "amax_skips_last_slot":
        a = a.clone()
        a[:, (torch.arange(c.H) // 8) >= (vpt - 1) * t] = 0
    qmax = 240.0 if kind == "fp8_max_240" else 448.0
    amax = a.amax(-1)
    s = torch.where(amax > 0, (amax / qmax).clamp_min(ro.FLT_MIN), torch.ones_like(amax))
    q = (x / s[:, None]).clamp(-qmax, qmax).to(ro.F8).view(torch.uint8)
    return dict(q=q, s=s)


def _il_mutant(c, kind):
    inp = ro.inputs(c)
    g, u = (inp["up"], inp["gate"]) if kind == "swap_gate_up" else (inp["gate"], inp["up"])
    return dict(y=(torch.nn.functional.silu(g.float()) * u.float()).to(BF))


PLAIN_QUANT = [c for c in ro.quant_cases() if not (c.norm or c.residual)]
IL = [c for c in ro.elementwise_cases() if c.kernel == "silu_il"]
MUTANTS = [
    ("drop_last_vector", _rms_mutant, ro.norm_cases("rms")),
    ("divisor", _rms_mutant, ro.norm_cases("rms")),
    ("no_eps", _rms_mutant, ro.norm_cases("rms")),
    ("unrounded_residual", _rms_mutant, ro.norm_cases("rms")),
    ("truncate", _rms_mutant, ro.norm_cases("rms")),
    ("shift_w", _rms_mutant, ro.norm_cases("rms")),
    ("amax_skips_last_slot", _quant_mutant, PLAIN_QUANT),
    ("fp8_max_240", _quant_mutant, PLAIN_QUANT),
    ("swap_gate_up", _il_mutant, IL),
    ("var_about_0", _ln_mutant, ro.norm_cases("ln")),
]


@pytest.mark.parametrize("fn,cases", [(MUTANTS[i][1], MUTANTS[i][2]) for i in (0, 6, 8, 9)],
                         ids=["rms", "quant", "silu_il", "ln"])
def test_unmutated_torch_versions_pass(fn, cases):
    """The torch implementations the mutants are made from meet every bound themselves, so a
    mutant's failure is the mutation's."""
    for c in cases:
        v = ro.evaluate(c, fn(c, "none"))
        assert v.ok, f"{c.ident()}: {v.problems}"


@pytest.mark.parametrize("kind,fn,cases", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutation_is_detected(kind, fn, cases):
    caught = [c.ident() for c in cases if not ro.evaluate(c, fn(c, kind)).ok]
    print(f"ROW-MUTANT {kind}: fails {len(caught)} of {len(cases)} cases")
    assert caught, f"mutation {kind} passes every case"
