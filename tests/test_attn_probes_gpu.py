"""The paged attention kernels (attention.hip, attn_core.h, attn_prefill32.hip) against the
token-space fp64 oracle of tests/attn_oracle.py, on inputs where every key counts:

  * positional probes: sign-code keys, q = beta * code of one chosen token, so the expected
    output is that token's V row and any wrong key, mask bit, slot or split is an O(1) error;
    invisible targets (the stale slot past the end, key p + 1, the token that just left the
    window, a sink's code in q) must NOT come back;
  * peaked dense softmax (logit std 5), keys sorted ascending / descending by score, so the
    running max and the split merges see far-apart maxima;
  * every case twice, stale cache slots holding 0 and +-240: the outputs must be bit-identical.

Accepted error: |out - o| <= 2^-8 * (A + |o|) + 1e-6 (attn_oracle.bound: twice the derived
worst case of the bf16 roundings of P and of the output).  Each test prints the largest
err / bound it saw as ``ATTN-RATIO <family> <case> <ratio>`` (run with -s to see them).

Run on an MI355X: ``python -m pytest tests/test_attn_probes_gpu.py -m gpu``.
"""
import functools

import numpy as np
import pytest
import torch

import attn_oracle as ao
from distributed_llm_inference import ops

pytestmark = pytest.mark.gpu

ONE_STEP_SAMPLE = tuple(range(0, 512, 37)) + tuple(range(3, 21))   # 32 rows, all seven lengths


def _ids(specs):
    return [s.ident() for s in specs]


@functools.lru_cache(maxsize=2)
def _device_inputs(spec, poison):
    """The case's tensors on the GPU, stale slots zero or poisoned."""
    c = ao.make_case(spec)
    dev = torch.device("cuda:0")
    kc, vc, bt = c.caches(poison)
    qs = c.q_sink.to(dev) if c.q_sink is not None else None
    return (c.q.to(dev), qs, kc.to(dev), vc.to(dev), bt.to(dev),
            torch.tensor(c.seq_lens, dtype=torch.int32, device=dev), c.q_start().to(dev))


def _decode(spec, poison, splits):
    g = spec.geo
    q, qs, kc, vc, bt, lens, _ = _device_inputs(spec, poison)
    return ops.attn_decode(q, qs, kc, vc, bt, lens, g.scale, *g.window_args(), num_splits=splits,
                           k_scale=g.k_scale, v_scale=g.v_scale)


def _prefill(spec, poison, qb, tiles):
    g = spec.geo
    q, qs, kc, vc, bt, lens, q_start = _device_inputs(spec, poison)
    tm = ops.prefill_tiles(list(spec.q_lens), g.nh, g.nkv, qb=qb).to(q.device) if tiles else None
    return ops.attn_prefill(q, qs, kc, vc, bt, lens, q_start, max(spec.q_lens), g.scale,
                            *g.window_args(), k_scale=g.k_scale, v_scale=g.v_scale, tile_map=tm,
                            qb=qb)


def _check(spec, family, label, run, sample=None):
    """Run twice (stale slots 0 / +-240): bit-identical, and within the bound of the oracle."""
    c = ao.make_case(spec)
    out = run(False).cpu()
    out_p = run(True).cpu()
    o, A, _ = ao.oracle(spec, sample)
    done = ~torch.isnan(o)
    err = torch.where(done, (out.double() - o).abs(), torch.zeros_like(o))
    tol = torch.where(done, ao.bound(o, A), torch.ones_like(o))
    ratio = (err / tol).max().item()
    print(f"ATTN-RATIO {family} {spec.ident()}/{label} {ratio:.4f}")
    if ratio > 1.0:
        row, head, d = [int(x) for x in np.unravel_index(int((err / tol).argmax()), err.shape)]
        b = int(c.seq_of[row])
        msg = (f"{spec.ident()}/{label}: err {err[row, head, d].item():.4g} > bound "
               f"{tol[row, head, d].item():.4g} ({ratio:.3g}x) at row {row} head {head} d {d}: "
               f"sequence {b} (len {c.seq_lens[b]}) position {int(c.qpos[row])}, got "
               f"{out[row, head, d].item():.5g} want {o[row, head, d].item():.5g}")
        if spec.data == "probe":
            msg += (f"; probe q -> token {int(c.tq[row, head])}, q_sink -> token "
                    f"{int(c.ts[row, head])}, target {int(c.target[row, head])}, found V row of "
                    f"token {ao.nearest_v_row(c, row, head, out[row, head])}")
        pytest.fail(msg)
    if not torch.equal(out, out_p):
        diff = (out.float() != out_p.float()).nonzero()
        row, head, d = diff[0].tolist()
        b = int(c.seq_of[row])
        pytest.fail(f"{spec.ident()}/{label}: stale slots leak: {diff.shape[0]} elements differ "
                    f"between 0 and +-240 fill, first at row {row} head {head} d {d} (sequence "
                    f"{b}, len {c.seq_lens[b]}, position {int(c.qpos[row])}): "
                    f"{out[row, head, d].item():.5g} vs {out_p[row, head, d].item():.5g}")


def _fam_decode(spec):
    if spec.geo.win:
        return "decode-window"
    return "decode-fp8" if spec.geo.fp8 else "decode-bf16"


# ------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("spec", ao.decode_full_specs(), ids=_ids(ao.decode_full_specs()))
def test_decode_probes(gpu, spec):
    """Full cache, every length around the 32-key steps and the page edge in one batch, through
    the ungrouped (1, 3), pair-merged (2, 6) and 4-merged (4, 12) split paths; with 9 steps at
    most, the larger split counts leave trailing splits empty."""
    for splits in ao.DECODE_SPLITS:
        _check(spec, _fam_decode(spec), f"s{splits}", lambda p: _decode(spec, p, splits))


@pytest.mark.parametrize("spec", ao.decode_head_specs(), ids=_ids(ao.decode_head_specs()))
def test_decode_head_shapes(gpu, spec):
    """GQA groups of 1, 7, 16, 20 (two 16-head groups, the second with 4 live columns) and 32."""
    for splits in (1, 4):
        _check(spec, _fam_decode(spec), f"s{splits}", lambda p: _decode(spec, p, splits))


@pytest.mark.parametrize("spec", ao.decode_one_step_specs(),
                         ids=_ids(ao.decode_one_step_specs()))
def test_decode_one_step_loop(gpu, spec):
    """4096 work items: the one-step loop on a 256-CU device.  The oracle runs for a sample of
    32 rows with all seven lengths; the poison comparison covers every row."""
    _check(spec, _fam_decode(spec), "s1", lambda p: _decode(spec, p, 1), sample=ONE_STEP_SAMPLE)


@pytest.mark.parametrize("spec", ao.decode_window_specs(), ids=_ids(ao.decode_window_specs()))
def test_decode_window_probes(gpu, spec):
    """Sink + ring caches from before the sinks fill to several wraps of the ring."""
    for splits in ao.WINDOW_SPLITS:
        _check(spec, _fam_decode(spec), f"s{splits}", lambda p: _decode(spec, p, splits))


# ----------------------------------------------------------------------------------- prefill
_LEGACY = ao.prefill_legacy_specs()
_M32 = ao.prefill_m32_specs()


def _fam_prefill(spec, m32):
    return ("prefill-m32" if m32 else "prefill-legacy") + ("-window" if spec.geo.win else "")


@pytest.mark.parametrize("spec,variants", _LEGACY, ids=_ids([s for s, _ in _LEGACY]))
def test_prefill_legacy_probes(gpu, spec, variants):
    """attention.hip's prefill kernel (head dim 128 through the prefill_m32=False policy):
    1 and 2 query blocks per wave, dense grid and tile map, 4 / 2 / 1 heads per K/V tile."""
    with ops.kernel_policy(prefill_m32=False):
        for qb, tiles in variants:
            _check(spec, _fam_prefill(spec, False), f"qb{qb}-{'tiles' if tiles else 'dense'}",
                   lambda p: _prefill(spec, p, qb, tiles))


@pytest.mark.parametrize("spec,qbs", _M32, ids=_ids([s for s, _ in _M32]))
def test_prefill_m32_probes(gpu, spec, qbs):
    """attn_prefill32.hip (workgroups of 8, 4, 2 and 1 heads; full and windowed caches), and
    attention.hip's kernel on the same inputs against the same oracle."""
    for qb in qbs:
        for tiles in (True, False):
            _check(spec, _fam_prefill(spec, True), f"qb{qb}-{'tiles' if tiles else 'dense'}",
                   lambda p: _prefill(spec, p, qb, tiles))
        with ops.kernel_policy(prefill_m32=False):
            _check(spec, _fam_prefill(spec, False), f"qb{qb}-tiles-legacy",
                   lambda p: _prefill(spec, p, qb, True))


# ----------------------------------------------------------------------- peaked dense softmax
_DENSE = ao.dense_specs()


@pytest.mark.parametrize("family,spec", _DENSE,
                         ids=[f"{f}-{s.ident()}" for f, s in _DENSE])
def test_peaked_dense_softmax(gpu, family, spec):
    """Logits of std 5 with the keys sorted by head 0's score: ascending, every step raises the
    running max and later splits dominate earlier ones; descending, the reverse."""
    if spec.kind == "decode":
        for splits in (1, 2, 3, 4, 12):
            _check(spec, family, f"s{splits}", lambda p: _decode(spec, p, splits))
        return
    m32 = family.startswith("prefill-m32")
    with ops.kernel_policy(prefill_m32=m32):
        for qb in (1, 2):
            _check(spec, family, f"qb{qb}-tiles", lambda p: _prefill(spec, p, qb, True))
