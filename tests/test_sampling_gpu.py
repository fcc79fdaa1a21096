"""The HIP sampler (csrc/kernels/sampling.hip) against its bit-exact CPU oracle
(tests/sampling_oracle.py): which token a seeded row must produce, on the register path (bf16
logits, V % 8 == 0, V <= 131072) and on the radix path (the same values as fp32 logits).

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import math

import numpy as np
import pytest
import torch

import sampling_oracle as so
from distributed_llm_inference import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DTYPES = [BF, torch.float32]
_IDS = ["bf16", "f32"]


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol)
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


def _sample(gpu, case, dtype, step=None, counters=True):
    """(tokens, log-probabilities) of one ops.sample call over a Case, on the CPU."""
    B = case.logits.shape[0]
    lp = torch.empty(B, device=gpu)
    tok = ops.sample(case.logits.to(gpu).to(dtype), temperature=case.temperature.to(gpu),
                     top_k=case.top_k.to(gpu), top_p=case.top_p.to(gpu),
                     seeds=case.seeds.to(gpu),
                     step=None if step is None else torch.tensor([step], device=gpu),
                     counters=case.counters.to(gpu) if counters else None, logprobs=lp)
    return tok.cpu().long().numpy(), lp.cpu()


_RESULTS = {}


def _matrix_result(gpu, V, dtype):
    if (V, dtype) not in _RESULTS:
        _RESULTS[(V, dtype)] = _sample(gpu, so.matrix_case(V), dtype)
    return _RESULTS[(V, dtype)]


def _check_tokens(tok, oracle, what):
    V = oracle[0].may_keep.shape[0]
    assert ((tok >= 0) & (tok < V)).all(), (what, tok)
    outside = [b for b, (t, o) in enumerate(zip(tok, oracle)) if not o.may_keep[t]]
    assert not outside, f"{what}: tokens outside may_keep in rows {outside}: {tok[outside]}"
    wrong = [(b, int(t), o.token, round(o.margin, 4))
             for b, (t, o) in enumerate(zip(tok, oracle)) if o.decisive and t != o.token]
    assert not wrong, f"{what}: (row, kernel, oracle, margin) {wrong}"


def _check_logprobs(tok, lp, oracle, what):
    want = torch.tensor([o.logprobs[t] for t, o in zip(tok, oracle)], dtype=torch.float64)
    assert torch.isfinite(lp).all(), (what, lp)
    _close(lp, want, 1e-3, 1e-3, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("V", so.VOCABS)
def test_tokens_equal_the_oracle(gpu, V, dtype):
    """Every token lies in may_keep and every decisive row is the oracle's token exactly, over
    temperatures, top-k x top-p pairs (and top_p = 0) with per-row seeds and counters."""
    tok, _ = _matrix_result(gpu, V, dtype)
    _check_tokens(tok, so.matrix_oracle(V), f"V={V} {dtype}")


def test_matrix_is_mostly_decisive():
    """The equality above is not vacuous: at most 5 % of the rows of the whole matrix are left
    undecided by the oracle (checked for the same inputs in test_sampling_oracle_cpu.py)."""
    rows = [r for V in so.VOCABS for r in so.matrix_oracle(V)]
    assert sum(not r.decisive for r in rows) <= so.MAX_NON_DECISIVE * len(rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("V", so.VOCABS)
def test_sampled_logprob(gpu, V, dtype):
    """Log-probability of the sampled token against the float64 log_softmax(x) of the whole
    row, within the bound of the greedy log-probability test."""
    tok, lp = _matrix_result(gpu, V, dtype)
    _check_logprobs(tok, lp, so.matrix_oracle(V), f"logprob V={V} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_step_and_row_keying(gpu, dtype):
    """Without counters the draw is keyed by (seed, step, row, i)."""
    oracle = so.step_oracle()
    assert sum(not r.decisive for r in oracle) <= so.MAX_NON_DECISIVE * len(oracle)
    tok, lp = _sample(gpu, so.matrix_case(so.STEP_V), dtype, step=so.STEP, counters=False)
    _check_tokens(tok, oracle, f"step keying {dtype}")
    _check_logprobs(tok, lp, oracle, f"step keying logprob {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_mixed_greedy_and_sampled_rows(gpu, dtype):
    """A batch with greedy (T = 0) and sampled rows: each row follows its own temperature."""
    case, oracle = so.mixed_case(), so.mixed_oracle()
    assert sum(not r.decisive for r in oracle) <= so.MAX_NON_DECISIVE * len(oracle)
    tok, lp = _sample(gpu, case, dtype)
    _check_tokens(tok, oracle, f"mixed {dtype}")
    _check_logprobs(tok, lp, oracle, f"mixed logprob {dtype}")
    greedy = (case.temperature == 0).numpy()
    assert greedy.any() and not greedy.all()
    assert np.array_equal(tok[greedy], case.logits.float().argmax(-1).numpy()[greedy])


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_largest_uniform_is_a_finite_draw(gpu, dtype):
    """(seed 3, counter 228, index 128165) hashes to all ones, the largest uniform.  Every logit
    is -30 but index 7 (0): the draw is 7, whatever the Gumbel term of index 128165 - as long as
    it is finite.  (A uniform of exactly 1.0 makes it +inf and returns 128165.)"""
    seed, ctr, idx = so.ALL_ONES_TRIPLE
    logits = so.all_ones_logits()
    o = so.sample_row(logits[0].numpy(), 1.0, seed=seed, counter=ctr)
    assert o.token == 7 and o.decisive
    lp = torch.empty(1, device=gpu)
    tok = ops.sample(logits.to(gpu).to(dtype), temperature=torch.ones(1, device=gpu),
                     seeds=torch.tensor([seed], device=gpu),
                     counters=torch.tensor([ctr], device=gpu), logprobs=lp)
    assert int(tok) == 7, (int(tok), idx)
    assert math.isfinite(float(lp)), float(lp)
    _close(lp, torch.tensor([o.logprobs[7]]), 1e-3, 1e-3, "logprob")


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("name,logits,k,p", so.support_rows(),
                         ids=[r[0] for r in so.support_rows()])
def test_support_equals_the_kept_set(gpu, dtype, name, logits, k, p):
    """2048 seeds on one constructed row (ties straddling the top-k and the top-p cut, -inf
    logits): the set of sampled tokens is exactly must_keep (== may_keep; every kept token has
    probability >= 0.02, so it misses 2048 draws with probability < 1e-17)."""
    B = 2048
    o = so.sample_row(logits.numpy(), 1.0, k, p, seed=0, counter=0)
    assert np.array_equal(o.must_keep, o.may_keep)
    tok = ops.sample(logits.to(gpu).to(dtype).repeat(B, 1).contiguous(),
                     temperature=torch.ones(B, device=gpu),
                     top_k=torch.full((B,), k, dtype=torch.int32, device=gpu),
                     top_p=torch.full((B,), p, device=gpu),
                     seeds=torch.arange(B, device=gpu) * 7919 + 11,
                     counters=torch.arange(B, device=gpu) % 5)
    seen = np.zeros(logits.shape[0], dtype=bool)
    seen[tok.cpu().long().numpy()] = True
    assert np.array_equal(seen, o.must_keep), (name, np.nonzero(seen)[0], np.nonzero(o.must_keep)[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("pad,offset", [(24, 0), (13, 0), (8, 4)],
                         ids=["stride%8==0", "stride%8!=0", "offset4"])
def test_strided_and_offset_views(gpu, dtype, pad, offset):
    """A [B, V] view of a wider buffer (padding columns hold +3e38), also one that starts 4
    elements into each row (a bf16 base pointer that is only 8-byte aligned, which must not take
    the 16-byte loads): greedy and sampled tokens equal those of the contiguous copy."""
    V = 1000
    case = so.matrix_case(V)
    B = case.logits.shape[0]
    big = torch.full((B, V + pad), 3e38, device=gpu, dtype=dtype)
    view = big[:, offset:offset + V]
    view.copy_(case.logits.to(gpu))
    assert view.stride(1) == 1 and view.stride(0) == V + pad and not view.is_contiguous()
    if offset:
        assert view.data_ptr() % 16 == (8 if dtype == BF else 0)
    flat = view.contiguous()
    assert torch.equal(ops.sample(view).cpu(), ops.sample(flat).cpu())
    assert torch.equal(ops.sample(view).cpu().long(), case.logits.float().argmax(-1))
    kw = dict(temperature=case.temperature.to(gpu), top_k=case.top_k.to(gpu),
              top_p=case.top_p.to(gpu), seeds=case.seeds.to(gpu), counters=case.counters.to(gpu))
    tok = ops.sample(view, **kw).cpu()
    assert int(tok.max()) < V and int(tok.min()) >= 0
    assert torch.equal(tok, ops.sample(flat, **kw).cpu())
    _check_tokens(tok.long().numpy(), so.matrix_oracle(V), f"view pad={pad} off={offset} {dtype}")
