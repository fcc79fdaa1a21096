"""The sampler's CPU oracle (tests/sampling_oracle.py) checked on its own: hash, uniform
conversion, kept sets against ops.reference.sample, goodness of fit of its draw, and that the
inputs of tests/test_sampling_gpu.py leave few rows undecided."""
import math
import statistics

import numpy as np
import pytest
import torch

import sampling_oracle as so
from distributed_llm_inference.ops import reference as ref


def test_splitmix64_first_output():
    assert int(so.splitmix64(0)) == 0xE220A8397B1DCDAF
    # array form, and wraparound of the state increment
    a = so.splitmix64(np.array([0, so.M64], dtype=np.uint64))
    assert int(a[0]) == 0xE220A8397B1DCDAF
    assert int(a[1]) == int(so.splitmix64(so.M64))


@pytest.mark.parametrize("top24", [0, 0xFFFFFF, 1 << 23, (1 << 23) + 1])
def test_uniform_is_strictly_inside_the_unit_interval(top24):
    """Smallest / largest raw draw and the first integers whose ``n + 0.5`` a 24-bit formula
    cannot represent: the formula in use maps them strictly inside (0, 1), exactly."""
    for low in (0, (1 << 40) - 1):
        r = (top24 << 40) | low
        u = so.uniform_from_raw(r)
        assert u.dtype == np.float32
        assert 0.0 < float(u) < 1.0, (hex(r), float(u))
        n = r >> (64 - so.UNIFORM_BITS)
        assert float(u) == (n + 0.5) / (1 << so.UNIFORM_BITS)   # no rounding anywhere
        g = -math.log(-math.log(float(u)))
        assert math.isfinite(g)


def test_24_bit_formula_reaches_one():
    """Why UNIFORM_BITS is 23: with 24 bits n + 0.5 rounds to even in fp32 and the largest n
    gives exactly 1.0 (an infinite Gumbel term)."""
    n = np.float32(0xFFFFFF)
    assert float((n + np.float32(0.5)) * np.float32(1.0 / 16777216.0)) == 1.0


def test_recorded_all_ones_triple():
    seed, ctr, idx = so.ALL_ONES_TRIPLE
    raw = so.raw_draws(seed, so.counter_base(0, ctr), so.ALL_ONES_V)
    ones = np.nonzero((raw >> np.uint64(40)) == np.uint64(0xFFFFFF))[0]
    assert ones.tolist() == [idx]
    assert int(raw[idx]) == int(so.raw_draws(seed, so.counter_base(0, ctr), 1, start=idx)[0])
    u = so.uniform_from_raw(raw)
    assert u.max() == u[idx] and 0.0 < float(u[idx]) < 1.0
    # the row of the GPU test: the oracle picks the only likely token, by a wide margin
    o = so.sample_row(so.all_ones_logits()[0].numpy(), 1.0, seed=seed, counter=ctr)
    assert o.token == 7 and o.decisive and o.margin > 5.0


def test_counter_base_keying():
    assert so.counter_base(5, counter=3) == 3 * 0x100000001B3
    assert so.counter_base(5, None, step=2) == (2 * 0x100000001B3) ^ (5 << 40)
    assert so.counter_base(0, counter=-1) == (-0x100000001B3) & so.M64


def _ref_mask(x, t, k, p, monkeypatch):
    """The kept set ops.reference.sample builds: the support of what it hands to multinomial."""
    seen = {}

    def fake(probs, n, generator=None):
        seen["mask"] = (probs > 0).numpy().copy()
        return torch.argmax(probs).reshape(1)

    monkeypatch.setattr(torch, "multinomial", fake)
    ref.sample(x[None], torch.tensor([t]), torch.tensor([k], dtype=torch.int32),
               torch.tensor([p]))
    monkeypatch.undo()
    return seen["mask"]


@pytest.mark.parametrize("k,p", [(0, 1.0), (5, 1.0), (0, 0.9), (20, 0.9), (40, 0.5), (3, 0.1),
                                 (63, 0.99), (64, 0.7), (1, 0.3), (0, 0.0), (5, 0.0)])
def test_kept_set_matches_reference(k, p, monkeypatch):
    g = torch.Generator().manual_seed(100 * k + int(100 * p))
    exact = 0
    for i in range(12):
        x = (torch.randn(64, generator=g) * (0.5 + i % 6)).to(torch.bfloat16).float()
        t = 0.5 + 0.25 * (i % 6)
        must, may = so.kept_sets(so.scaled(x.numpy(), t), k, p)
        mask = _ref_mask(x, t, k, p, monkeypatch)
        # always must <= reference <= may; a random row whose top-p cut falls inside the band
        # (must != may) decides nothing more, every other row pins the set exactly
        assert not (must & ~mask).any() and not (mask & ~may).any(), (k, p, i)
        if np.array_equal(must, may):
            assert np.array_equal(must, mask), (k, p, i)
            exact += 1
    # the comparison is not vacuous: at least half the rows are pinned.  (Not at p = 0.99, where
    # the elements at the cut of a 64-value row weigh less than the band of 2e-3 * Z itself.)
    if p <= 0.9:
        assert exact >= 6, exact


def test_kept_set_ties_and_edges():
    x = np.array([3.0, 1.0, 2.0, 2.0, 2.0, 0.0, -np.inf, 0.5])
    must, may = so.kept_sets(x, 2, 1.0)          # the cut falls inside the tie: all three stay
    assert must.tolist() == [True, False, True, True, True, False, False, False]
    assert np.array_equal(must, may)
    must, _ = so.kept_sets(x, 0, 0.0)            # top_p <= 0: the maximum value group
    assert must.tolist() == [True] + [False] * 7
    must, _ = so.kept_sets(x, 0, -1.0)
    assert must.tolist() == [True] + [False] * 7
    z = np.exp(x - 3.0).sum()
    p = float(np.exp(0.0) + 1.5 * np.exp(-1.0)) / z   # the target ends inside the tie of 2.0
    must, may = so.kept_sets(x, 0, p)
    assert must.tolist() == [True, False, True, True, True, False, False, False]
    assert np.array_equal(must, may)
    # a -inf logit is in no support, and never drawn
    o = so.sample_row(x, 1.0, seed=1, counter=0)
    assert not o.must_keep[6] and o.must_keep.sum() == 7


def _chi2_quantile(df: int, alpha: float) -> float:
    try:
        from scipy.stats import chi2
        return float(chi2.isf(alpha, df))
    except ImportError:
        z = statistics.NormalDist().inv_cdf(1.0 - alpha)   # Wilson-Hilferty
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def test_draw_fits_the_renormalised_softmax():
    """Many seeds on one row (V = 64, top-k 20, top-p 0.9): the oracle's tokens follow the
    softmax renormalised over the kept set (chi-square at significance 1e-6)."""
    V, N, T = 64, 40000, 0.9
    g = torch.Generator().manual_seed(5)
    lg = (torch.randn(V, generator=g) * 1.5).to(torch.bfloat16).float().numpy()
    x = so.scaled(lg, T)
    must, may = so.kept_sets(x, 20, 0.9)
    assert np.array_equal(must, may) and 3 <= must.sum() <= 20
    with np.errstate(over="ignore"):
        h = so.splitmix64(np.asarray(so.counter_base(0, 11), dtype=np.uint64)
                          + np.arange(V, dtype=np.uint64))
    seeds = np.arange(N, dtype=np.uint64) * np.uint64(7919) + np.uint64(1)
    u = so.uniform_from_raw(so.splitmix64(seeds[:, None] ^ h[None, :])).astype(np.float64)
    y = np.where(must[None, :], x[None, :] - np.log(-np.log(u)), -np.inf)
    tok = y.argmax(1)
    # the vectorised draw above is the oracle's own
    for b in (0, 1, N - 1):
        assert so.sample_row(lg, T, 20, 0.9, seed=int(seeds[b]), counter=11).token == tok[b]
    idx = np.nonzero(must)[0]
    prob = np.exp(x[idx] - x[idx].max())
    prob /= prob.sum()
    expect = N * prob
    assert expect.min() >= 5.0
    obs = np.bincount(tok, minlength=V)
    assert obs[~must].sum() == 0
    chi2 = float((((obs[idx] - expect) ** 2) / expect).sum())
    bound = _chi2_quantile(len(idx) - 1, 1e-6)
    assert chi2 < bound, (chi2, bound, len(idx))


def test_gpu_test_inputs_are_mostly_decisive():
    """The exact inputs of tests/test_sampling_gpu.py: at most 5 % of the rows of the whole
    matrix (and of the step-keyed and mixed repeats) are undecided by the oracle."""
    total = bad = 0
    share = {}
    for V in so.VOCABS:
        o = so.matrix_oracle(V)
        nd = sum(not r.decisive for r in o)
        share[V] = f"{nd}/{len(o)}"
        total += len(o)
        bad += nd
    for name, o in (("step", so.step_oracle()), ("mixed", so.mixed_oracle())):
        nd = sum(not r.decisive for r in o)
        share[name] = f"{nd}/{len(o)}"
        assert nd <= so.MAX_NON_DECISIVE * len(o), share
    print("non-decisive rows:", share)
    assert bad <= so.MAX_NON_DECISIVE * total, share
    # the top_p = 0 row keeps the maximum value group only
    for V in so.VOCABS:
        c, r = so.matrix_case(V), so.matrix_oracle(V)[-1]
        mx = c.logits[-1].float().max()
        assert np.array_equal(r.must_keep, (c.logits[-1].float() == mx).numpy())


def test_support_rows_are_unambiguous():
    for name, lg, k, p in so.support_rows():
        assert torch.equal(lg.to(torch.bfloat16).float(), lg), name
        x = so.scaled(lg.numpy(), 1.0)
        must, may = so.kept_sets(x, k, p)
        must, may = must & (x > -np.inf), may & (x > -np.inf)
        assert np.array_equal(must, may), name
        pr = np.exp(x[must] - x[must].max())
        assert (pr / pr.sum()).min() >= 0.02, name
        o = so.sample_row(lg.numpy(), 1.0, k, p, seed=9, counter=1)
        assert np.array_equal(o.must_keep, must), name
    by = {n: (lg, k, p) for n, lg, k, p in so.support_rows()}
    lg, k, p = by["topk_tie"]
    assert int(so.kept_sets(lg.double().numpy(), k, p)[0].sum()) == 5 > k
    lg, k, p = by["topp_tie"]
    assert int(so.kept_sets(lg.double().numpy(), k, p)[0].sum()) == 5
