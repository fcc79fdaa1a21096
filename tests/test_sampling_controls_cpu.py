"""The sampling-controls oracle (tests/sampling_controls_oracle.py) checked on its own, the
conditions its fixed cases must meet, the torch reference paths of ``ops`` against it, and
mutated implementations that it has to reject."""
import math
from collections import Counter

import numpy as np
import pytest
import torch

import sampling_controls_oracle as sc
import sampling_oracle as so
from distributed_llm_inference import ops
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16
SMALL = (8, 1003)


# ------------------------------------------------------------------ oracle self-checks (V = 8)
L8 = np.array([2.0, -2.0, 1.0, 0.5, -1.0, 3.0, 0.0, 4.0])


def test_repetition_on_a_positive_and_a_negative_logit():
    in_prompt = np.array([1, 1, 0, 0, 0, 0, 0, 0], dtype=bool)
    o = sc.penalise_row(L8, in_prompt, np.zeros(8, dtype=int), 2.0, 0.0, 0.0)
    assert o.value.tolist() == [1.0, -4.0, 1.0, 0.5, -1.0, 3.0, 0.0, 4.0]
    assert o.touched.tolist() == in_prompt.tolist() and o.exact
    assert o.expect.float().tolist() == o.value.tolist()


def test_frequency_and_presence_over_counts_0_1_3():
    n = np.array([0, 0, 1, 3, 0, 0, 0, 0])
    o = sc.penalise_row(L8, np.zeros(8, dtype=bool), n, 1.0, 0.5, 1.0)
    # count 0: untouched; count 1: 1.0 - 0.5 - 1.0; count 3: 0.5 - 1.5 - 1.0
    assert o.value.tolist() == [2.0, -2.0, -0.5, -2.0, -1.0, 3.0, 0.0, 4.0]
    assert o.touched.tolist() == (n > 0).tolist()
    # all three at once on a generated token: (0.5 / 2) - 1.5 - 1.0
    o = sc.penalise_row(L8, np.zeros(8, dtype=bool), n, 2.0, 0.5, 1.0)
    assert o.value[3] == -2.25 and o.value[2] == -1.0


def test_prompt_only_token_is_untouched_by_frequency_and_presence():
    in_prompt = np.array([0, 0, 0, 0, 0, 1, 0, 0], dtype=bool)
    o = sc.penalise_row(L8, in_prompt, np.zeros(8, dtype=int), 1.0, 2.0, 2.0)
    assert o.value.tolist() == L8.tolist()
    assert o.touched.tolist() == in_prompt.tolist()     # (seen: stored, with the same value)
    o = sc.penalise_row(L8, in_prompt, np.zeros(8, dtype=int), 1.5, 2.0, 2.0)
    assert o.value[5] == 2.0 and np.delete(o.value, 5).tolist() == np.delete(L8, 5).tolist()


def test_neg_inf_stays_neg_inf_and_is_not_ambiguous():
    l = L8.copy()
    l[2] = -np.inf
    o = sc.penalise_row(l, np.zeros(8, dtype=bool), np.array([0, 0, 5, 0, 0, 0, 0, 0]), 1.5, -1.0,
                        -1.0)
    assert o.value[2] == -np.inf and o.exact and o.expect[2].item() == -math.inf


def test_ambiguity_needs_a_rounded_operation_near_a_midpoint():
    first = np.array([1] + [0] * 7, dtype=bool)
    none = np.zeros(8, dtype=int)
    # 2.21875 / 0.8 = 2.7734375 is the midpoint of the bf16 neighbours 2.765625 and 2.78125; with
    # r = fp32(0.8) the quotient misses it by 4e-8, less than one fp32 rounding: ambiguous
    l = np.zeros(8)
    l[0] = 2.21875
    o = sc.penalise_row(l, first, none, 0.8, 0, 0)
    assert o.ambiguous.tolist() == [True] + [False] * 7 and not o.exact
    assert {o.lo[0].item(), o.hi[0].item()} == {2.765625, 2.78125}
    # 1.5 * -1.671875 = -2.5078125 is a midpoint too, but the product is exact in fp32: RNE
    # decides (ties to even), nothing is ambiguous
    l[0] = -1.671875
    o = sc.penalise_row(l, first, none, 1.5, 0, 0)
    assert o.exact and o.value[0] == -2.5078125 and o.expect[0].item() == -2.5
    # away from a midpoint a rounded quotient is not ambiguous either
    l[0] = 2.0
    assert sc.penalise_row(l, first, none, 1.1, 0, 0).exact


def test_table_row_words():
    w = sc.table_row(8, [1, 1, 5], [5, 5, 2])
    assert w.tolist() == [0, sc.PROMPT_BIT, 1, 0, 0, sc.PROMPT_BIT + 2, 0, 0]
    assert ops.PENALTY_PROMPT_BIT == sc.PROMPT_BIT


def test_min_p_zero_is_off_and_one_keeps_the_maximum_group():
    l = np.array([1.0, 3.0, 3.0, 2.5, -1.0, 0.0, 3.0, 2.0])
    off = sc.sample_row(l, 0.7, min_p=0.0, seed=5, counter=9)
    ref_ = so.sample_row(l, 0.7, seed=5, counter=9)
    assert off.token == ref_.token and off.may_keep.all()
    one = sc.sample_row(l, 0.7, min_p=1.0, seed=5, counter=9)
    assert one.may_keep.tolist() == one.must_keep.tolist() == (l == 3.0).tolist()
    assert one.token in (1, 2, 6)
    # exp(-0.5 / 0.7) = 0.49 of the maximum: 2.5 is kept at m = 0.3 and dropped at m = 0.6
    assert sc.sample_row(l, 0.7, min_p=0.3).may_keep.tolist() == (l >= 2.5).tolist()
    assert sc.sample_row(l, 0.7, min_p=0.6).may_keep.tolist() == (l == 3.0).tolist()
    # greedy rows ignore it
    assert sc.sample_row(l, 0.0, min_p=1.0).token == 1


# ------------------------------------------------------------------ conditions on the fixed cases
def test_cases_cover_what_they_claim():
    for V in sc.VOCABS:
        c = sc.case(V)
        lens = {len(p) + len(o) for p, o in zip(c.prompts, c.outputs)}
        assert {0, 1, 64} <= lens
        tab = c.table.numpy().astype(np.int64)
        cnt = tab & 0x7FFFFFFF
        assert cnt.max() >= 40 or V == 8
        assert (tab[:, 0] != 0).any() and (tab[:, V - 1] != 0).any()
        assert ((tab < 0) & (cnt == 0)).any() and ((tab > 0)).any() and ((tab < 0) & (cnt > 0)).any()
        slots = c.pen_slot.tolist()
        assert -1 in slots and slots != sorted(slots) and set(slots) - {-1} == set(range(sc.SLOTS))
        neg = [r for r, s in enumerate(slots) if s == sc.NEG_INF_SLOT]
        assert all(c.base.logits[r, c.prompts[sc.NEG_INF_SLOT][0]] == -math.inf for r in neg)
        for vals, t in ((sc.REPS, c.rep), (sc.FREQS, c.freq), (sc.PRESS, c.pres),
                        (sc.MINPS, c.min_p)):
            assert {round(v, 4) for v in t.tolist()} == {round(sc.f32(v), 4) for v in vals}
        assert all(c.base.temperature[r] == 0 and slots[r] >= 0 for r in sc.GREEDY_ROWS)


def test_ambiguous_elements_are_rare():
    """At most 1 % of the touched elements are ambiguous (from the oracle alone)."""
    touched = amb = 0
    for V in sc.VOCABS:
        for o in sc.penalty_oracle(V):
            if o is not None:
                touched += int(o.touched.sum())
                amb += int(o.ambiguous.sum())
    assert touched > 1000
    assert amb <= sc.MAX_AMBIGUOUS * touched, (amb, touched)


def test_most_rows_are_exact_and_decisive():
    """At least 90 % of the rows of the whole case set are both exact and decisive: the token
    equality of the GPU test is not vacuous."""
    good = total = 0
    for V in sc.VOCABS:
        for row, o in enumerate(sc.token_oracle(V)):
            total += 1
            good += bool(o.decisive and sc.row_exact(V, row))
    assert good >= sc.MIN_EXACT_DECISIVE * total, (good, total)
    only = [o for V in sc.VOCABS for o in sc.min_p_only_oracle(V)]
    assert sum(o.decisive for o in only) >= sc.MIN_EXACT_DECISIVE * len(only)


# ------------------------------------------------------------------ ops.reference (CPU paths)
def _apply_ref(V, dtype):
    c = sc.case(V)
    lg = c.base.logits.to(dtype)
    out = ops.apply_penalties(lg.clone(), c.table.clone(), c.pen_slot, c.rep, c.pres, c.freq)
    return lg, out


@pytest.mark.parametrize("V", sc.VOCABS)
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
def test_reference_apply_penalties_equals_the_oracle(V, dtype):
    lg, out = _apply_ref(V, dtype)
    for row, o in enumerate(sc.penalty_oracle(V)):
        if o is None:
            assert torch.equal(out[row].view(torch.int16 if dtype == BF else torch.int32),
                               lg[row].view(torch.int16 if dtype == BF else torch.int32))
            continue
        bad = sc.penalty_mismatches(out[row], lg[row], o)
        assert not bad, (V, row, bad[:5])
        if o.exact and dtype == BF:
            assert torch.equal(out[row].view(torch.int16), o.expect.view(torch.int16))


def _counter_model(V, slots, steps):
    """Python model of a table: per slot (prompt set, Counter of outputs) -> int32 words."""
    state = [(set(), Counter()) for _ in range(slots)]
    for slot, kind, reset, toks in steps:
        if reset:
            state[slot] = (set(), Counter())
        if kind == 0:
            state[slot][0].update(toks)
        else:
            state[slot][1].update(toks)
    tab = np.zeros((slots, V), dtype=np.int64)
    for s, (pr, cnt) in enumerate(state):
        for t in pr:
            tab[s, t] += sc.PROMPT_BIT
        for t, n in cnt.items():
            tab[s, t] += n
    return torch.from_numpy(tab.astype(np.int32))


FEED_STEPS = [  # (slot, kind, reset, tokens)
    (2, 0, 1, [5, 5, 0, 7, 3]), (2, 1, 0, [7, 7, 7, 1, 0]),
    (0, 0, 1, [1]), (3, 1, 1, [6] * 40 + [2, 2]),
]


def test_reference_feed_and_update_match_a_counter_model():
    V, S = 8, 4
    tab = ops.penalty_table(S, V, "cpu")
    tab[3] = 77                                     # stale words of an earlier owner
    segs = [(s, k, r, len(t)) for s, k, r, t in FEED_STEPS]
    toks = [t for st in FEED_STEPS for t in st[3]]
    ops.penalty_feed(tab, segs, toks)
    assert torch.equal(tab, _counter_model(V, S, FEED_STEPS))
    # without reset counts accumulate; a reused slot with reset shows none of its past
    more = [(2, 1, 0, [7, 4]), (3, 0, 1, [0, 1])]
    ops.penalty_feed(tab, [(s, k, r, len(t)) for s, k, r, t in more], [7, 4, 0, 1])
    assert torch.equal(tab, _counter_model(V, S, FEED_STEPS + more))
    # update: one count per row with a slot, at its token
    slot = torch.tensor([2, -1, 0, 2], dtype=torch.int32)
    tok = torch.tensor([4, 3, 1, 4], dtype=torch.int32)
    ops.penalty_update(tab, slot, tok)
    upd = [(2, 1, 0, [4, 4]), (0, 1, 0, [1])]
    assert torch.equal(tab, _counter_model(V, S, FEED_STEPS + more + upd))
    with pytest.raises(ValueError):
        ops.penalty_feed(tab, [(S, 0, 0, 1)], [0])
    # a reset after another segment of its slot would be ordered differently on the GPU (all
    # resets first): refused on both paths
    with pytest.raises(ValueError, match="first segment"):
        ops.penalty_feed(tab, [(1, 1, 0, 1), (1, 0, 1, 1)], [1, 2])


@pytest.mark.parametrize("V", SMALL)
def test_reference_sample_with_min_p_stays_in_may_keep(V):
    c = sc.case(V)
    b = c.base
    oracle = sc.min_p_only_oracle(V)
    for draw in range(8):
        tok = ref.sample(b.logits, b.temperature, b.top_k, b.top_p, seeds=b.seeds,
                         counters=b.counters + draw, min_p=c.min_p)
        for row, (t, o) in enumerate(zip(tok.tolist(), oracle)):
            if b.temperature[row] > 0:
                assert o.may_keep[t], (V, row, t)
    # a None min_p is the sampler without the predicate
    g = torch.Generator().manual_seed(3)
    g2 = torch.Generator().manual_seed(3)
    assert torch.equal(ref.sample(b.logits, b.temperature, b.top_k, b.top_p, g),
                       ref.sample(b.logits, b.temperature, b.top_k, b.top_p, g2,
                                  min_p=torch.zeros_like(c.min_p)))


# ------------------------------------------------------------------ mutation check
def _mutant_apply(V, kind):
    """apply_penalties with one rule broken, in float64 then bf16."""
    c = sc.case(V)
    lg = c.base.logits.clone()
    tab = c.table.numpy().astype(np.int64)
    for row, s in enumerate(sc.ROW_SLOT):
        if s < 0:
            continue
        w = tab[s]
        n = (w & 0x7FFFFFFF).astype(np.float64)
        seen, gen = w != 0, (w & 0x7FFFFFFF) > 0
        r, f, p = (sc.f32(t[row]) for t in (c.rep, c.freq, c.pres))
        l = lg[row].double().numpy()
        with np.errstate(invalid="ignore"):
            if kind == "rep_multiplies_positive":
                a = np.where(l > 0, l * r, l * r)
            else:
                a = np.where(l > 0, l / r, l * r)
            v = np.where(seen, a, l)
            v = np.where(gen, v - f * n, v)
            v = np.where(seen if kind == "presence_on_prompt" else gen, v - p, v)
        lg[row] = sc._bf16(v)
    return lg


@pytest.mark.parametrize("kind", ["presence_on_prompt", "rep_multiplies_positive"])
def test_mutated_penalties_fail_the_oracle(kind):
    V = 1003
    orig = sc.case(V).base.logits
    out = _mutant_apply(V, kind)
    bad = sum(len(sc.penalty_mismatches(out[row], orig[row], o))
              for row, o in enumerate(sc.penalty_oracle(V)) if o is not None)
    assert bad > 0
    # (and the unmutated evaluation passes the same comparison)
    good = _mutant_apply(V, "none")
    assert not any(sc.penalty_mismatches(good[row], orig[row], o)
                   for row, o in enumerate(sc.penalty_oracle(V)) if o is not None)


def test_min_p_compared_before_the_temperature_fails_the_oracle():
    """A sampler that applies ``l >= max(l) + ln m`` to the unscaled logits keeps another set
    whenever T != 1: for some row it is not between the oracle's must_keep and may_keep."""
    V = 1003
    c = sc.case(V)
    lg = c.base.logits.double().numpy()
    broken = right = 0
    for row, o in enumerate(sc.min_p_only_oracle(V)):
        m, T = float(c.min_p[row]), float(c.base.temperature[row])
        if not (m > 0 and T > 0):
            continue
        base = so.sample_row(lg[row], T, int(c.base.top_k[row]), float(c.base.top_p[row]),
                             int(c.base.seeds[row]), row, int(c.base.counters[row]))
        for scale, tally in ((1.0, "broken"), (1.0 / sc.f32(T), "right")):
            x = lg[row] * scale
            keep = base.may_keep & (x >= x.max() + math.log(sc.f32(m)))
            ok = bool((o.must_keep <= keep).all() and (keep <= o.may_keep).all())
            if tally == "broken":
                broken += not ok
            else:
                right += not ok and base.must_keep.tolist() == base.may_keep.tolist()
    assert broken > 0 and right == 0
