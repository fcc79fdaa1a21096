"""The penalty kernels (csrc/kernels/penalty.hip) and the sampler's min-p predicate
(csrc/kernels/sampling.hip) against their CPU oracle (tests/sampling_controls_oracle.py).

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
from collections import Counter

import numpy as np
import pytest
import torch

import sampling_controls_oracle as sc
import sampling_oracle as so
from distributed_llm_inference import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DTYPES = [BF, torch.float32]
_IDS = ["bf16", "f32"]
GUARD = 24          # elements after each logits row (row_stride = V + GUARD: keeps 16-byte rows
                    # for V % 8 == 0) and words after the table


def _guarded_logits(gpu, logits, dtype):
    """[B, V] view of a [B, V + GUARD] buffer whose guard columns hold a pattern."""
    B, V = logits.shape
    buf = torch.full((B, V + GUARD), 7.5, dtype=dtype, device=gpu)
    buf[:, :V] = logits.to(gpu).to(dtype)
    return buf, buf[:, :V]


def _guarded_table(gpu, table):
    """The table as a contiguous [slots, V] view at the front of a longer buffer."""
    S, V = table.shape
    buf = torch.full((S * V + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    view = buf[: S * V].view(S, V)
    view.copy_(table)
    return buf, view


def _params(gpu, c):
    return [t.to(gpu) for t in (c.pen_slot, c.rep, c.pres, c.freq)]


_APPLIED = {}


def _applied(gpu, V, dtype):
    """(input logits, penalised logits, guard columns, table buffer) on the CPU, one launch per
    (V, dtype) for all the tests that read it."""
    if (V, dtype) not in _APPLIED:
        c = sc.case(V)
        buf, lg = _guarded_logits(gpu, c.base.logits, dtype)
        tbuf, tab = _guarded_table(gpu, c.table)
        ops.apply_penalties(lg, tab, *_params(gpu, c))
        torch.cuda.synchronize()
        _APPLIED[(V, dtype)] = (c.base.logits.to(dtype), lg.cpu(), buf[:, V:].cpu(), tbuf.cpu())
    return _APPLIED[(V, dtype)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("V", sc.VOCABS)
def test_penalty_apply_equals_the_oracle(gpu, V, dtype):
    """Bit-equal to the oracle on every non-ambiguous element (bf16) / within its bound (fp32),
    a neighbour on ambiguous ones; untouched elements, rows with slot -1, the guard bytes after
    each row and the table are unchanged."""
    orig, got, guard, tbuf = _applied(gpu, V, dtype)
    c = sc.case(V)
    bits = torch.int16 if dtype == BF else torch.int32
    for row, o in enumerate(sc.penalty_oracle(V)):
        if o is None:
            assert torch.equal(got[row].view(bits), orig[row].view(bits)), f"slot -1 row {row}"
            continue
        bad = sc.penalty_mismatches(got[row], orig[row], o)
        assert not bad, f"V={V} row {row}: {len(bad)} mismatches, first at {bad[:5]}: " \
                        f"{got[row][bad[:5]].tolist()} want {o.value[bad[:5]]}"
    assert (guard == 7.5).all()
    assert torch.equal(tbuf[: c.table.numel()].view_as(c.table), c.table)
    assert (tbuf[c.table.numel():] == 0x5A5A5A5A).all()


def test_penalty_apply_unaligned_rows_take_the_scalar_path(gpu):
    """A [B, V] view that starts 2 bytes into its buffer (V % 4 == 0, odd offset): same result."""
    V = 32776
    c = sc.case(V)
    B = c.base.logits.shape[0]
    buf = torch.zeros(B * V + 1, dtype=BF, device=gpu)
    lg = buf[1:].view(B, V)
    lg.copy_(c.base.logits)
    ops.apply_penalties(lg, c.table.to(gpu), *_params(gpu, c))
    assert torch.equal(lg.cpu().view(torch.int16), _applied(gpu, V, BF)[1].view(torch.int16))
    assert buf[0].item() == 0


# ------------------------------------------------------------------ feed / update
def _model(V, slots, steps):
    state = [(set(), Counter()) for _ in range(slots)]
    for slot, kind, reset, toks in steps:
        if reset:
            state[slot] = (set(), Counter())
        state[slot][kind].update(toks)
    tab = np.zeros((slots, V), dtype=np.int64)
    for s, (pr, cnt) in enumerate(state):
        for t in pr:
            tab[s, t] += sc.PROMPT_BIT
        for t, n in cnt.items():
            tab[s, t] += n
    return torch.from_numpy(tab.astype(np.int32))


def _feed(tab, steps):
    ops.penalty_feed(tab, [(s, k, r, len(t)) for s, k, r, t in steps],
                     [t for st in steps for t in st[3]])


@pytest.mark.parametrize("V", [1003, 128256])
def test_penalty_feed_matches_the_counter_model(gpu, V):
    S = 5
    g = np.random.default_rng(V)
    long_prompt = [int(t) for t in g.integers(0, V, 3000)] + [0, V - 1, V - 1]
    outs = [int(t) for t in g.integers(0, 50, 300)] + [V - 1] * 40
    steps = [(3, 0, 1, long_prompt), (3, 1, 0, outs),       # a chunk straddling prompt | outputs
             (0, 0, 1, [5]), (4, 1, 1, [7] * 33)]
    tbuf, tab = _guarded_table(gpu, torch.full((S, V), 77, dtype=torch.int32))
    tab[1].zero_()
    tab[2].zero_()
    _feed(tab, steps)
    want = _model(V, S, steps)
    want[1] = 0
    want[2] = 0
    assert torch.equal(tab.cpu(), want)
    # a second sequence into a reused slot with reset shows none of the first; without reset
    # counts accumulate
    more = [(3, 0, 1, [1, 2, 2]), (4, 1, 0, [7, 8]), (4, 0, 0, [8])]
    _feed(tab, more)
    want2 = _model(V, S, steps + more)
    want2[1] = 0
    want2[2] = 0
    assert torch.equal(tab.cpu(), want2)
    assert (tab[3].cpu() != 0).sum() == 2
    assert (tbuf[S * V:] == 0x5A5A5A5A).all()


@pytest.mark.parametrize("V", [1003, 128256])
def test_update_counts_the_sampled_token(gpu, V):
    """After ``sample``, exactly one word per penalised row grew by one, at the returned token;
    rows with slot -1 change nothing."""
    c = sc.case(V)
    b = c.base
    tbuf, tab = _guarded_table(gpu, c.table)
    slot = c.pen_slot.to(gpu)
    tok = ops.sample(b.logits.to(gpu), temperature=b.temperature.to(gpu), top_k=b.top_k.to(gpu),
                     top_p=b.top_p.to(gpu), seeds=b.seeds.to(gpu), counters=b.counters.to(gpu))
    ops.penalty_update(tab, slot, tok)
    want = c.table.clone().long()
    for s, t in zip(c.pen_slot.tolist(), tok.cpu().tolist()):
        if s >= 0:
            want[s, t] += 1
    assert torch.equal(tab.cpu().long(), want)
    assert (want - c.table).sum() == sum(s >= 0 for s in sc.ROW_SLOT)
    assert (tbuf[c.table.numel():] == 0x5A5A5A5A).all()


# ------------------------------------------------------------------ tokens
def _check_tokens(tok, oracle, what, exact=None):
    V = oracle[0].may_keep.shape[0]
    assert ((tok >= 0) & (tok < V)).all(), (what, tok)
    outside = [b for b, (t, o) in enumerate(zip(tok, oracle)) if not o.may_keep[t]]
    assert not outside, f"{what}: tokens outside may_keep in rows {outside}: {tok[outside]}"
    wrong = [(b, int(t), o.token, round(o.margin, 4))
             for b, (t, o) in enumerate(zip(tok, oracle))
             if o.decisive and (exact is None or exact[b]) and t != o.token]
    assert not wrong, f"{what}: (row, kernel, oracle, margin) {wrong}"


def _sample(gpu, logits, c, min_p):
    b = c.base
    return ops.sample(logits, temperature=b.temperature.to(gpu), top_k=b.top_k.to(gpu),
                      top_p=b.top_p.to(gpu), seeds=b.seeds.to(gpu), counters=b.counters.to(gpu),
                      min_p=None if min_p is None else min_p.to(gpu)).cpu().long().numpy()


@pytest.mark.parametrize("path", ["regs", "radix"])
@pytest.mark.parametrize("V", sc.VOCABS)
def test_apply_then_sample_equals_the_oracle(gpu, V, path):
    """apply -> sample against the oracle's sample_row on the oracle-penalised logits: every
    token lies in may_keep, every exact and decisive row is the oracle's token.  ``regs``: bf16
    logits (the register path where V % 8 == 0); ``radix``: the penalised bf16 values as fp32
    logits (the radix path at every V)."""
    c = sc.case(V)
    lg = c.base.logits.to(gpu)
    ops.apply_penalties(lg, c.table.to(gpu), *_params(gpu, c))
    if path == "radix":
        lg = lg.float()
    tok = _sample(gpu, lg, c, c.min_p)
    exact = [sc.row_exact(V, row) for row in range(len(sc.ROW_SLOT))]
    _check_tokens(tok, sc.token_oracle(V), f"V={V} {path}", exact)
    for row in sc.GREEDY_ROWS:      # greedy rows are penalised too (and ignore min_p = 1)
        if exact[row]:
            assert tok[row] == int(sc.penalised_logits(V)[row].float().argmax())


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("V", sc.VOCABS)
def test_min_p_alone_equals_the_oracle(gpu, V, dtype):
    c = sc.case(V)
    tok = _sample(gpu, c.base.logits.to(gpu).to(dtype), c, c.min_p)
    _check_tokens(tok, sc.min_p_only_oracle(V), f"min_p V={V} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("V", sc.VOCABS)
def test_without_min_p_the_sampler_is_unchanged(gpu, V, dtype):
    """``min_p=None`` returns the tokens of sampling_oracle's matrix case, and so does an
    all-zero ``min_p`` (the kernels with the predicate, switched off per row)."""
    m = so.matrix_case(V)
    c = sc.Case(m, V, [], [], None, None, None, None, None, None)
    lg = m.logits.to(gpu).to(dtype)
    none = _sample(gpu, lg, c, None)
    _check_tokens(none, so.matrix_oracle(V), f"no min_p V={V} {dtype}")
    zero = _sample(gpu, lg, c, torch.zeros(m.logits.shape[0]))
    assert np.array_equal(none, zero)


# ------------------------------------------------------------------ rejected inputs
def test_bindings_reject_bad_inputs(gpu):
    V, S, B = 64, 4, 3
    lg = torch.zeros(B, V, dtype=BF, device=gpu)
    tab = torch.zeros(S, V, dtype=torch.int32, device=gpu)
    slot = torch.zeros(B, dtype=torch.int32, device=gpu)
    one = torch.ones(B, device=gpu)
    tok = torch.zeros(B, dtype=torch.int32, device=gpu)
    ops.apply_penalties(lg, tab, slot, one, one, one)       # (the well-formed call passes)
    with pytest.raises(RuntimeError, match="int32"):
        ops.apply_penalties(lg, tab.long(), slot, one, one, one)
    with pytest.raises(RuntimeError, match="V ="):
        ops.apply_penalties(lg, torch.zeros(S, V + 8, dtype=torch.int32, device=gpu), slot, one,
                            one, one)
    wide = torch.zeros(S, 2 * V, dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.apply_penalties(lg, wide[:, :V], slot, one, one, one)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.penalty_update(wide[:, :V], slot, tok)
    with pytest.raises(RuntimeError, match="int32"):
        ops.penalty_feed(tab.long(), [(0, 0, 0, 1)], [1])
    with pytest.raises(RuntimeError, match="slot"):
        ops.penalty_feed(tab, [(S, 0, 1, 1)], [1])
    with pytest.raises(RuntimeError, match="first segment"):
        ops.penalty_feed(tab, [(1, 1, 0, 1), (1, 0, 1, 1)], [1, 2])
    with pytest.raises(RuntimeError, match="cover"):
        ops.penalty_feed(tab, [(0, 0, 1, 2)], [1])
    with pytest.raises(RuntimeError, match="B entries"):
        ops.apply_penalties(lg, tab, slot[:2], one, one, one)
    torch.cuda.synchronize()
    assert not tab.any() and not lg.any()
