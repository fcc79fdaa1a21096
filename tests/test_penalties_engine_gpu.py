"""Repetition / presence / frequency penalties and min-p through the engine on the GPU: captured
decode graphs (captured lazily, inside the first decode step that needs them), lookahead, the
rotating head's split, preemption, and the device table against a host model.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
from collections import Counter

import pytest
import torch

from distributed_llm_inference.config import CacheConfig, ModelSpec, ServeConfig
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.scheduler import Scheduler
from distributed_llm_inference.runtime.sequence import SamplingParams, Sequence

pytestmark = pytest.mark.gpu

SPEC = ModelSpec(name="t", vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=4,
                 num_heads=8, num_kv_heads=4, head_dim=32, rope_theta=10000.0,
                 max_position_embeddings=4096)
PROMPTS = [list(range(3, 40)), [7, 8, 9], list(range(200, 330)), [11], [5, 5, 5, 6], [900, 1, 2]]
PROMPT_BIT = -(1 << 31)


def _engine(pp=1, graphs=True, mbs=0, slots=4, num_blocks=256):
    cfg = EngineConfig(model="t", pp=pp, seed=5,
                       cache=CacheConfig(num_blocks=num_blocks, block_size=64, max_chunk=256),
                       serve=ServeConfig(max_batch_size=8, max_num_batched_tokens=512,
                                         max_seq_len=1024, use_graphs=graphs, num_micro_batches=mbs,
                                         graph_batch_sizes=[1, 2, 4, 8], penalty_slots=slots))
    return LLMEngine(SPEC, device="cuda:0", cfg=cfg)


def _params(max_tokens=12):
    """Mixed requests: penalised (greedy and seeded), min-p only, plain."""
    kinds = [dict(repetition_penalty=1.3, frequency_penalty=0.5),
             dict(),
             dict(temperature=0.8, min_p=0.1),
             dict(temperature=0.8, presence_penalty=1.0, min_p=0.05),
             dict(repetition_penalty=0.8, presence_penalty=-1.0, frequency_penalty=2.0),
             dict(temperature=0.8, top_k=40)]
    return [SamplingParams(max_tokens=max_tokens, seed=50 + i, ignore_eos=True, **k)
            for i, k in enumerate(kinds)]


def _run(eng, params=None, lookahead=None):
    params = params or _params()
    if lookahead is not None:
        eng.pipeline.lookahead = lookahead and eng.pipeline.sched.M == 1
    seqs = [Sequence(list(p), sp) for p, sp in zip(PROMPTS, params)]
    for s in seqs:
        eng.pipeline.sched.add(s)
    done = {s.seq_id: s for s in eng.pipeline.run_until_done()}
    return [done[s.seq_id].output for s in seqs]


_EAGER = {}


def _eager(mbs=0):
    if mbs not in _EAGER:
        _EAGER[mbs] = _run(_engine(graphs=False, mbs=mbs), lookahead=False)
    return _EAGER[mbs]


def test_graph_decode_equals_eager(gpu):
    """The graph engine is built without warm-up, so the first penalised decode step captures
    its graph inside ``_execute``: the two warm-up runs of the capture must leave the table (and
    the logits) alone, or the step would count - and penalise - its own token early."""
    eng = _engine(graphs=True)
    assert not eng.executors[0]._graphs
    got = _run(eng, lookahead=False)
    keys = set(eng.executors[0]._graphs)
    assert any(isinstance(k, int) for k in keys) or any(k[1] == "min_p" for k in keys
                                                        if isinstance(k, tuple))
    assert got == _eager()
    plain = _run(_engine(graphs=True), [SamplingParams(max_tokens=12, seed=50 + i, ignore_eos=True,
                                                       temperature=p.temperature, top_k=p.top_k)
                                        for i, p in enumerate(_params())], lookahead=False)
    assert sum(a != b for a, b in zip(got, plain)) >= 2     # (the controls do change tokens)


def _no_capture(*a, **k):
    raise AssertionError("a decode graph was captured after warm-up")


def test_warmed_up_executor_replays_min_p_graphs(gpu, monkeypatch):
    """An executor prepared the way a pipeline rank prepares it (every graph captured by
    ``warmup_graphs(min_p=True)`` before the first request, none afterwards): steps with a min-p
    row replay the bucket's min-p variant, steps with penalised rows the plain one, and the
    tokens are the eager engine's."""
    eng = _engine(graphs=True)
    ex = eng.executors[0]
    ex.warmup_graphs(variants=(True,), min_p=True)
    assert set(ex._graphs) == set(ex.graph_sizes) | {(r, "min_p") for r in ex.graph_sizes}
    monkeypatch.setattr(ex, "_capture", _no_capture)
    replayed = []
    for key, entry in ex._graphs.items():
        real = entry.graph

        class Spy:
            def __init__(self, g, key):
                self.g, self.key = g, key

            def replay(self):
                replayed.append(self.key)
                self.g.replay()

        entry.graph = Spy(real, key)
    assert _run(eng, lookahead=False) == _eager()
    assert any(isinstance(k, tuple) and k[1] == "min_p" for k in replayed)
    # the min-p requests finish with the others here, so every decode step had a min-p row
    plain = _run(eng, [SamplingParams(max_tokens=5, seed=50 + i, ignore_eos=True,
                                      repetition_penalty=1.2) for i in range(len(PROMPTS))][:4],
                 lookahead=False)
    assert len(plain) == 4 and any(isinstance(k, int) for k in replayed)
    # a stage that does not sample has no min-p variant to capture
    two = _engine(pp=2, graphs=True)
    two.executors[0].warmup_graphs(min_p=True)
    assert all(isinstance(k, int) for k in two.executors[0]._graphs)


def test_lookahead_equals_plain_decode(gpu):
    assert _run(_engine(graphs=True, mbs=1), lookahead=True) == _eager()


def test_rotating_head_split_equals_single_stage(gpu):
    """pp = 2 loopback with the head placed by HeadPolicy: steps with a penalised row sample on
    the last stage (where the table lives), the others end at the final norm and sample in a
    HeadRunner (min-p included) - the tokens of the single-stage engine."""
    from distributed_llm_inference.parallel.pipeline import _sample_tokens_to_host
    from distributed_llm_inference.runtime.head import HeadPolicy, HeadRunner
    # two waves: the penalised requests finish first (fewer tokens), then the steps rotate
    params = _params()
    for p in params:
        if p.has_penalty:
            p.max_tokens = 6
    ref = _run(_engine(pp=1, mbs=3), params)
    eng = _engine(pp=2, mbs=3)
    pipe = eng.pipeline
    last = pipe.executors[-1]
    assert last.pen_table is not None and pipe.executors[0].pen_table is None
    runner = HeadRunner(last.stage.head, last.device, last.max_num_seqs, True, last.graph_sizes)
    runner.warmup()      # as a pipeline rank does: both variants of every bucket, none later
    assert set(runner._graphs) == set(runner.graph_sizes) | {(r, "min_p")
                                                             for r in runner.graph_sizes}
    runner._capture = _no_capture
    policy = HeadPolicy(2, True, last.max_num_seqs)
    side = torch.cuda.Stream()
    orig, split, kept = pipe._issue, [], []

    def issue(plan):
        if not policy.offloaded(plan):
            kept.append(plan.penalised)
            return orig(plan)
        assert not plan.penalised
        x = None
        for ex in pipe.executors[:-1]:
            x = ex.execute(plan, x)
        h = last.execute(plan, x, project=False)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            tok = runner.run(plan, h).clone()
        torch.cuda.current_stream().wait_stream(side)
        pipe._last_tokens = tok
        pipe._results[plan.step] = _sample_tokens_to_host(tok)
        split.append(plan.uses_min_p)

    pipe._issue = issue
    got = _run(eng, params)
    assert any(split) and any(kept)      # min-p steps rotated, penalised steps stayed
    assert got == ref


def test_preemption_with_graphs_keeps_the_tokens(gpu):
    params = _params(max_tokens=40)
    ref = _run(_engine(graphs=True), params)
    eng = _engine(graphs=True, num_blocks=5)
    got = _run(eng, params)
    assert eng.pipeline.sched.preemptions > 0
    assert got == ref


def test_device_table_equals_the_host_model(gpu, monkeypatch):
    """Each penalised sequence's slot row, read just before the slot is released: bit 31 on its
    prompt's tokens, Counter(outputs) in the low bits - with two slots for three penalised
    requests (one waits for a slot and takes a used one) and preemption."""
    eng = _engine(graphs=True, slots=2, num_blocks=5)
    table = eng.executors[-1].pen_table
    assert table.shape == (2, SPEC.vocab_size) and table.dtype == torch.int32
    seen = []
    release = Scheduler._release_slot

    def spy(self, s):
        if s.pen_slot >= 0 and s.is_finished():
            seen.append((list(s.prompt), list(s.output), table[s.pen_slot].cpu()))
        release(self, s)

    monkeypatch.setattr(Scheduler, "_release_slot", spy)
    params = _params(max_tokens=40)
    _run(eng, params)
    assert eng.pipeline.sched.max_slots_held == 2
    assert len(seen) == sum(p.has_penalty for p in params) == 3
    for prompt, output, row in seen:
        want = torch.zeros(SPEC.vocab_size, dtype=torch.int64)
        for t in set(prompt):
            want[t] += PROMPT_BIT
        for t, n in Counter(output).items():
            want[t] += n
        assert torch.equal(row.long(), want)


def test_zero_slots(gpu):
    """penalty_slots = 0: no table, a penalised request is refused, min-p runs."""
    eng = _engine(slots=0)
    assert eng.executors[0].pen_table is None
    with pytest.raises(ValueError, match="penalty_slots"):
        eng.generate(PROMPTS[:1], SamplingParams(max_tokens=2, frequency_penalty=1.0))
    p = SamplingParams(max_tokens=8, temperature=0.8, seed=2, min_p=0.2, ignore_eos=True)
    a = [s.output for s in eng.generate(PROMPTS[:3], p)]
    b = [s.output for s in _engine(slots=0, graphs=False).generate(PROMPTS[:3], p)]
    assert a == b and all(len(o) == 8 for o in a)
    assert any(isinstance(k, tuple) and k[1] == "min_p" for k in eng.executors[0]._graphs)
