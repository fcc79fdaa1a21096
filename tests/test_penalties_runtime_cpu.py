"""Repetition / presence / frequency penalties and min-p through the runtime, on CPU engines:
request validation, the scheduler's penalty slots, the step plan's wire format, head placement,
and token equality across pipeline depth, micro-batches, lookahead and preemption."""
import multiprocessing as mp
import os
import socket
from collections import Counter

import pytest
import torch

from distributed_llm_inference.config import CacheConfig, ModelSpec, ServeConfig
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.executor import StepPlan
from distributed_llm_inference.runtime.head import HeadPolicy
from distributed_llm_inference.runtime.scheduler import Scheduler
from distributed_llm_inference.runtime.sequence import SamplingParams, Sequence

SPEC = ModelSpec(name="t", vocab_size=300, hidden_size=128, intermediate_size=256, num_layers=4,
                 num_heads=4, num_kv_heads=2, head_dim=32, rope_theta=10000.0,
                 max_position_embeddings=4096)
BS = 32
PROMPTS = [list(range(3 + i, 23 + i + (i % 3) * 4)) for i in range(8)]   # 20-28 tokens each
MAX_TOKENS = 24
PROMPT_BIT = -(1 << 31)


def _cfg(num_blocks=256, pp=1, mbs=0, seqs=8, slots=8):
    return EngineConfig(model="t", pp=pp, seed=3,
                        cache=CacheConfig(num_blocks=num_blocks, block_size=BS, max_chunk=64),
                        serve=ServeConfig(max_batch_size=seqs, max_num_batched_tokens=256,
                                          num_micro_batches=mbs, max_seq_len=256,
                                          use_graphs=False, penalty_slots=slots))


def _engine(**kw):
    return LLMEngine(SPEC, cfg=_cfg(**kw))


def _mixed_params(temperature=0.0, max_tokens=MAX_TOKENS):
    """Per prompt: penalised (each penalty alone and together), min-p only, and plain requests."""
    kinds = [dict(repetition_penalty=1.5), dict(), dict(frequency_penalty=0.5, min_p=0.05),
             dict(min_p=0.1), dict(presence_penalty=2.0), dict(),
             dict(repetition_penalty=0.8, presence_penalty=-1.0, frequency_penalty=2.0),
             dict(repetition_penalty=1.1, frequency_penalty=0.5, min_p=0.02)]
    return [SamplingParams(max_tokens=max_tokens, temperature=temperature, seed=100 + i,
                           ignore_eos=True, **k) for i, k in enumerate(kinds)]


def _run(eng, params, lookahead=None):
    if lookahead is not None:
        eng.pipeline.lookahead = lookahead and eng.pipeline.sched.M == 1
    seqs = [Sequence(list(p), sp) for p, sp in zip(PROMPTS, params)]
    for s in seqs:
        eng.pipeline.sched.add(s)
    done = {s.seq_id: s for s in eng.pipeline.run_until_done()}
    return [done[s.seq_id].output for s in seqs]


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("field,bad", [
    ("repetition_penalty", 0.0), ("repetition_penalty", -1.0), ("presence_penalty", 2.5),
    ("presence_penalty", -2.01), ("frequency_penalty", 3.0), ("frequency_penalty", -2.5),
    ("min_p", -0.1), ("min_p", 1.01)])
def test_sampling_params_ranges(field, bad):
    with pytest.raises(ValueError, match=field):
        SamplingParams(**{field: bad})


def test_sampling_params_accept_the_range_ends():
    p = SamplingParams(repetition_penalty=0.01, presence_penalty=-2.0, frequency_penalty=2.0,
                       min_p=1.0)
    assert p.has_penalty
    assert not SamplingParams(min_p=0.5).has_penalty and not SamplingParams().has_penalty


def test_scheduler_refuses_penalties_without_slots_and_accepts_min_p():
    sch = Scheduler(1, 8, 64, lambda n: -(-n // 4), total_blocks=64)
    with pytest.raises(ValueError, match="penalty_slots"):
        sch.add(Sequence([1, 2, 3], SamplingParams(presence_penalty=0.5)))
    assert not sch.waiting
    sch.add(Sequence([1, 2, 3], SamplingParams(min_p=0.1)))
    p = sch.plan(0)
    assert p.min_p == [pytest.approx(0.1)] and p.pen_slot == [] and not p.penalised
    # a plan of plain requests carries none of the control lists
    sch2 = Scheduler(1, 8, 64, lambda n: -(-n // 4), total_blocks=64, penalty_slots=2)
    sch2.add(Sequence([1, 2, 3], SamplingParams()))
    p2 = sch2.plan(0)
    assert p2.min_p == [] and p2.pen_slot == [] and p2.pen_feed == []


# ------------------------------------------------------------------ slots
def test_two_slots_serve_four_penalised_requests():
    """At most two hold a slot at once, all finish; admission behind a blocked penalised request
    waits like it does behind a KV shortage (the head of the queue blocks the rest)."""
    eng = _engine(slots=2)
    sch = eng.pipeline.sched
    pen = SamplingParams(max_tokens=6, ignore_eos=True, repetition_penalty=1.3)
    plain = SamplingParams(max_tokens=6, ignore_eos=True)
    seqs = [Sequence(list(p), pen if i < 4 else plain) for i, p in enumerate(PROMPTS[:5])]
    for s in seqs:
        sch.add(s)
    plan = sch.plan(0)
    # two penalised admitted; the third blocks the queue, the plain request behind it included
    assert plan.seq_ids == [seqs[0].seq_id, seqs[1].seq_id]
    assert sorted(plan.pen_slot) == [0, 1] and not sch._free_slots
    assert [s.seq_id for s in sch.waiting] == [s.seq_id for s in seqs[2:]]
    eng2 = _engine(slots=2)
    seqs2 = [Sequence(list(p), pen if i < 4 else plain) for i, p in enumerate(PROMPTS[:5])]
    for s in seqs2:
        eng2.pipeline.sched.add(s)
    done = eng2.pipeline.run_until_done()
    assert len(done) == 5 and all(len(s.output) == 6 for s in done)
    s2 = eng2.pipeline.sched
    assert s2.max_slots_held == 2 and sorted(s2._free_slots) == [0, 1]
    assert all(s.pen_slot == -1 for s in done)


def test_feed_segments_split_prompt_and_outputs_and_reset_once():
    sch = Scheduler(1, 8, 8, lambda n: -(-n // 4), total_blocks=64, penalty_slots=1)
    s = Sequence([1, 2, 3, 4, 5], SamplingParams(max_tokens=9, ignore_eos=True,
                                                 frequency_penalty=1.0))
    s.output = [7, 8, 7]                      # as after a preemption: recompute prompt + outputs
    sch.add(s)
    p = sch.plan(0)                           # budget 8: the whole prompt and all three outputs
    assert p.pen_feed == [[0, 0, 1, 5], [0, 1, 0, 3]] and p.pen_feed_tokens == [1, 2, 3, 4, 5, 7, 8, 7]
    assert p.pen_slot == [0] and p.freq == [1.0] and p.rep == [1.0] and p.pres == [0.0]
    sch.on_tokens(0, [9])
    p = sch.plan(0)                           # decode: the sampler counted 9 itself
    assert p.pen_feed == [] and p.pen_slot == [0]
    # chunked: 6 tokens per step
    sch = Scheduler(1, 8, 6, lambda n: -(-n // 4), total_blocks=64, penalty_slots=1)
    s = Sequence([1, 2, 3, 4, 5], SamplingParams(max_tokens=9, ignore_eos=True,
                                                 presence_penalty=1.0))
    s.output = [7, 8, 7]
    sch.add(s)
    p = sch.plan(0)
    assert p.pen_feed == [[0, 0, 1, 5], [0, 1, 0, 1]] and p.pen_feed_tokens == [1, 2, 3, 4, 5, 7]
    assert p.sample_rows == []
    sch.on_tokens(0, [])
    p = sch.plan(0)
    assert p.pen_feed == [[0, 1, 0, 2]] and p.pen_feed_tokens == [8, 7] and p.sample_rows == [0]


# ------------------------------------------------------------------ wire
def test_step_plan_wire_round_trip():
    p = StepPlan(step=4, mb=1, seq_ids=[7, 9], q_lens=[3, 1], sample_rows=[0, 1],
                 temperature=[0.0, 0.8], top_k=[0, 5], top_p=[1.0, 0.9], seeds=[1, 2],
                 sample_pos=[3, 11], min_p=[0.0, 0.1], pen_slot=[2, -1], rep=[1.2, 1.0],
                 pres=[0.5, 0.0], freq=[0.0, 0.0], pen_feed=[[2, 0, 1, 3]],
                 pen_feed_tokens=[5, 6, 5])
    import msgpack
    d = msgpack.unpackb(msgpack.packb(p.to_wire()))
    q = StepPlan.from_wire(d)
    for k in ("min_p", "pen_slot", "rep", "pres", "freq", "pen_feed", "pen_feed_tokens",
              "seq_ids", "sample_pos"):
        assert getattr(q, k) == getattr(p, k), k
    assert q.penalised and q.uses_min_p
    old = {k: v for k, v in p.to_wire().items()
           if k not in ("min_p", "pen_slot", "rep", "pres", "freq", "pen_feed", "pen_feed_tokens")}
    o = StepPlan.from_wire(old)
    assert o.pen_slot == [] and o.min_p == [] and o.pen_feed == [] and not o.penalised \
        and not o.uses_min_p


# ------------------------------------------------------------------ head placement
def test_penalised_plans_keep_the_head_on_the_last_rank():
    pol = HeadPolicy(4, True, 16)
    base = dict(mb=0, seq_ids=[1, 2], q_lens=[1, 1], sample_rows=[0, 1])
    for step in range(8):
        assert pol.rank_for(StepPlan(step=step, **base)) == step % 4
        assert pol.rank_for(StepPlan(step=step, min_p=[0.1, 0.0], **base)) == step % 4
        assert pol.rank_for(StepPlan(step=step, pen_slot=[-1, 3], rep=[1, 1.2], pres=[0, 0],
                                     freq=[0, 0], **base)) == 3
        assert pol.rank_for(StepPlan(step=step, pen_slot=[-1, -1], **base)) == step % 4


# ------------------------------------------------------------------ execution-mode equality
_REF = {}


def _reference(temperature):
    if temperature not in _REF:
        _REF[temperature] = _run(_engine(), _mixed_params(temperature), lookahead=False)
    return _REF[temperature]


@pytest.mark.parametrize("temperature", [0.0, 0.8], ids=["greedy", "seeded"])
@pytest.mark.parametrize("pp,mbs,lookahead", [(1, 0, True), (1, 3, False), (2, 0, False),
                                              (2, 1, True), (2, 3, False)])
def test_tokens_do_not_depend_on_the_execution_mode(temperature, pp, mbs, lookahead):
    """In-process pipelines: PP = 1 / 2, 1 / 3 micro-batches, lookahead on / off."""
    eng = _engine(pp=pp, mbs=mbs)
    out = _run(eng, _mixed_params(temperature), lookahead=lookahead)
    assert out == _reference(temperature)
    assert sorted(eng.pipeline.sched._free_slots) == list(range(8))


def test_penalties_and_min_p_change_the_tokens():
    """The reference runs are not the unpenalised runs in disguise: requests without a control
    keep their tokens, and some request with one gets other tokens."""
    for temperature in (0.0, 0.8):
        plain = [SamplingParams(max_tokens=MAX_TOKENS, temperature=temperature, seed=100 + i,
                                ignore_eos=True) for i in range(len(PROMPTS))]
        base = _run(_engine(), plain, lookahead=False)
        ref = _reference(temperature)
        params = _mixed_params(temperature)
        for i, p in enumerate(params):
            if not p.has_penalty and p.min_p == 0:
                assert ref[i] == base[i]
        assert any(ref[i] != base[i] for i, p in enumerate(params) if p.has_penalty), temperature


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _mp_worker(rank, world, port, q, temperature, rotation):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DLI_HEAD_ROTATION=rotation)
    import torch.distributed as dist
    from distributed_llm_inference.runtime.engine import init_pipeline_rank
    cfg = _cfg(pp=world)
    cfg.model = SPEC  # type: ignore[assignment]
    role, obj = init_pipeline_rank(cfg)
    if role == "driver":
        seqs = [Sequence(list(p), sp) for p, sp in zip(PROMPTS, _mixed_params(temperature))]
        for s in seqs:
            obj.sched.add(s)
        done = {s.seq_id: s for s in obj.run_until_done()}
        obj.stop()
        obj.close()
        q.put([done[s.seq_id].output for s in seqs])
    else:
        obj.run()
        obj.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("temperature,rotation", [(0.0, "1"), (0.8, "1"), (0.8, "0")],
                         ids=["greedy-rotating", "seeded-rotating", "seeded-pinned"])
def test_multiprocess_pipeline_equals_the_single_stage_engine(temperature, rotation):
    """PP = 2 over gloo (one process per stage), the LM head rotating (min-p only steps rotate,
    steps with a penalised row stay on the last stage) and pinned."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_mp_worker, args=(r, 2, port, q, temperature, rotation))
          for r in range(2)]
    for pr in ps:
        pr.start()
    got = q.get(timeout=240)
    for pr in ps:
        pr.join(60)
        assert pr.exitcode == 0
    assert got == _reference(temperature)


# ------------------------------------------------------------------ preemption
@pytest.mark.parametrize("temperature", [0.0, 0.8], ids=["greedy", "seeded"])
def test_preempted_penalised_sequences_resume_with_the_same_tokens(temperature):
    params = _mixed_params(temperature, max_tokens=40)
    ref = _run(_engine(), params)
    eng = _engine(num_blocks=10)
    out = _run(eng, params)
    assert eng.pipeline.sched.preemptions > 0
    assert out == ref


# ------------------------------------------------------------------ state
def test_slot_rows_hold_prompt_set_and_output_counts_at_release(monkeypatch):
    """Just before a finished penalised sequence gives its slot back, the slot's row equals its
    prompt set + Counter(outputs) - after preemptions too."""
    eng = _engine(num_blocks=10)
    table = eng.executors[-1].pen_table
    seen = []
    release = Scheduler._release_slot

    def spy(self, s):
        if s.pen_slot >= 0 and s.is_finished():
            seen.append((list(s.prompt), list(s.output), table[s.pen_slot].clone()))
        release(self, s)

    monkeypatch.setattr(Scheduler, "_release_slot", spy)
    eng.pipeline.lookahead = False     # (a lookahead step may have counted one more token)
    params = _mixed_params(0.8, max_tokens=40)
    _run(eng, params)
    assert eng.pipeline.sched.preemptions > 0
    assert len(seen) == sum(p.has_penalty for p in params)
    for prompt, output, row in seen:
        want = torch.zeros(SPEC.vocab_size, dtype=torch.int64)
        for t in set(prompt):
            want[t] += PROMPT_BIT
        for t, n in Counter(output).items():
            want[t] += n
        assert torch.equal(row.long(), want)


# ------------------------------------------------------------------ sanity
def test_penalties_reduce_repetition_in_a_greedy_run():
    def most_common(**kw):
        eng = _engine()
        out = eng.generate(PROMPTS[:4], SamplingParams(max_tokens=64, ignore_eos=True, **kw))
        return [max(Counter(s.output).values()) for s in out]
    plain = most_common()
    pen = most_common(repetition_penalty=2.0, frequency_penalty=2.0)
    assert all(b < a for a, b in zip(plain, pen)), (plain, pen)


def test_zero_slots_means_no_table():
    eng = _engine(slots=0)
    assert all(ex.pen_table is None for ex in eng.executors)
    with pytest.raises(ValueError, match="penalty_slots"):
        eng.generate(PROMPTS[:1], SamplingParams(max_tokens=2, presence_penalty=1.0))
    out = eng.generate(PROMPTS[:2], SamplingParams(max_tokens=4, temperature=0.7, seed=1,
                                                   min_p=0.2, ignore_eos=True))
    assert all(len(s.output) == 4 for s in out)
    assert _engine(slots=4, pp=2).executors[0].pen_table is None
