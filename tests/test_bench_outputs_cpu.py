"""bench.py on one in-process stage (tiny Llama on the CPU): ``--dump-outputs`` writes the timed
steps' tokens, the same arguments give the same tokens, a plain run replicates the KV of one
step's worth of prefilled prompts, and ``--full`` prefills every prompt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, G, PROMPT, BUDGET = 3, 1, 8, 16, 64
N_SRC = BUDGET // PROMPT   # prompts one prefill step holds


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--model", "tiny-llama-8l", "--batch-per-mb", str(G),
           "--prompt-len", str(PROMPT), "--max-batched-tokens", str(BUDGET),
           "--dump-outputs", str(out_dir), *extra]
    env = dict(os.environ, OMP_NUM_THREADS="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(out_dir))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return (json.loads(lines[0]), np.load(os.path.join(out_dir, "tokens.npy")),
            np.load(os.path.join(out_dir, "tokens_timed.npy")))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return {"plain": _bench(tmp_path_factory.mktemp("plain")),
            "again": _bench(tmp_path_factory.mktemp("again")),
            "full": _bench(tmp_path_factory.mktemp("full"), "--full")}


def test_dump_outputs_files(runs):
    for res, last, timed in runs.values():
        assert last.dtype == np.float32 and timed.dtype == np.float32
        assert timed.shape == (STEPS, G) and last.shape == (G,)
        assert np.array_equal(last, timed[-1])
        assert np.all((timed >= 0) & (timed < 512) & (timed == np.floor(timed)))
        assert res["steps"] == STEPS and res["tokens_timed"] == STEPS * G
        assert res["ms_per_step"] > 0
        assert abs(res["value"] - res["tokens_timed"] / (res["ms_per_step"] * STEPS / 1e3)) \
            < 0.02 * res["value"]


def test_same_arguments_same_outputs(runs):
    assert np.array_equal(runs["plain"][2], runs["again"][2])


def test_plain_run_replicates_prefilled_kv(runs):
    res, _, timed = runs["plain"]
    assert res["prompts_prefilled"] == N_SRC
    # a sequence decodes exactly what the sequence whose prompt and KV blocks it copied decodes
    for j in range(N_SRC, G):
        assert np.array_equal(timed[:, j], timed[:, j % N_SRC]), (j, timed)


def _bench_module(monkeypatch):
    """bench.py as a module; the environment defaults it sets at import are undone after the test."""
    import importlib.util
    for k in ("HSA_ENABLE_IPC_MODE_LEGACY", "DLI_STAGE_TIMING", "DLI_HOP_CHECK", "DLI_TUNING_DIR"):
        monkeypatch.setenv(k, os.environ.get(k, ""))
        if not os.environ[k]:
            monkeypatch.delenv(k)
    monkeypatch.setattr(sys, "path", list(sys.path))
    spec = importlib.util.spec_from_file_location("_bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_adopt_books_like_admission(monkeypatch):
    bench = _bench_module(monkeypatch)
    from distributed_llm_inference.runtime.scheduler import Scheduler
    from distributed_llm_inference.runtime.sequence import SamplingParams, Sequence

    def sched():
        return Scheduler(1, 2, 64, lambda n: -(-n // 4), total_blocks=8, max_seq_len=32)

    params = SamplingParams(max_tokens=4, ignore_eos=True)
    a, b = sched(), sched()
    s = Sequence([5] * 8, params)
    a.add(s)
    p = a.plan(0)               # prefill step: 8 prompt tokens, samples the first token
    assert p.q_lens == [8]
    a.on_tokens(0, [7])
    t = Sequence([5] * 8, params)
    t.append_token(7, None)
    bench._adopt(b, t, 0)
    assert (b.reserved_blocks, t.num_computed, t.status) == (a.reserved_blocks, s.num_computed,
                                                             s.status)
    pa, pb = a.plan(0), b.plan(0)   # both decode the sampled token next
    assert pa.q_lens == pb.q_lens == [1] and pa.tokens == pb.tokens == [7]
    assert pa.sample_pos == pb.sample_pos
    with pytest.raises(ValueError):
        bench._adopt(b, Sequence([5] * 8, params), 0)        # no first token yet
    big = Sequence([5] * 24, params)
    big.append_token(1, None)
    with pytest.raises(MemoryError):
        bench._adopt(b, big, 0)                       # 7 blocks next to the 3 already reserved


def test_tuning_dir_leaves_an_unwritable_tree(monkeypatch, tmp_path):
    bench = _bench_module(monkeypatch)
    monkeypatch.delenv("DLI_TUNING_DIR", raising=False)
    # a source tree the user may write to keeps the engine's default (build/tuning in the tree)
    monkeypatch.setattr(bench, "REPO", str(tmp_path / "tree"))
    bench._tuning_dir()
    assert "DLI_TUNING_DIR" not in os.environ and (tmp_path / "tree" / "build" / "tuning").is_dir()
    # build/ cannot hold a directory (here: it is a file): the user's cache directory is used
    (tmp_path / "ro").mkdir()
    (tmp_path / "ro" / "build").write_text("")
    monkeypatch.setattr(bench, "REPO", str(tmp_path / "ro"))
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "cache"))
    bench._tuning_dir()
    d = os.environ["DLI_TUNING_DIR"]
    assert d.startswith(str(tmp_path / "cache")) and os.path.isdir(d)
    # an explicit setting is left alone
    monkeypatch.setenv("DLI_TUNING_DIR", "off")
    bench._tuning_dir()
    assert os.environ["DLI_TUNING_DIR"] == "off"


def test_full_run_prefills_every_prompt(runs):
    res, _, _ = runs["full"]
    assert res["prompts_prefilled"] == G
    assert res["prefill_s"] > 0
