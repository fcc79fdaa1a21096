"""The four sampling controls through the HTTP front end (a CPU engine behind EngineService, as
in tests/test_server_cpu.py): both endpoints pass them to the engine, out-of-range values and
penalties on a server without penalty slots answer 400."""
from collections import Counter

import pytest

from distributed_llm_inference.config import CacheConfig, ModelSpec, ServeConfig
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

SPEC = ModelSpec(name="t", vocab_size=300, hidden_size=128, intermediate_size=256, num_layers=4,
                 num_heads=4, num_kv_heads=2, head_dim=32, rope_theta=10000.0,
                 max_position_embeddings=4096)
PROMPT = list(range(3, 23))
CONTROLS = dict(repetition_penalty=1.5, presence_penalty=1.0, frequency_penalty=0.5, min_p=0.05)


def _engine(slots):
    cfg = EngineConfig(model="t", seed=3, cache=CacheConfig(num_blocks=128, block_size=32),
                       serve=ServeConfig(max_batch_size=8, max_num_batched_tokens=128,
                                         max_seq_len=256, use_graphs=False, penalty_slots=slots))
    return LLMEngine(SPEC, cfg=cfg)


@pytest.fixture(scope="module")
def app():
    from fastapi.testclient import TestClient
    from distributed_llm_inference.server.http import build_app
    from distributed_llm_inference.server.service import EngineService
    svc = EngineService(_engine(4).pipeline)
    yield TestClient(build_app(svc, model_name="t"))
    svc.shutdown()


@pytest.fixture(scope="module")
def app_no_slots():
    from fastapi.testclient import TestClient
    from distributed_llm_inference.server.http import build_app
    from distributed_llm_inference.server.service import EngineService
    svc = EngineService(_engine(0).pipeline)
    yield TestClient(build_app(svc, model_name="t"))
    svc.shutdown()


def _direct(**kw):
    p = SamplingParams(max_tokens=32, ignore_eos=True, **kw)
    return _engine(4).generate([PROMPT], p)[0].output


def _ids(r, endpoint):
    assert r.status_code == 200, r.text
    return r.json()["output_ids"] if endpoint == "/generate" else r.json()["choices"][0]["token_ids"]


@pytest.mark.parametrize("endpoint", ["/generate", "/v1/completions"])
def test_both_endpoints_pass_the_controls_through(app, endpoint):
    body = {"prompt_ids": PROMPT, "max_tokens": 32, "ignore_eos": True}
    plain = _ids(app.post(endpoint, json=body), endpoint)
    assert plain == _direct()
    # greedy with the three penalties: the tokens of the engine given the same parameters
    pen = {k: v for k, v in CONTROLS.items() if k != "min_p"}
    got = _ids(app.post(endpoint, json={**body, **pen}), endpoint)
    assert got == _direct(**pen) and got != plain
    # seeded sampling with all four
    samp = {"temperature": 0.8, "seed": 7, **CONTROLS}
    got = _ids(app.post(endpoint, json={**body, **samp}), endpoint)
    assert got == _direct(**samp)
    assert got != _ids(app.post(endpoint, json={**body, "temperature": 0.8, "seed": 7}), endpoint)
    # null fields (OpenAI clients send them) mean the defaults
    nulls = {k: None for k in CONTROLS}
    assert _ids(app.post(endpoint, json={**body, **nulls}), endpoint) == plain


def test_presence_penalty_breaks_a_greedy_loop(app):
    body = {"prompt_ids": PROMPT, "max_tokens": 48, "ignore_eos": True}
    a = _ids(app.post("/v1/completions", json=body), "/v1/completions")
    b = _ids(app.post("/v1/completions", json={**body, "presence_penalty": 2.0}),
             "/v1/completions")
    assert a != b
    assert max(Counter(b).values()) <= max(Counter(a).values())
    assert len(set(b)) > len(set(a))


@pytest.mark.parametrize("endpoint", ["/generate", "/v1/completions"])
@pytest.mark.parametrize("field,bad", [("repetition_penalty", 0), ("repetition_penalty", -1),
                                       ("presence_penalty", 2.5), ("frequency_penalty", -3),
                                       ("min_p", 1.5), ("min_p", -0.1),
                                       ("presence_penalty", "much")])
def test_out_of_range_values_answer_400(app, endpoint, field, bad):
    r = app.post(endpoint, json={"prompt_ids": [1, 2], "max_tokens": 2, field: bad})
    assert r.status_code == 400, r.text
    if not isinstance(bad, str):
        assert field in r.text


@pytest.mark.parametrize("endpoint", ["/generate", "/v1/completions"])
def test_penalties_without_slots_answer_400_and_min_p_runs(app_no_slots, endpoint):
    body = {"prompt_ids": [1, 2, 3], "max_tokens": 3, "ignore_eos": True}
    for field in ("repetition_penalty", "presence_penalty", "frequency_penalty"):
        r = app_no_slots.post(endpoint, json={**body, field: 1.5})
        assert r.status_code == 400 and "penalty-slots" in r.text, r.text
    r = app_no_slots.post(endpoint, json={**body, "temperature": 0.7, "min_p": 0.2})
    assert len(_ids(r, endpoint)) == 3
