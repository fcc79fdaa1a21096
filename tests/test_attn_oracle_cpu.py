"""The attention oracle (tests/attn_oracle.py) checked on its own, without a GPU: the cache
builder against ref.rope_cache's writes, the oracle against ops/reference.py (the CPU fallback
of ops.attn_* and the yardstick of the older attention tests) on every input the GPU tests use,
and the probes' discriminating power: every visible target carries weight >= 1 - 2^-12, and
every single mutation of the oracle (a dropped or admitted key, sinks scored with q, a dropped
split) moves a probed output by more than 4x the bound the GPU tests accept."""
import pytest
import torch

import attn_oracle as ao
from distributed_llm_inference.ops import reference as ref

DECODE_PROBES = (ao.decode_full_specs() + ao.decode_head_specs() + ao.decode_one_step_specs()
                 + ao.decode_window_specs())
PREFILL_PROBES = [s for s, _ in ao.prefill_legacy_specs() + ao.prefill_m32_specs()]
DENSE = [s for _, s in ao.dense_specs()]
ONE_STEP_SAMPLE = tuple(range(0, 512, 37)) + tuple(range(3, 21))   # 32 rows, all seven lengths


def _ids(specs):
    return [s.ident() for s in specs]


def _sample(spec):
    return ONE_STEP_SAMPLE if spec.rows else None


def test_one_step_sample_has_every_length():
    c = ao.make_case(ao.decode_one_step_specs()[0])
    assert len(set(ONE_STEP_SAMPLE)) == 32
    assert {c.seq_lens[b] for b in ONE_STEP_SAMPLE} == set(ao.ONE_STEP_LENS)


def test_oracle_by_hand():
    """Two keys, one head: softmax weights and A by hand; an empty row gives zeros."""
    g = ao.Geo(1, 1, 32)
    K = torch.zeros(2, 1, 32, dtype=torch.float64)
    K[1, 0, 0] = 1.0
    V = torch.zeros(2, 1, 32, dtype=torch.float64)
    V[0, 0, 0], V[1, 0, 0] = -1.0, 3.0
    q = torch.zeros(2, 1, 32)
    q[:, 0, 0] = 2.0
    o, A, P = ao.attend(q, None, torch.tensor([0, 1]), K, V, g)
    w = 1.0 / (1.0 + torch.exp(torch.tensor(-2.0 * g.scale, dtype=torch.float64)))
    assert P[0, 0].tolist() == [1.0, 0.0] and o[0, 0, 0] == -1.0
    assert abs(P[1, 0, 1] - w) < 1e-15
    assert abs(o[1, 0, 0] - (3.0 * w - (1.0 - w))) < 1e-15
    assert abs(A[1, 0, 0] - (3.0 * w + (1.0 - w))) < 1e-15
    vis = torch.zeros(2, 2, dtype=torch.bool)
    o, A, _ = ao.attend(q, None, torch.tensor([0, 1]), K, V, g, vis=vis)
    assert not o.any() and not A.any()


def test_window_visibility_by_hand():
    g = ao.Geo(1, 1, 32, n_sink=2, sink_pad=32, ring=32, window=6)
    vis = ao.visible(torch.tensor([1, 5, 6, 9]), 11, g)
    assert vis[0].nonzero().flatten().tolist() == [0, 1]
    assert vis[1].nonzero().flatten().tolist() == [0, 1, 2, 3, 4, 5]
    assert vis[2].nonzero().flatten().tolist() == [0, 1, 3, 4, 5, 6]       # 2 just expired
    assert vis[3].nonzero().flatten().tolist() == [0, 1, 6, 7, 8, 9]


@pytest.mark.parametrize("fp8", [False, True])
def test_builder_layout_matches_rope_cache_writes(fp8):
    """Full cache: the builder's K and V^T layouts are what ref.rope_cache writes for the same
    tokens through a slot mapping built from the builder's block tables."""
    g = ao.Geo(4, 2, 32, fp8)
    gen = torch.Generator().manual_seed(5)
    lens = [1, 63, 64, 130]
    K_tok = [torch.randn(L, g.nkv, g.D, generator=gen) for L in lens]
    V_tok = [torch.randn(L, g.nkv, g.D, generator=gen) for L in lens]
    kc, vc, bt = ao.build_caches(g, K_tok, V_tok, lens, seed=3)
    assert bt.unique().numel() > 2 and not torch.equal(bt.flatten().sort().values, bt.flatten())
    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
    for b, L in enumerate(lens):
        a = torch.arange(L)
        slot_mapping = bt[b, a // g.bs].long() * g.bs + a % g.bs
        qkv = torch.cat([torch.zeros(L, g.nh * g.D), K_tok[b].reshape(L, -1),
                         V_tok[b].reshape(L, -1)], dim=1).to(ao.BF)
        ref.rope_cache(qkv, None, slot_mapping, None, g.nh, g.nkv, g.D, kc2, vc2,
                       k_scale=g.k_scale, v_scale=g.v_scale)
    assert torch.equal(kc.view(torch.uint8), kc2.view(torch.uint8))
    assert torch.equal(vc.view(torch.uint8), vc2.view(torch.uint8))


def test_builder_fill_and_ring_overwrite():
    """Window mode: later tokens overwrite earlier ones in the ring, sinks stay, and every slot
    not written (sink gap, unreached ring, spare and outside pages) holds the fill."""
    g = ao.Geo(2, 1, 32, n_sink=2, sink_pad=32, ring=32, window=20)
    K = [torch.arange(1, 41).float()[:, None, None].expand(40, 1, 32).contiguous(),
         torch.arange(1, 6).float()[:, None, None].expand(5, 1, 32).contiguous()]
    kc, vc, bt = ao.build_caches(g, K, K, [40, 5], poison=True, seed=1)
    for cache, get in ((kc, lambda pg, s: kc[pg, 0, s, 0]), (vc, lambda pg, s: vc[pg, 0, s // 8, 0, s % 8])):
        row = [float(get(int(bt[0, 0]), s)) for s in range(64)]
        assert row[:2] == [1.0, 2.0]
        assert all(abs(x) == ao.POISON for x in row[2:32])
        # ring slot o holds the newest token a with (a - 2) % 32 == o: tokens 8 .. 39
        assert row[32:] == [float(a + 1) for a in list(range(34, 40)) + list(range(8, 34))]
        row = [float(get(int(bt[1, 0]), s)) for s in range(64)]
        assert row[:2] == [1.0, 2.0] and row[32:35] == [3.0, 4.0, 5.0]
        assert all(abs(x) == ao.POISON for x in row[2:32] + row[35:])
        used = set(bt.flatten().tolist())
        for pg in range(cache.shape[0]):
            if pg not in used:
                assert (cache[pg].float().abs() == ao.POISON).all()
    z = ao.build_caches(g, K, K, [40, 5], poison=False, seed=1)[0]
    assert (z.float()[kc.float().abs() == ao.POISON] == 0).all()


@pytest.mark.parametrize("spec", DECODE_PROBES + PREFILL_PROBES,
                         ids=_ids(DECODE_PROBES + PREFILL_PROBES))
def test_probe_targets_carry_the_weight(spec):
    """Every visible-target probe puts >= 1 - 2^-12 of the fp64 softmax on its token, so the
    expected output is that token's V row; each case has visible and invisible probes."""
    c = ao.make_case(spec)
    o, A, wt = ao.oracle(spec, _sample(spec))
    done = ~torch.isnan(o[:, 0, 0])
    vis = (c.target >= 0) & done[:, None]
    assert vis.any() and ((c.target < 0) & done[:, None]).any()
    w = wt[vis]
    assert (w >= 1 - 2.0 ** -12).all(), f"min target weight {w.min().item()}"
    # ... and returns that token's V row to within the bound
    rows, heads = vis.nonzero(as_tuple=True)
    for b in set(c.seq_of[rows].tolist()):
        sel = c.seq_of[rows] == b
        r, h = rows[sel], heads[sel]
        want = c.Vr(b)[c.target[r, h], h // c.geo.G]
        assert ((o[r, h] - want).abs() <= ao.bound(o[r, h], A[r, h])).all()


def _reference(c, sample):
    """ops/reference.py on the case's caches, in fp32 (q is widened: its values are bf16)."""
    g = c.geo
    kc, vc, bt = c.caches(poison=False)
    lens = torch.tensor(c.seq_lens, dtype=torch.int32)
    q = c.q.float()
    qs = c.q_sink.float() if c.q_sink is not None else None
    if c.spec.kind == "decode":
        idx = torch.arange(len(c.seq_lens)) if sample is None else torch.tensor(sample)
        out = torch.full(q.shape, float("nan"))
        out[idx] = ref.attn_decode(q[idx], qs[idx] if qs is not None else None, kc, vc, bt[idx],
                                   lens[idx], g.scale, *g.window_args(), k_scale=g.k_scale,
                                   v_scale=g.v_scale)
        return out
    return ref.attn_prefill(q, qs, kc, vc, bt, lens, c.q_start(), g.scale, *g.window_args(),
                            k_scale=g.k_scale, v_scale=g.v_scale)


@pytest.mark.parametrize("spec", DECODE_PROBES + PREFILL_PROBES + DENSE,
                         ids=_ids(DECODE_PROBES + PREFILL_PROBES + DENSE))
def test_reference_matches_oracle(spec):
    """ref.attn_decode / ref.attn_prefill (slot space, fp32) against the token-space fp64
    oracle: 1e-5 relative to the magnitude of the summed terms A + |o| (fp32 products and
    sums of terms of that size; scores up to 45 lose ~45 * 2^-24 in the exponent)."""
    c = ao.make_case(spec)
    o, A, _ = ao.oracle(spec, _sample(spec))
    out = _reference(c, _sample(spec)).double()
    done = ~torch.isnan(o)
    assert torch.equal(done, ~torch.isnan(out))
    err = (out - o).abs()[done]
    tol = (1e-5 * (A + o.abs()) + 1e-7)[done]
    assert (err <= tol).all(), f"max err/tol {(err / tol).max().item():.3g}"


def _moved(spec, kind, **kw):
    """Largest move of a probed output under a mutation, in units of the GPU tests' bound."""
    o, A, _ = ao.oracle(spec, None)
    om, hit = ao.mutated(spec, kind, **kw)
    if not hit.any():
        return None
    return ((om - o).abs() / ao.bound(o, A)).max().item()


def _mutations(spec):
    g = spec.geo
    kinds = ["drop_newest", "drop_oldest", "admit_next"]
    if g.win:
        kinds += ["drop_oldest_rolling", "admit_expired"]
        if g.n_sink:
            kinds.append("sinks_with_q")
    return kinds


@pytest.mark.parametrize("spec", DECODE_PROBES + PREFILL_PROBES,
                         ids=_ids(DECODE_PROBES + PREFILL_PROBES))
def test_probes_have_teeth(spec):
    """Each single mutation of the oracle moves at least one probed output by more than 4x the
    bound the GPU tests accept: the probes cannot pass vacuously."""
    for kind in _mutations(spec):
        r = _moved(spec, kind)
        assert r is not None and r > 4.0, f"{kind}: moved {r} x bound"
    if spec.kind == "decode" and not spec.rows:
        splits = ao.WINDOW_SPLITS if spec.geo.win else ao.DECODE_SPLITS
        seen = 0
        for S in splits:
            for j in range(S if S > 1 else 0):
                r = _moved(spec, "drop_split", splits=S, split=j)
                if r is None:
                    continue      # a split with no keys at any length
                seen += 1
                assert r > 4.0, f"drop_split {j}/{S}: moved {r} x bound"
        assert seen >= 2
