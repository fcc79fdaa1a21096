"""The RoPE / KV-write oracle (tests/rope_oracle.py) checked on its own, without a GPU: its
expected images against literal loops, its bound against planted errors (each must be rejected),
and ops/reference.py -- the CPU fallback of ops.rope_cache -- held to the same contract as the
HIP kernels on every case, the fp8 edge values included."""
import pytest
import torch

import rope_oracle as ro
from distributed_llm_inference import ops

BF = ro.BF
CASES = ro.cases()


# -------------------------------------------------------------------------- the oracle itself
def test_case_list_covers_the_parameter_space():
    cs = CASES
    assert {(c.nh, c.nkv) for c in cs} == {(4, 2), (9, 3), (14, 2), (12, 12), (32, 8)}
    assert {c.D for c in cs} == {8, 32, 48, 64, 80, 96, 128, 256}
    assert {c.bs for c in cs} == {8, 16, 64, 256}
    assert {c.T for c in cs} == {1, 11} and {c.pad for c in cs} == {0, 4, 8}
    assert {c.path for c in cs} == {"v4", "v8", "v8norm"}
    assert {c.D for c in cs if c.norm} == {32, 64, 128, 256}
    for key in ("D", "bs", "pad", "path"):
        for val in {getattr(c, key) for c in cs}:
            assert {bool(c.window) for c in cs if getattr(c, key) == val} == {False, True}, (key, val)
    assert any(c.sliced for c in cs) and {c.parts for c in cs} >= {
        (1, "f32"), (1, "bf16"), (8, "f32"), (8, "bf16"), (3, "f32")}
    assert {c.k_scale for c in cs if c.family.startswith("fp8edge")} == {1.0, 0.5, 0.3}
    # a workgroup (8 heads) that starts past the first v head; q|k|v inside one workgroup that
    # is not the first; the q|k boundary inside a workgroup
    def wgs(c):
        return [(lo, min(lo + 8, c.nh + 2 * c.nkv)) for lo in range(0, c.nh + 2 * c.nkv, 8)]
    for path in ("v4", "v8"):
        mine = [c for c in cs if c.path == path]
        assert any(lo > c.nh + c.nkv for c in mine for lo, hi in wgs(c)), path
        assert any(0 < lo < c.nh and hi > c.nh + c.nkv for c in mine for lo, hi in wgs(c)), path
        assert any(lo < c.nh < hi for c in mine for lo, hi in wgs(c)), path


@pytest.mark.parametrize("bs,nb,T", [(8, 4, 11), (16, 3, 11), (64, 3, 11), (256, 3, 11), (64, 4, 1)])
def test_slots(bs, nb, T):
    s = ro.slots_for(ro.Case(4, 2, 8, bs, "coord", nblocks=nb, T=T)).tolist()
    w = [x for x in s if x >= 0]
    assert len(set(w)) == len(w) and all(x < nb * bs for x in w)
    if T == 11:
        assert s.count(-1) == 1 and s != sorted(s)
        assert {x % 8 for x in w} == set(range(8))
        assert {0, bs - 1, (nb - 1) * bs, nb * bs - 1} <= set(w)
        assert len({x // bs for x in w}) == min(nb, 3)
        assert bs == 8 or len({(x % bs) // 8 for x in w}) >= 2


def test_coord_codes_are_unique_and_finite():
    for normal in (False, True):
        x = ro.coord_codes(60000, normal)
        assert x.view(torch.int16).unique().numel() == 60000
        assert bool(torch.isfinite(x.float()).all())
        if normal:
            a = x.float().abs()
            assert float(a.min()) >= 2.0 ** -119 and float(a.max()) < 2.0 ** 121


@pytest.mark.parametrize("c", [ro._geo(6, "coord"), ro._geo(2, "coord1", window=64),
                               ro._geo(4, "table", window=ro.TABLE_WINDOW)],
                         ids=lambda c: c.ident())
def test_expected_images_by_literal_loops(c):
    inp = ro.inputs(c)
    e = ro.expected(c, inp)
    qkv, half, n_qk = inp["qkv"], c.D // 2, c.nh + c.nkv
    K = torch.full(ro.k_shape(c), ro.SENT, dtype=BF)
    V = torch.full(ro.v_shape(c), ro.SENT, dtype=BF)
    Q = torch.zeros(c.T, c.nh, c.D, dtype=BF)
    QS = torch.zeros(c.T, c.nh, c.D, dtype=BF)
    cs = inp["cos_sin"]
    for t in range(c.T):
        slot = int(inp["slots"][t])
        blk, off = slot // c.bs, slot % c.bs
        if c.family == "table":
            pos = int(inp["positions"][t])
            pc = min(max(pos, 0), ro.TABLE_MAX_POS - 1)
            ps = min(max(min(pos, c.window - 1), 0), ro.TABLE_MAX_POS - 1)
        for h in range(n_qk):
            for d in range(c.D):
                val = valsink = qkv[t, h * c.D + d]
                if c.family == "table":         # out[i] = cos[p, i], out[i + half] = sin[p, i]
                    val, valsink = cs[pc, d].to(BF), cs[ps, d].to(BF)
                if h < c.nh:
                    Q[t, h, d], QS[t, h, d] = val, valsink
                elif slot >= 0:
                    K[blk, h - c.nh, off, d] = val
        if slot >= 0:
            for kh in range(c.nkv):
                for d in range(c.D):
                    V[blk, kh, off // 8, d, off % 8] = qkv[t, (n_qk + kh) * c.D + d]
    bits = lambda x: x.to(BF).view(torch.int16)
    assert torch.equal(bits(e["q"]), bits(Q)) and torch.equal(bits(e["k"]), bits(K))
    assert torch.equal(bits(e["v"]), bits(V))
    if c.window:
        assert torch.equal(bits(e["qs"]), bits(QS))
    assert not bool(e["bq"].any()) and not bool(e["bk"].any())
    if c.family == "table":
        assert not torch.equal(bits(e["qs"]), bits(e["q"]))
        assert e["q"].unique().numel() >= 9 * c.D - 3 * c.D     # 7 distinct rows of the table


def test_fp8_bytes_by_hand():
    x = torch.tensor([447., 448, 463, 464, 480, 1e4, 3e38, float("inf"), -464, -float("inf"),
                      2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10, 0.0], dtype=BF)
    want = [0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0xFE, 0x01, 0x00, 0x01, 0x00]
    assert ro.fp8_bytes(x, 1.0).tolist() == want
    assert ro.fp8_bytes(x * 0.5, 0.5).tolist() == want
    assert bool(ro.is_nan_code(ro.fp8_bytes(torch.tensor([float("nan")], dtype=BF), 0.3)).all())
    # 0.3: the fp32 reciprocal, not a division
    y = torch.tensor([134.0], dtype=BF)
    inv = torch.tensor(1.0 / 0.3, dtype=torch.float64).float()
    assert ro.fp8_bytes(y, 0.3).tolist() == (y.float() * inv).to(ro.F8).view(torch.uint8).tolist()


# ---------------------------------------------------------------------------- the bound bites
PLANT = ro._geo(6, "randn", window=64)       # (12, 12), D = 96


def _planted(name):
    c, inp = PLANT, ro.inputs(PLANT)
    out = ro.ideal_out(c, inp)
    if name == "pos+1":             # one element rotated at pos + 1
        bad = ro.ideal_out(c, inp, "pos+1")
        out["q"][3, 5, 17] = bad["q"][3, 5, 17]
    elif name in ("sin_neg", "partner4"):
        out = ro.ideal_out(c, inp, name)
    elif name == "truncate":        # a truncating instead of rounding bf16 store
        e = ro.expected(c, inp)
        for n, k in (("q", "q"), ("qs", "qs"), ("k", "k")):
            bits = e[k].float().view(torch.int32) & ~0xFFFF
            out[n] = bits.view(torch.float32).to(BF)
    elif name == "v_lane":          # one V element in the neighbouring off % 8 lane
        slot = int(inp["slots"][0])
        blk, off = slot // c.bs, slot % c.bs
        v = out["v"]
        a, b = (blk, 7, off // 8, 31, off % 8), (blk, 7, off // 8, 31, (off % 8) ^ 1)
        v[a], v[b] = v[b].clone(), v[a].clone()
    return c, inp, out


def test_ideal_implementation_passes():
    c, inp, out = _planted(None)
    v = ro.evaluate(c, ro.expected(c, inp), out)
    assert v.ok and 0.9 < v.ratio <= 1.0, v.problems   # half an ulp is nearly the whole bound


@pytest.mark.parametrize("name", ["pos+1", "sin_neg", "partner4", "truncate", "v_lane"])
def test_planted_error_is_rejected(name):
    c, inp, out = _planted(name)
    v = ro.evaluate(c, ro.expected(c, inp), out)
    assert not v.ok and v.ratio > 1.0, name
    print(f"ROPE-RATIO planted {name} {v.ratio:.3g}")


def test_fp8_image_rejects_nan_codes_and_wrong_bytes():
    c = ro._geo(1, "fp8edge", k_scale=0.3, v_scale=0.3)
    inp = ro.inputs(c)
    kb = ro.ideal_out(c, inp)["k"]
    e = ro.expected(c, inp, k_bf16=kb)
    good = dict(q=e["q"].to(BF), qs=None, k=e["k8"].clone(), v=e["v8"].clone(), guards=[])
    assert ro.evaluate(c, e, good).ok
    big = (ro.fp8_bytes(kb, c.k_scale) == 0x7E) & (e["k8"] != ro.SENT8) & (kb.float().abs() > 200)
    assert int(big.sum()) > 10
    bad = dict(good, k=torch.where(big, torch.tensor(0x7F, dtype=torch.uint8), good["k"]))
    assert not ro.evaluate(c, e, bad).ok            # overflow to the NaN code
    bad = dict(good, v=good["v"] ^ (good["v"] == 0x01).to(torch.uint8))
    assert not ro.evaluate(c, e, bad).ok            # smallest subnormal flushed


# ------------------------------------------------------- ops/reference.py under the same cases
@pytest.mark.parametrize("c", CASES, ids=ro.ids(CASES))
def test_reference_meets_the_contract(c):
    res = ro.check_both(c, "cpu")
    for name, v in res.items():
        print(f"ROPE-RATIO cpu {c.path} {c.family} {name} {v.ratio:.4f}")
    for name, v in res.items():
        assert v.ok, f"{name}: " + "\n".join(v.problems[:8])
