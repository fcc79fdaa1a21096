"""The fused RoPE + paged-KV-write on the GPU -- rope_cache.hip's 4-element kernel, 16-byte kernel
and q/k-norm instantiation through ``ops.rope_cache``, and the GEMV's kEpRope epilogue through
``ops.skinny_gemm_qkv_rope`` -- against the fp64 oracle, derived bounds and bit-exact probes of
tests/rope_oracle.py: coordinate codes (which input element landed where), table codes (which
table row and column every output used, at every clamp), random data on a real table, and the
fp8 edge values (saturation at +-448, NaN kept, subnormals, scales that are no power of two).

Every case runs with bf16 caches (held to the bound, or to bit equality where the result is
exactly representable) and with fp8 caches (byte equality with the image made from that run's
K).  Outputs and caches are sentinel-filled and guarded on both sides.

Each test prints ``ROPE-RATIO gpu <kernel path> <family> <cache> <largest err / bound>`` (run
with -s; 0 for a bit-exact match, inf for a mismatch of bits).

Run on an MI355X: ``python -m pytest tests/test_rope_oracle_gpu.py -m gpu``.
"""
import pytest
import torch

import rope_oracle as ro
from distributed_llm_inference import ops

pytestmark = pytest.mark.gpu
BF = ro.BF
CASES = ro.cases()
GEMV_CASES = ro.gemv_cases()
GEMV_K = 64


def _report(c, path, res):
    for name, v in res.items():
        print(f"ROPE-RATIO gpu {path} {c.family} {name} {v.ratio:.4f}")
    for name, v in res.items():
        assert v.ok, f"{c.ident()} {name}: " + "\n".join(v.problems[:8])


@pytest.mark.parametrize("c", CASES, ids=ro.ids(CASES))
def test_rope_cache(gpu, c):
    _report(c, c.path, ro.check_both(c, gpu))


def _run_gemv(c, inp, dev, fp8):
    """x one-hot (x[m, m] = 1), W[:, m] = the qkv row of token m: the GEMV's output is the case's
    qkv exactly (fp32 accumulation of one non-zero product per row)."""
    M = c.T
    W = torch.zeros(c.width, GEMV_K, dtype=BF)
    W[:, :M] = inp["qkv"].t()
    x = torch.zeros(M, GEMV_K, dtype=BF)
    x[torch.arange(M), torch.arange(M)] = 1.0
    _, pos, slots, cs, _, _ = ro.device_inputs(c, inp, dev, False)
    cdt = torch.uint8 if fp8 else BF
    kbuf, k = ro._guarded(ro.k_shape(c), cdt, dev)
    vbuf, v = ro._guarded(ro.v_shape(c), cdt, dev)
    kc, vc = (k.view(ro.F8), v.view(ro.F8)) if fp8 else (k, v)
    q = ops.skinny_gemm_qkv_rope(x.to(dev), W.to(dev), None, None, pos, slots, cs, c.nh, c.nkv,
                                 c.D, kc, vc, k_scale=c.k_scale, v_scale=c.v_scale)
    torch.cuda.synchronize()
    guards = ro._guard_problems(dict(K=(kbuf, k.numel()), V=(vbuf, v.numel())))
    return dict(q=q.cpu(), qs=None, k=k.cpu(), v=v.cpu(), guards=guards)


@pytest.mark.parametrize("c", GEMV_CASES, ids=ro.ids(GEMV_CASES))
def test_gemv_rope_epilogue(gpu, c):
    inp = ro.inputs(c)
    out = _run_gemv(c, inp, gpu, False)
    res = dict(bf16=ro.evaluate(c, ro.expected(c, inp), out))
    out8 = _run_gemv(c, inp, gpu, True)
    res["fp8"] = ro.evaluate(c, ro.expected(c, inp, k_bf16=out["k"]), out8)
    _report(c, "gemv", res)


def test_fp8_overflow_bytes_observed(gpu):
    """What the KV writers store for |x| > 448, printed byte by byte (docs/kernels.md quotes it),
    and the contract: +-448 for finite values and +-inf, a NaN code for NaN only."""
    vals = torch.tensor([448.0, 464.0, 480.0, 1e4, 3e38, float("inf"), -464.0, -480.0, -3e38,
                         float("-inf"), float("nan")], dtype=BF)
    c = ro.Case(4, 2, 32, 16, "fp8edge", T=1)
    qkv = torch.ones(1, c.width, dtype=BF)
    n = vals.numel()
    qkv[0, 4 * 32:4 * 32 + n] = vals            # k head 0
    qkv[0, 6 * 32:6 * 32 + n] = vals            # v head 0
    inp = dict(qkv=qkv, slots=torch.tensor([5]), positions=None, cos_sin=None)
    out = ro.run_ops(c, inp, gpu, True)
    kb, vb = out["k"][0, 0, 5, :n].tolist(), out["v"][0, 0, 0, :n, 5].tolist()
    for x, a, b in zip(vals.tolist(), kb, vb):
        print(f"ROPE-FP8-BYTE x={x:g} K=0x{a:02X} V=0x{b:02X}")
    want = [0x7E] * 6 + [0xFE] * 4
    assert kb[:-1] == want and vb[:-1] == want, (kb, vb)
    assert kb[-1] & 0x7F == 0x7F and vb[-1] & 0x7F == 0x7F
