"""The MXFP4 weight-streaming MFMA kernel for 3-32 rows (KernelPolicy.fp4_small_m) without a GPU:
the policy field, Linear.fp4_small_ok, and the dispatch of Linear / LlamaMLP, whose CPU branch is
the oracle of the GPU kernel."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import KernelPolicy, ModelSpec
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.models.llama.modules import LlamaMLP
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16
SPEC = ModelSpec(name="t", vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=4,
                 num_heads=8, num_kv_heads=2, head_dim=32, rope_theta=10000.0,
                 max_position_embeddings=4096)


def test_policy_field():
    assert KernelPolicy().fp4_small_m == 0
    assert ops.FP4_SMALL_MAX_M == 32
    assert KernelPolicy().with_overrides("fp4_small_m=16").fp4_small_m == 16
    assert KernelPolicy().with_overrides("fp4_small_m=0").fp4_small_m == 0
    for ok in (3, 32):
        assert KernelPolicy(fp4_small_m=ok).fp4_small_m == ok
    for bad in (1, 2, 33, -1):
        with pytest.raises(ValueError):
            KernelPolicy(fp4_small_m=bad)
        with pytest.raises(ValueError):
            KernelPolicy().with_overrides(f"fp4_small_m={bad}")


def _fp4_linear(k, n, seed=0, bias=False):
    torch.manual_seed(seed)
    lin = Linear(k, n, bias=bias)
    lin.weight.data.copy_((torch.randn(n, k) * 0.05).to(BF))
    if bias:
        lin.bias.data.copy_((torch.randn(n) * 0.1).to(BF))
    lin.quantize_mxfp4()
    return lin


def test_fp4_small_ok_matrix():
    lin = _fp4_linear(512, 256)
    x = lambda m: torch.zeros(m, 512, dtype=BF)
    assert not lin.fp4_small_ok(x(3))                       # flag off
    with ops.kernel_policy(fp4_small_m=16):
        assert lin.fp4_small_ok(x(3)) and lin.fp4_small_ok(x(16))
        for m in (1, 2, 17):
            assert not lin.fp4_small_ok(x(m)), m
        assert not lin.fp4_small_ok(torch.zeros(1, 3, 512, dtype=BF))      # 3-D
        assert not lin.fp4_small_ok(torch.zeros(3, 512))                   # fp32 rows
        assert not lin.fp4_small_ok(None)
        dense = Linear(512, 256)
        assert not dense.fp4_small_ok(x(3))                                # bf16 weights
        assert not _fp4_linear(96, 256).fp4_small_ok(torch.zeros(3, 96, dtype=BF))   # K % 128
        assert not _fp4_linear(128, 24).fp4_small_ok(torch.zeros(3, 128, dtype=BF))  # N % 16


def _spy(monkeypatch, name):
    calls, real = [], getattr(ops, name)

    def wrapped(*a, **kw):
        calls.append(a[0].shape[0] if hasattr(a[0], "shape") else a[0].q.shape[0])
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, wrapped)
    return calls


def _gemv_arithmetic(x, lin, swiglu=False):
    """ops.skinny_gemm_fp4's CPU arithmetic, on any number of rows."""
    y = x.float() @ ref.dequantize_mxfp4(lin.weight_fp4, lin.weight_block_scale).float().t()
    if lin.bias is not None:
        y = y + lin.bias.float()
    return ops._swiglu_ref(y) if swiglu else y.to(BF)


@pytest.mark.parametrize("bias", [False, True])
def test_linear_dispatch_cpu(monkeypatch, bias):
    lin = _fp4_linear(512, 256, 1, bias=bias)
    small = _spy(monkeypatch, "small_gemm_fp4")
    torch.manual_seed(2)
    x = torch.randn(5, 512).to(BF)
    off = lin(x)
    assert small == []                                      # flag off: never
    with ops.kernel_policy(fp4_small_m=16):
        y = lin(x)
        assert small == [5]
        assert torch.equal(y, _gemv_arithmetic(x, lin))
        yd = lin(x, defer_reduce=True)
        assert isinstance(yd, torch.Tensor) and torch.equal(yd, y)
        lin(torch.randn(17, 512).to(BF))
        assert small == [5, 5]                              # 17 rows: not this kernel
    assert off.shape == y.shape


def test_small_before_fp4_mfma(monkeypatch):
    lin = _fp4_linear(512, 256, 3)
    small = _spy(monkeypatch, "small_gemm_fp4")
    tile = _spy(monkeypatch, "gemm_fp4_mx")
    with ops.kernel_policy(fp4_small_m=8, fp4_mfma=True):
        lin(torch.randn(8, 512).to(BF))
        assert small == [8] and tile == []
        lin(torch.randn(9, 512).to(BF))
        assert small == [8] and tile == [9]


def _fp4_mlp(seed=4):
    torch.manual_seed(seed)
    mlp = LlamaMLP(SPEC)
    for lin in (mlp.gate_up_proj, mlp.down_proj):
        lin.weight.data.copy_((torch.randn(lin.out_features, lin.in_features) * 0.05).to(BF))
        lin.quantize_mxfp4()
    mlp.set_fused_swiglu(True)
    assert mlp.fused_swiglu
    return mlp


def test_mlp_dispatch_cpu(monkeypatch):
    mlp = _fp4_mlp()
    small = _spy(monkeypatch, "small_gemm_fp4")
    tile = _spy(monkeypatch, "gemm_fp4_mx")
    torch.manual_seed(5)
    x = torch.randn(6, SPEC.hidden_size).to(BF)
    mlp(x)
    assert small == []
    with ops.kernel_policy(fp4_small_m=8):
        y = mlp(x)
        assert small == [6, 6]                              # gate|up (SwiGLU epilogue), down
        h = _gemv_arithmetic(x, mlp.gate_up_proj, swiglu=True)
        assert h.shape == (6, SPEC.intermediate_size)
        assert torch.equal(y, _gemv_arithmetic(h, mlp.down_proj))
    with ops.kernel_policy(fp4_small_m=8, fp4_mfma=True):
        del small[:]
        mlp(torch.randn(8, SPEC.hidden_size).to(BF))
        assert small == [8, 8] and tile == []
        mlp(torch.randn(9, SPEC.hidden_size).to(BF))
        assert small == [8, 8] and tile == [9, 9]
