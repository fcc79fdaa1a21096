"""``KernelPolicy.fp4_mfma`` on the CPU: the policy field, the ``Linear`` / ``LlamaMLP`` dispatch
(shape- and policy-based only, so the CPU arithmetic is the oracle of the GPU kernels) and the
composition of the path: MX-quantise the rows, multiply the two dequantised operands."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import KernelPolicy, ModelSpec
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.models.llama.modules import LlamaMLP
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16


def _lin(K, N, seed):
    g = torch.Generator().manual_seed(seed)
    lin = Linear(K, N)
    lin.weight.data.copy_((torch.randn(N, K, generator=g) * 0.05).to(BF))
    lin.quantize_mxfp4()
    return lin


def test_policy_field():
    assert KernelPolicy().fp4_mfma is False
    assert KernelPolicy().with_overrides("fp4_mfma=1").fp4_mfma is True
    assert KernelPolicy(fp4_mfma=True).with_overrides("fp4_mfma=0").fp4_mfma is False


def test_linear_dispatch_and_value():
    lin = _lin(512, 768, 1)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 512, generator=g).to(BF)
    off = lin(x)
    assert not lin.fp4_mfma_ok(x)
    with ops.kernel_policy(fp4_mfma=True):
        assert lin.fp4_mfma_ok(x)
        on = lin(x)
        want = ops.gemm_fp4_mx(ops.mx_quantize(x), lin.weight_fp4, lin.weight_block_scale)
        assert on.dtype == BF and torch.equal(on, want)
        assert not torch.equal(on, off)          # the fp8 activation rounding shows
        # the oracle itself: the fp32 product of the two dequantised operands
        ref_y = ops.mx_quantize(x).dequantize() @ ref.dequantize_mxfp4(
            lin.weight_fp4, lin.weight_block_scale).float().t()
        assert torch.equal(on, ref_y.to(BF))
        # 1-2 rows stay with the GEMV's rows; with the GEMV off they come here
        assert not lin.fp4_mfma_ok(x[:2]) and torch.equal(lin(x[:2]), off[:2])
        with ops.kernel_policy(gemv=False):
            assert lin.fp4_mfma_ok(x[:2]) and lin.fp4_mfma_ok(x[:1])
        assert not lin.fp4_mfma_ok(x.view(1, 5, 512))            # 2-D only
        with ops.kernel_policy(tile_gemm_max_m=4):
            assert not lin.fp4_mfma_ok(x)
        with ops.kernel_policy(tile_gemm_max_m=0):
            assert lin.fp4_mfma_ok(x)


@pytest.mark.parametrize("K,N", [(96, 768), (512, 384)])
def test_ineligible_shapes_keep_the_dequantise_path(K, N):
    lin = _lin(K, N, 3)
    x = torch.randn(5, K, generator=torch.Generator().manual_seed(4)).to(BF)
    off = lin(x)
    with ops.kernel_policy(fp4_mfma=True):
        assert not lin.fp4_mfma_ok(x)
        assert torch.equal(lin(x), off)


def test_bias_is_added_after_the_product():
    lin = Linear(256, 256, bias=True)
    g = torch.Generator().manual_seed(5)
    lin.weight.data.copy_((torch.randn(256, 256, generator=g) * 0.05).to(BF))
    lin.bias.data.copy_(torch.randn(256, generator=g).to(BF))
    lin.quantize_mxfp4()
    x = torch.randn(3, 256, generator=g).to(BF)
    with ops.kernel_policy(fp4_mfma=True):
        y = lin(x, defer_reduce=True)
        want = ops.gemm_fp4_mx(ops.mx_quantize(x), lin.weight_fp4, lin.weight_block_scale)
    assert torch.equal(y, want + lin.bias)


def test_mlp_fused_swiglu_equals_hand_composed():
    spec = ModelSpec(name="t", vocab_size=100, hidden_size=256, intermediate_size=512, num_layers=1,
                     num_heads=8, num_kv_heads=2, head_dim=32, rope_theta=10000.0,
                     max_position_embeddings=128)
    mlp = LlamaMLP(spec)
    g = torch.Generator().manual_seed(6)
    for lin in (mlp.gate_up_proj, mlp.down_proj):
        lin.weight.data.copy_((torch.randn(lin.out_features, lin.in_features, generator=g) * 0.05).to(BF))
        lin.quantize_mxfp4()
    mlp.set_fused_swiglu(True)
    assert mlp.fused_swiglu
    x = torch.randn(7, 256, generator=g).to(BF)
    gp, dp = mlp.gate_up_proj, mlp.down_proj
    off = mlp(x)
    with ops.kernel_policy(fp4_mfma=True):
        on = mlp(x)
    gu = ops.gemm_fp4_mx(ops.mx_quantize(x), gp.weight_fp4, gp.weight_block_scale)
    h = ops.swiglu_interleaved(gu)
    want = ops.gemm_fp4_mx(ops.mx_quantize(h), dp.weight_fp4, dp.weight_block_scale)
    assert on.shape == (7, 256) and torch.equal(on, want)
    assert not torch.equal(on, off)
    # the fused epilogue's CPU form is the same composition
    with ops.kernel_policy(fp4_mfma=True):
        assert torch.equal(ops.gemm_fp4_mx(ops.mx_quantize(x), gp.weight_fp4,
                                           gp.weight_block_scale, swiglu=True), h)


def test_splits_rule():
    # always >= 1, every split owns between 1 and FP4_MAX_KTILES k-tiles
    for M, N, K in [(3, 256, 128), (64, 8192, 28672), (512, 57344, 8192), (512, 8192, 28672),
                    (4096, 8192, 28672), (5, 256, 128 * 1000)]:
        s = ops.tile_gemm_splits_fp4(M, N, K)
        kt = K // 128
        kps = -(-kt // s)
        assert s >= 1 and (s - 1) * kps < kt and kps <= ops.FP4_MAX_KTILES, (M, N, K, s)
    assert ops.tile_gemm_splits_fp4(512, 8192, 8192) == ops.tile_gemm_splits_fp8(512, 8192, 8192)
