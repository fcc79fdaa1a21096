"""The fp8 weight-streaming MFMA kernel for 3-32 rows (KernelPolicy.fp8_small_m) without a GPU: the
policy field, Linear.fp8_small_ok, the dispatch of Linear / LlamaMLP / a whole stage, whose CPU
branch is the oracle of the GPU kernel, and the distance of the new route from bf16."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import KernelPolicy, ModelSpec
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.models.llama.modules import LlamaMLP

BF = torch.bfloat16
# tests/test_fp4_small_gpu.py's SPEC
SPEC = ModelSpec(name="t", vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=4,
                 num_heads=8, num_kv_heads=2, head_dim=32, rope_theta=10000.0,
                 max_position_embeddings=4096)


def test_policy_field():
    assert KernelPolicy().fp8_small_m == 0
    assert ops.FP8_SMALL_MAX_M == 32
    assert KernelPolicy().with_overrides("fp8_small_m=16").fp8_small_m == 16
    assert KernelPolicy().with_overrides("fp8_small_m=0").fp8_small_m == 0
    for ok in (3, 32):
        assert KernelPolicy(fp8_small_m=ok).fp8_small_m == ok
        assert KernelPolicy().with_overrides(f"fp8_small_m={ok}").fp8_small_m == ok
    for bad in (1, 2, 33, -1):
        with pytest.raises(ValueError):
            KernelPolicy(fp8_small_m=bad)
        with pytest.raises(ValueError):
            KernelPolicy().with_overrides(f"fp8_small_m={bad}")


def test_policy_field_from_env(monkeypatch):
    """DLI_KERNELS reaches the field (ops.set_policy applies the variable on top)."""
    prev = ops.policy()
    try:
        monkeypatch.setenv("DLI_KERNELS", "fp8_small_m=8")
        ops.set_policy(KernelPolicy())
        assert ops.policy().fp8_small_m == 8
    finally:
        monkeypatch.delenv("DLI_KERNELS")
        ops.set_policy(prev)


def _linear(k, n, seed=0, bias=False, mode="fp8"):
    torch.manual_seed(seed)
    lin = Linear(k, n, bias=bias)
    lin.weight.data.copy_((torch.randn(n, k) * 0.05).to(BF))
    if bias:
        lin.bias.data.copy_((torch.randn(n) * 0.1).to(BF))
    if mode == "fp8":
        lin.quantize_fp8()
    elif mode == "mxfp4":
        lin.quantize_mxfp4()
    elif mode == "int8":
        lin.quantize_int8()
    return lin


def test_fp8_small_ok_matrix():
    lin = _linear(512, 256)
    x = lambda m: torch.zeros(m, 512, dtype=BF)
    assert not lin.fp8_small_ok(x(3))                       # flag off
    with ops.kernel_policy(fp8_small_m=16):
        assert lin.fp8_small_ok(x(3)) and lin.fp8_small_ok(x(16))
        for m in (1, 2, 17):
            assert not lin.fp8_small_ok(x(m)), m
        assert not lin.fp8_small_ok(torch.zeros(1, 3, 512, dtype=BF))      # 3-D
        assert not lin.fp8_small_ok(torch.zeros(3, 512))                   # fp32 rows
        assert not lin.fp8_small_ok(None)
        for mode in ("bf16", "mxfp4", "int8"):                             # other weights
            assert not _linear(512, 256, mode=mode).fp8_small_ok(x(3)), mode
        assert not _linear(96, 256).fp8_small_ok(torch.zeros(3, 96, dtype=BF))    # K % 128
        assert not _linear(128, 24).fp8_small_ok(torch.zeros(3, 128, dtype=BF))   # N % 16
    with ops.kernel_policy(fp8_small_m=32):                 # the kernel's own limit
        assert lin.fp8_small_ok(x(32)) and not lin.fp8_small_ok(x(33))


def _spy(monkeypatch, name):
    calls, real = [], getattr(ops, name)

    def wrapped(*a, **kw):
        src = a[0].parts if isinstance(a[0], ops.SplitKPartials) else a[0]
        calls.append(src.shape[0])
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, wrapped)
    return calls


def _gemv_arithmetic(x, lin, swiglu=False):
    """ops.skinny_gemm_fp8's CPU arithmetic for bf16 rows (x_scale=None), on any number of rows."""
    y = x.float() @ (lin.weight_fp8.float() * lin.weight_scale.reshape(-1, 1)).t()
    if lin.bias is not None:
        y = y + lin.bias.float()
    return ops._swiglu_ref(y) if swiglu else y.to(BF)


@pytest.mark.parametrize("bias", [False, True])
def test_linear_dispatch_cpu(monkeypatch, bias):
    lin = _linear(512, 256, 1, bias=bias)
    torch.manual_seed(2)
    x = torch.randn(5, 512).to(BF)
    parent = lin(x)                                         # before any spy: the parent's route
    small = _spy(monkeypatch, "small_gemm_fp8")
    quant = _spy(monkeypatch, "quant_rowwise")
    off = lin(x)
    assert small == [] and quant == [5]                     # flag off: rows quantised, as before
    assert torch.equal(off, parent)
    del quant[:]
    with ops.kernel_policy(fp8_small_m=16):
        y = lin(x)
        assert small == [5] and quant == []
        assert torch.equal(y, _gemv_arithmetic(x, lin))
        assert torch.equal(y, ops.skinny_gemm_fp8(x, lin.weight_fp8, lin.weight_scale, None,
                                                  lin.bias))
        yd = lin(x, defer_reduce=True)
        assert isinstance(yd, torch.Tensor) and torch.equal(yd, y)
        lin(torch.randn(17, 512).to(BF))
        assert small == [5, 5] and quant == [17]            # 17 rows: not this kernel
        lin(None, x_q=ops._quant_ref(x.float(), x.shape))
        assert small == [5, 5]                              # rows already quantised: not either
    assert off.shape == y.shape


def _mlp(seed=4):
    torch.manual_seed(seed)
    mlp = LlamaMLP(SPEC)
    for lin in (mlp.gate_up_proj, mlp.down_proj):
        lin.weight.data.copy_((torch.randn(lin.out_features, lin.in_features) * 0.05).to(BF))
        lin.quantize_fp8()
    mlp.set_fused_swiglu(True)
    assert mlp.fused_swiglu
    return mlp


def test_mlp_dispatch_cpu(monkeypatch):
    mlp = _mlp()
    torch.manual_seed(5)
    x = torch.randn(6, SPEC.hidden_size).to(BF)
    parent = mlp(x)
    small = _spy(monkeypatch, "small_gemm_fp8")
    quant = _spy(monkeypatch, "quant_rowwise")
    off = mlp(x)
    assert small == [] and quant == [6, 6]
    assert torch.equal(off, parent)
    del quant[:]
    with ops.kernel_policy(fp8_small_m=8):
        y = mlp(x)
        assert small == [6, 6] and quant == []              # gate|up (SwiGLU epilogue), down
        h = _gemv_arithmetic(x, mlp.gate_up_proj, swiglu=True)
        assert h.shape == (6, SPEC.intermediate_size)
        assert torch.equal(y, _gemv_arithmetic(h, mlp.down_proj))
        mlp(torch.randn(9, SPEC.hidden_size).to(BF))
        assert small == [6, 6] and quant == [9, 9]
        # rows a fused producer already quantised: gate|up stays on the parent's route; its
        # bf16 h is a product like any other for down_proj
        mlp(None, x_q=ops._quant_ref(x.float(), x.shape))
        assert small == [6, 6, 6]


# ------------------------------------------------------------------------------------- stage
_STAGES = {}


def _stage(mode):
    """The 4-layer CPU stage of SPEC, bf16 or fp8, same weights; built once."""
    if mode not in _STAGES:
        st = CausalLMStage(SPEC, 0, 4).init_random(3)
        if mode == "fp8":
            st.quantize("fp8")
        _STAGES[mode] = st
    return _STAGES[mode]


def _stage_logits(stage, prompts):
    pool = stage.make_pool(128, block_size=64)
    sids = list(range(len(prompts)))
    for s, p in zip(sids, prompts):
        pool.manager.append(s, len(p))
    meta = pool.build_metadata(sids, [len(p) for p in prompts])
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=stage.device)
    return meta, stage(ids, meta, pool).float().cpu()


def test_stage_dispatch_cpu(monkeypatch):
    """5 sequences of one token each = 5 decode rows: with the flag on every layer makes 4 calls
    (QKV, O, gate|up, down) and the row quantiser is never called; 2 rows and 40 rows never
    reach the kernel."""
    st = _stage("fp8")
    small = _spy(monkeypatch, "small_gemm_fp8")
    quant = _spy(monkeypatch, "quant_rowwise")
    smq = _spy(monkeypatch, "silu_mul_quant")
    rows = lambda n: [[7 + i] for i in range(n)]
    meta, _ = _stage_logits(st, rows(5))
    assert meta.is_decode
    assert small == [] and len(quant) + len(smq) >= 3 * 4   # flag off: the parent's quantisers
    del quant[:], smq[:]
    with ops.kernel_policy(fp8_small_m=8):
        _stage_logits(st, rows(5))
        assert small == [5] * 16, small
        assert quant == [] and smq == []
        _stage_logits(st, rows(2))
        _stage_logits(st, rows(40))
        _stage_logits(st, [list(range(1, 10))])             # 9 prefill rows, limit 8
        assert small == [5] * 16
    with ops.kernel_policy(fp8_small_m=32):
        del small[:]
        _stage_logits(st, rows(40))
        assert small == []


def _rel(a, b):
    return ((a - b).norm() / a.norm()).item()


def test_stage_accuracy_vs_bf16():
    """Logits of 5 prefill rows (two prompts): the flag-on fp8 stage is no further from the bf16
    stage than the flag-off one -- the new route drops the per-row fp8 rounding of the activations
    and adds no rounding of its own (the weights are the same fp8 weights)."""
    prompts = [[1, 2, 3], [4, 5]]
    _, ref_logits = _stage_logits(_stage("bf16"), prompts)
    _, off = _stage_logits(_stage("fp8"), prompts)
    with ops.kernel_policy(fp8_small_m=8):
        _, on = _stage_logits(_stage("fp8"), prompts)
    assert ref_logits.shape[0] == 5
    r_on, r_off = _rel(ref_logits, on), _rel(ref_logits, off)
    print(f"fp8 stage vs bf16, 5 rows: flag on {r_on:.5f}, flag off {r_off:.5f}")
    assert r_on <= r_off, (r_on, r_off)
