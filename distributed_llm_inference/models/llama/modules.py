"""Llama decoder layer on the CDNA4 kernels.

Reference: ``OptimizedLlamaDecoderLayer`` / ``OptimizedLlamaInferenceAttention``
(/root/reference/distributed_llm_inference/models/llama/modules.py:23-184).  Same computation,
intended semantics (SURVEY B1/B2/B6/B7/B8/B9 fixed), MI355X-first data flow per layer:

    normed, residual = add_rmsnorm(h, residual)            # csrc/kernels/norm.hip
    qkv  = normed @ W_qkv^T                                 # ONE fused GEMM (hipBLASLt / fp8)
    q    = rope_cache(qkv) ; k,v -> paged KV cache          # csrc/kernels/rope_cache.hip
    o    = paged attention (decode split-K | prefill)       # csrc/kernels/attention.hip (MFMA)
    a    = o @ W_o^T
    normed, residual = add_rmsnorm(a, residual)
    h    = silu_mul(normed @ W_gate_up^T) @ W_down^T        # fused gate|up GEMM + activation.hip
                                                            # (decode: SwiGLU in the tile GEMM epilogue)

The residual stream is carried *separately* from the layer output, so each residual add is fused
into the following RMSNorm kernel (one HBM pass) instead of being a standalone elementwise op.
``pretraining_tp`` (reference modules.py:44-59, 107-110) is single-device weight slicing that is
mathematically identical to the unsliced projection; it is accepted and ignored.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ... import ops
from ...config import ModelSpec
from ..common import AttnMetadata, Linear


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    """``cat(-x2, x1)`` over the last dim (HF / reference ``rotate_half``)."""
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat((-x2, x1), dim=-1)


def apply_rotary_pos_emb(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                         unsqueeze_dim: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reference ``apply_rotary_pos_emb`` (modules.py:17-20) with the intended broadcasting (B2):
    ``cos``/``sin`` [B, T, D] are unsqueezed over the head axis of q [B, H, T, D] / k [B, KVH, T, D],
    and the rotation is computed in fp32.  The runtime path fuses RoPE into the KV-cache write
    kernel (csrc/kernels/rope_cache.hip); this helper serves library users and tests."""
    c = cos.unsqueeze(unsqueeze_dim).float()
    s = sin.unsqueeze(unsqueeze_dim).float()
    qf, kf = q.float(), k.float()
    return ((qf * c + rotate_half(qf) * s).to(q.dtype), (kf * c + rotate_half(kf) * s).to(k.dtype))


class RMSNorm(nn.Module):
    def __init__(self, hidden: int, eps: float, device=None, dtype=torch.bfloat16):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden, dtype=dtype, device=device), requires_grad=False)
        self.eps = eps

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None,
                residual_out: Optional[torch.Tensor] = None):
        return ops.rms_norm(x, self.weight, self.eps, residual=residual, residual_out=residual_out)


class LlamaAttention(nn.Module):
    def __init__(self, spec: ModelSpec, layer_idx: int, device=None, dtype=torch.bfloat16):
        super().__init__()
        self.layer_idx = layer_idx
        self.num_heads = spec.num_heads
        self.num_kv_heads = spec.num_kv_heads
        self.head_dim = spec.head_dim
        self.scale = spec.head_dim ** -0.5
        self.qkv_proj = Linear(spec.hidden_size, spec.qkv_size, bias=spec.attention_bias,
                               dtype=dtype, device=device)
        self.o_proj = Linear(spec.q_size, spec.hidden_size, bias=spec.has_o_proj_bias, dtype=dtype,
                             device=device)
        self.qkv_proj.role, self.o_proj.role = "qkv", "o"
        # Qwen3: every q / k head RMS-normalised over head_dim before RoPE, inside the RoPE /
        # KV-write kernel (csrc/kernels/rope_cache.hip); the weights stay bf16 under every
        # weight-quantisation mode
        self.qk_norm = spec.qk_norm
        if spec.qk_norm:
            self.q_norm = RMSNorm(spec.head_dim, spec.rms_norm_eps, device, dtype)
            self.k_norm = RMSNorm(spec.head_dim, spec.rms_norm_eps, device, dtype)

    def forward(self, normed: Optional[torch.Tensor], meta: AttnMetadata, k_cache: torch.Tensor,
                v_cache: torch.Tensor, cos_sin: torch.Tensor, x_q=None, defer_reduce: bool = False,
                norm: Optional[ops.RowNorm] = None):
        """``norm``: ``normed`` is the UN-normalised row and the QKV GEMV applies the input
        RMSNorm itself (1-2 decode rows, LlamaDecoderLayer._forward_gemv)."""
        q = None
        if norm is not None:
            # 1-2 rows: RMSNorm -> QKV -> RoPE / KV write in one GEMV launch when it applies.
            # Not with q/k norms: a wave of that epilogue holds two elements of a head, so the
            # GEMV (input RMSNorm still fused) is followed by the RoPE kernel, one launch more
            if not self.qk_norm:
                q = self.qkv_proj.gemv_qkv_rope(normed, meta, k_cache, v_cache, cos_sin,
                                                self.num_heads, self.num_kv_heads, self.head_dim,
                                                norm=norm)
            q_sink = None
            if q is None:
                qkv = self.qkv_proj.gemv(normed, norm=norm)
                if qkv is None:
                    raise RuntimeError("fused-norm QKV: the GEMV does not take this product")
        else:
            # split-K partials of the QKV GEMM are summed inside the RoPE / KV-write kernel
            qkv = self.qkv_proj(normed, x_q, defer_reduce=True)
        if q is None:
            qk = (dict(q_norm=self.q_norm.weight, k_norm=self.k_norm.weight,
                       norm_eps=self.q_norm.eps) if self.qk_norm else {})
            q, q_sink = ops.rope_cache(qkv, meta.positions, meta.slot_mapping, cos_sin,
                                       self.num_heads, self.num_kv_heads, self.head_dim, k_cache,
                                       v_cache, window=meta.window, want_sink=meta.want_sink,
                                       k_scale=meta.k_scale, v_scale=meta.v_scale, **qk)
        T = q.shape[0]
        if meta.custom_mask is not None:
            # reference-API custom 4-D additive mask (reference model.py:115-119, modules.py:92-94):
            # the prefill kernel's masked variant (any T, full cache) adds it before the online
            # softmax in place of the causal mask
            o = ops.attn_prefill(q, None, k_cache, v_cache, meta.block_tables, meta.seq_lens,
                                 meta.q_start, meta.max_q, self.scale, k_scale=meta.k_scale,
                                 v_scale=meta.v_scale, mask=meta.custom_mask)
        elif meta.is_decode:
            op = self.o_proj
            mx = (op.is_fp8 and op.bias is None and ops.policy().fp8_mx
                  and ops.attn_decode_mx_ok(self.head_dim, meta.num_splits)
                  and not op.fp8_small_rows(T))   # those rows stay bf16 for ops.small_gemm_fp8
            if mx and q.is_cuda:
                sp = ops.tile_gemm_splits_fp8(T, op.out_features, op.in_features)
                mx = bool(sp) and ops.mx_tileable(op.in_features, sp)
            if mx:
                # fp8 O projection: the attention epilogue quantises its output itself (one e8m0
                # scale per head row), consumed by the block-scaled MFMA -- no bf16 [T, nh*D]
                # store and no per-row quantisation pass
                o = ops.attn_decode(q, q_sink, k_cache, v_cache, meta.block_tables, meta.seq_lens,
                                    self.scale, meta.n_sink, meta.sink_pad, meta.ring, meta.window,
                                    num_splits=meta.num_splits, workspace=meta.workspace,
                                    k_scale=meta.k_scale, v_scale=meta.v_scale, mx_out=True)
                return op(None, x_q=o, defer_reduce=defer_reduce)
            o = ops.attn_decode(q, q_sink, k_cache, v_cache, meta.block_tables, meta.seq_lens,
                                self.scale, meta.n_sink, meta.sink_pad, meta.ring, meta.window,
                                num_splits=meta.num_splits, workspace=meta.workspace,
                                k_scale=meta.k_scale, v_scale=meta.v_scale)
        else:
            o = ops.attn_prefill(q, q_sink, k_cache, v_cache, meta.block_tables, meta.seq_lens,
                                 meta.q_start, meta.max_q, self.scale, meta.n_sink, meta.sink_pad,
                                 meta.ring, meta.window, k_scale=meta.k_scale,
                                 v_scale=meta.v_scale, tile_map=meta.tile_map)
        o = o.view(T, self.num_heads * self.head_dim)
        return self.o_proj(o, defer_reduce=defer_reduce)


class LlamaMLP(nn.Module):
    def __init__(self, spec: ModelSpec, device=None, dtype=torch.bfloat16,
                 intermediate_size: Optional[int] = None):
        """``intermediate_size``: a width other than the spec's (Qwen2-MoE's shared expert)."""
        super().__init__()
        if spec.hidden_act != "silu":
            raise ValueError(f"unsupported Llama activation {spec.hidden_act!r}")
        inter = spec.intermediate_size if intermediate_size is None else int(intermediate_size)
        self.intermediate_size = inter
        self.gate_up_proj = Linear(spec.hidden_size, 2 * inter, bias=spec.mlp_bias,
                                   dtype=dtype, device=device)
        self.down_proj = Linear(inter, spec.hidden_size, bias=spec.mlp_bias,
                                dtype=dtype, device=device)
        self.gate_up_proj.role, self.down_proj.role = "gate_up", "down"
        # True once gate_up_proj.weight's rows are in ops.swiglu_interleave order, so the tile
        # GEMM's epilogue can apply SwiGLU itself (no [M, 2I] intermediate, no silu_mul launch)
        self.fused_swiglu = False

    def set_fused_swiglu(self, on: bool) -> None:
        """Permute gate_up_proj's rows in place to / from the fused-SwiGLU tile order (bf16
        weights, or fp8 weights + their per-channel scales when the fp8 tile path is on)."""
        w = self.gate_up_proj
        if on == self.fused_swiglu:
            return
        if w.bias is not None or w.out_features % 256:
            return
        perm = ops.swiglu_interleave if on else ops.swiglu_deinterleave
        with torch.no_grad():
            if w.is_int8:
                # LLM.int8: rows of the int8 weight and its per-channel scale, columns of the
                # transposed copy; the outlier columns are gathered from these per product
                w.weight_int8.copy_(perm(w.weight_int8))
                w.weight_scale.copy_(perm(w.weight_scale.reshape(-1, 1)).reshape(w.weight_scale.shape))
                if w.weight_int8_t is not None:
                    w.weight_int8_t.copy_(perm(w.weight_int8_t.t()).t())
            elif w.is_fp4:
                # per-row blocks along K: quantisation commutes with the row permutation
                w.weight_fp4.copy_(perm(w.weight_fp4))
                w.weight_block_scale.copy_(perm(w.weight_block_scale))
            elif w.is_fp8:
                # per-output-channel quantisation commutes with the row permutation
                w.weight_fp8.copy_(perm(w.weight_fp8.view(torch.uint8)).view(w.weight_fp8.dtype))
                w.weight_scale.copy_(perm(w.weight_scale.reshape(-1, 1)).reshape(w.weight_scale.shape))
            else:
                w.weight.data.copy_(perm(w.weight.data))
        self.fused_swiglu = on

    def forward(self, normed: Optional[torch.Tensor], x_q=None, defer_reduce: bool = False,
                norm: Optional[ops.RowNorm] = None):
        gp = self.gate_up_proj
        if norm is not None:   # un-normalised rows: the gate|up GEMV applies the RMSNorm itself
            h = gp.gemv(normed, swiglu=True, norm=norm)
            if h is None:
                raise RuntimeError("fused-norm gate|up: the GEMV does not take this product")
            return self.down_proj(h, defer_reduce=defer_reduce)
        if self.fused_swiglu and ops.policy().gemv:
            # 1-2 decode rows: SwiGLU in the weight-streaming GEMV's epilogue (any weight dtype)
            h = gp.gemv_swiglu(normed, x_q)
            if h is not None:
                return self.down_proj(h, defer_reduce=defer_reduce)
        if self.fused_swiglu and gp.is_int8:
            # SwiGLU in the int8 tile GEMM's epilogue, after the fused bf16 outlier product
            h = ops.llm_int8_linear(normed, gp.weight_int8, gp.weight_scale, gp.int8_threshold,
                                    wq_t=gp.weight_int8_t, swiglu=True)
            return self.down_proj(h, defer_reduce=defer_reduce)
        if (self.fused_swiglu and gp.bias is None and x_q is None
                and gp.fp8_small_ok(normed)):
            # fp8, 3 to KernelPolicy.fp8_small_m bf16 rows: the weight-streaming MFMA kernel with
            # SwiGLU in its epilogue, no row quantisation; down_proj dispatches itself
            h = ops.small_gemm_fp8(normed, gp.weight_fp8, gp.weight_scale, swiglu=True)
            return self.down_proj(h, defer_reduce=defer_reduce)
        if self.fused_swiglu and gp.is_fp8:
            xq, xs = x_q if x_q is not None else ops.quant_rowwise(normed)
            if xq.is_cuda and ops.tile_gemm_splits_fp8(xq.shape[0], gp.out_features,
                                                        gp.in_features):
                dp = self.down_proj
                dsp = ops.tile_gemm_splits_fp8(xq.shape[0], dp.out_features, dp.in_features)
                g4 = ops.policy().fp8_on_gemm4("gate_up")
                if (ops.policy().fp8_mx and dsp and dp.bias is None
                        and ops.mx_tileable(dp.in_features, dsp)):
                    # SwiGLU output quantised in the epilogue with per-(row, 128-column) e8m0
                    # scales, consumed by the down projection's block-scaled MFMA: no bf16 h,
                    # no per-row quantisation pass
                    h = ops.gemm_tile_fp8(xq, xs, gp.weight_fp8, gp.weight_scale, swiglu=True,
                                          mx_out=True, gemm4=g4)
                    return dp(None, x_q=h, defer_reduce=defer_reduce)
                # fp8 gate|up on the block-scaled tile kernel, SwiGLU in its epilogue (bf16 out;
                # down_proj quantises it: one [M, I] pass instead of silu_mul_quant's [M, 2I])
                h = ops.gemm_tile_fp8(xq, xs, gp.weight_fp8, gp.weight_scale, swiglu=True,
                                      gemm4=g4)
            else:
                h = ops.swiglu_interleaved(gp(None, (xq, xs)))
            return self.down_proj(h, defer_reduce=defer_reduce)
        if self.fused_swiglu and gp.bias is None and gp.fp4_small_ok(normed):
            # MXFP4, 3 to KernelPolicy.fp4_small_m rows: the weight-streaming MFMA kernel with
            # SwiGLU in its epilogue; down_proj dispatches itself
            h = ops.small_gemm_fp4(normed, gp.weight_fp4, gp.weight_block_scale, swiglu=True)
            return self.down_proj(h, defer_reduce=defer_reduce)
        if self.fused_swiglu and gp.fp4_mfma_ok(normed):
            # MXFP4 on the fp4 x fp8 MFMA tile GEMM (KernelPolicy.fp4_mfma), SwiGLU in its epilogue
            if gp.in_features // 128 <= ops.FP4_MAX_KTILES:
                h = ops.gemm_fp4_mx(ops.quant_mx(normed), gp.weight_fp4, gp.weight_block_scale,
                                    swiglu=True)
            else:   # K past the whole-K kernel's scale slot: split-K product, SwiGLU after it
                h = ops.swiglu_interleaved(gp(normed))
            return self.down_proj(h, defer_reduce=defer_reduce)
        if self.fused_swiglu:
            if gp.tile_splits(normed):
                h = ops.gemm_tile(normed, gp.dense_weight(), swiglu=True)
            else:
                h = ops.swiglu_interleaved(gp(normed))
            return self.down_proj(h, defer_reduce=defer_reduce)
        gu = gp(normed, x_q)
        if x_q is None and self.down_proj.fp8_small_rows(gu.shape[0]) and gu.dim() == 2:
            # fp8 down projection on ops.small_gemm_fp8 (KernelPolicy.fp8_small_m): bf16 h
            return self.down_proj(ops.silu_mul(gu), defer_reduce=defer_reduce)
        if self.down_proj.is_fp8:  # SwiGLU fused with the fp8 quantisation of down_proj's input
            if not gu.is_cuda and ops.policy().fp8_mx and self.down_proj.bias is None:
                # CPU reference of the GPU tile path: h handed over in MX form (per-(row,
                # 128-column) e8m0 scales), as the fused SwiGLU epilogue quantises it
                return self.down_proj(None, x_q=ops.mx_quantize(ops.silu_mul(gu)),
                                      defer_reduce=defer_reduce)
            return self.down_proj(None, ops.silu_mul_quant(gu), defer_reduce=defer_reduce)
        return self.down_proj(ops.silu_mul(gu), defer_reduce=defer_reduce)


class MoEMLP(nn.Module):
    """Sparse mixture-of-experts MLP (Qwen3-MoE, Mixtral, Qwen2-MoE; HF
    ``Qwen3MoeSparseMoeBlock``): a bf16 router ``gate`` (H -> E), and per token the ``top_k`` most probable of E SwiGLU experts,
    weighted by their (optionally renormalised) router probabilities.

        logits = gate(x)                                   # Linear.forward, bf16
        route  = ops.moe_route(logits, k, renorm)          # csrc/kernels/moe.hip
        h      = swiglu(x[token] . w_gate_up[e]^T)         # grouped GEMM, rows sorted by expert
        y      = h . w_down[e]^T                           # grouped GEMM, rows back in pair order
        out[t] = bf16(sum_slot w[t, slot] * y[t k + slot]) # fp32, slot order, one rounding

    ``w_gate_up [E, 2I, H]`` holds every expert's rows in ``ops.swiglu_interleave`` order, always
    (``set_fused_swiglu`` leaves them alone); ``w_down [E, H, I]``.  Expert weights are bf16, or after
    :meth:`quantize_experts_fp8` e4m3 with one fp32 scale per weight row (``w_gate_up_scale
    [E, 2I]``, ``w_down_scale [E, H]``), or after :meth:`quantize_experts_mxfp4` MXFP4 nibbles
    ``[E, 2I, H / 2]`` / ``[E, H, I / 2]`` with one e8m0 scale per 32 input features
    (``w_gate_up_block_scale [E, 2I, H / 32]``, ``w_down_block_scale [E, H, I / 32]``); the router
    stays bf16 and the activations are never quantised.  The block returns a plain bf16 tensor:
    nothing is deferred to the next RMSNorm.

    Shared expert (Qwen2-MoE, HF ``Qwen2MoeSparseMoeBlock``; ``spec.shared_expert_intermediate_size
    > 0``): every token also runs ``shared_expert``, a dense :class:`LlamaMLP` of that width on
    the dense kernels, scaled by ``sigmoid(shared_expert_gate(x))``.  The gate's one row is stored
    as row E of ``gate.weight [E + 1, H]``, so the router product yields its logit as column E --
    one product per layer, no N = 1 launch:

        s      = shared_expert(x)                           # GEMV / tile GEMM, bf16 [T, H]
        logits = gate(x)                                    # [T, E + 1]
        route  = ops.moe_route(logits, k, renorm, E)        # shared_w[t] = bf16(sigmoid(logits[t, E]))
        out[t] = bf16(sum_slot w[t, slot] * y[t k + slot] + shared_w[t] * s[t])

    The shared expert stays bf16 under the expert-only quantisation modes (it is part of
    "everything but the routed experts")."""

    def __init__(self, spec: ModelSpec, device=None, dtype=torch.bfloat16):
        super().__init__()
        if spec.hidden_act != "silu":
            raise ValueError(f"unsupported MoE activation {spec.hidden_act!r}")
        E, I, H = spec.num_experts, spec.moe_intermediate_size, spec.hidden_size
        self.num_experts, self.top_k = E, spec.num_experts_per_tok
        self.intermediate_size = I
        self.norm_topk_prob = spec.norm_topk_prob
        # checkpoint key names: Mixtral's block_sparse_moe.experts.{e}.w1 / w3 / w2
        self.mixtral_keys = spec.model_type == "mixtral"
        self.shared_size = spec.shared_expert_intermediate_size
        # rows 0 .. E - 1: the router; with a shared expert, row E: its gate (shared_expert_gate)
        self.gate = Linear(H, E + (1 if self.shared_size else 0), bias=False, dtype=dtype,
                           device=device)
        self.gate.role = "router"
        if self.shared_size:
            self.shared_expert = LlamaMLP(spec, device, dtype, intermediate_size=self.shared_size)
        self.w_gate_up = nn.Parameter(torch.empty(E, 2 * I, H, dtype=dtype, device=device),
                                      requires_grad=False)
        self.w_down = nn.Parameter(torch.empty(E, H, I, dtype=dtype, device=device),
                                   requires_grad=False)
        self.register_buffer("w_gate_up_scale", None, persistent=False)
        self.register_buffer("w_down_scale", None, persistent=False)
        self.register_buffer("w_gate_up_block_scale", None, persistent=False)
        self.register_buffer("w_down_block_scale", None, persistent=False)
        self.fused_swiglu = True   # the experts' gate|up rows are always interleaved

    @property
    def is_fp8(self) -> bool:
        return self.w_gate_up_scale is not None

    @property
    def is_mxfp4(self) -> bool:
        return self.w_gate_up_block_scale is not None

    def experts(self, name: str) -> ops.ExpertWeights:
        """``w_gate_up`` or ``w_down`` with whichever of its scale buffers is set."""
        scale = getattr(self, name + "_scale")
        if scale is None:
            scale = getattr(self, name + "_block_scale")
        return ops.ExpertWeights(getattr(self, name), scale)

    def _quantize_experts(self, fmt: str) -> None:
        """Expert weights -> ``fmt`` (ops.ExpertWeights.quantize: one expert at a time), in place
        of the bf16 tensors, which are freed.  A scale belongs to a stored gate|up row (MXFP4: to
        32 input features of it), so the rows are quantised in their interleaved order."""
        have = "fp8" if self.is_fp8 else "mxfp4" if self.is_mxfp4 else "bf16"
        if have == fmt:
            return
        if have != "bf16":
            raise ValueError(f"quantize_experts_{fmt}: the experts are "
                             f"{'MXFP4' if have == 'mxfp4' else have} already")
        for name in ("w_gate_up", "w_down"):
            q = ops.ExpertWeights.quantize(getattr(self, name).data, fmt)
            setattr(self, name, nn.Parameter(q.w, requires_grad=False))
            setattr(self, name + ("_scale" if fmt == "fp8" else "_block_scale"), q.scale)

    def quantize_experts_fp8(self) -> None:
        """Expert weights -> fp8 e4m3 with per-row scales."""
        self._quantize_experts("fp8")

    def quantize_experts_mxfp4(self) -> None:
        """Expert weights -> MXFP4 nibbles with e8m0 block scales."""
        self._quantize_experts("mxfp4")

    def set_fused_swiglu(self, on: bool) -> None:
        """No-op for the routed experts: the grouped GEMM's only epilogue reads interleaved
        rows.  The shared expert is a dense MLP and follows the block's setting."""
        if self.shared_size:
            self.shared_expert.set_fused_swiglu(on)

    def forward(self, normed: torch.Tensor, x_q=None, defer_reduce: bool = False, norm=None):
        if x_q is not None or norm is not None:
            raise RuntimeError("MoEMLP takes normalised bf16 rows (the layer's generic body)")
        # the shared expert's output is a plain bf16 [T, H]: nothing deferred
        shared = self.shared_expert(normed) if self.shared_size else None
        return ops.moe_mlp(normed, self.gate(normed), self.experts("w_gate_up"),
                           self.experts("w_down"), self.top_k, self.norm_topk_prob,
                           num_experts=self.num_experts if self.shared_size else None,
                           shared=shared)

    # ------------------------------------------------------------------ weights
    def load_hf(self, g, sd: dict, dt: torch.dtype) -> None:
        """From a layer state dict ``sd`` (``g`` = its checked getter): the hub's per-expert keys
        (Qwen3-MoE ``mlp.experts.{e}.{gate,up,down}_proj.weight``, Mixtral
        ``block_sparse_moe.experts.{e}.{w1,w3,w2}.weight`` with w1 = gate, w3 = up, w2 = down), or
        the fused 3-D tensors ``experts.gate_up_proj [E, 2I, H]`` (gate half first) and
        ``experts.down_proj [E, H, I]`` under either prefix."""
        if self.is_fp8:
            raise RuntimeError("MoEMLP.load_hf on fp8 experts: load the bf16 weights first, then "
                               "quantize_experts_fp8()")
        if self.is_mxfp4:
            raise RuntimeError("MoEMLP.load_hf on MXFP4 experts: load the bf16 weights first, "
                               "then quantize_experts_mxfp4()")
        pre = next((p for p in ("mlp.", "block_sparse_moe.") if p + "gate.weight" in sd), None)
        if pre is None:
            g("block_sparse_moe.gate.weight" if self.mixtral_keys else "mlp.gate.weight")
        router = g(pre + "gate.weight")
        if tuple(router.shape) != (self.num_experts, self.gate.in_features):
            raise ValueError(f"{pre}gate.weight {tuple(router.shape)} is not "
                             f"[{self.num_experts}, {self.gate.in_features}]")
        self.gate.weight[:self.num_experts].copy_(router.to(dt))
        if self.shared_size:
            # Qwen2-MoE: mlp.shared_expert_gate.weight [1, H] becomes row E of the router, and
            # mlp.shared_expert.* the dense shared MLP
            self.gate.weight[self.num_experts:].copy_(
                g(pre + "shared_expert_gate.weight").reshape(1, -1).to(dt))
            sh = self.shared_expert
            gu = torch.cat([g(pre + "shared_expert.gate_proj.weight"),
                            g(pre + "shared_expert.up_proj.weight")], 0)
            if sh.fused_swiglu:
                gu = ops.swiglu_interleave(gu)
            sh.gate_up_proj.weight.copy_(gu.to(dt))
            sh.down_proj.weight.copy_(g(pre + "shared_expert.down_proj.weight").to(dt))
        if pre + "experts.gate_up_proj" in sd:
            gu, down = g(pre + "experts.gate_up_proj"), g(pre + "experts.down_proj")
            if gu.shape != self.w_gate_up.shape or down.shape != self.w_down.shape:
                raise ValueError(f"fused expert tensors {tuple(gu.shape)} / {tuple(down.shape)} "
                                 f"do not match {tuple(self.w_gate_up.shape)} / "
                                 f"{tuple(self.w_down.shape)}")
            for e in range(self.num_experts):
                self.w_gate_up[e].copy_(ops.swiglu_interleave(gu[e]).to(dt))
            self.w_down.copy_(down.to(dt))
            return
        names = ("w1", "w3", "w2") if pre + "experts.0.w1.weight" in sd else (
            "gate_proj", "up_proj", "down_proj")
        for e in range(self.num_experts):
            gate, up, down = (g(f"{pre}experts.{e}.{n}.weight") for n in names)
            self.w_gate_up[e].copy_(ops.swiglu_interleave(torch.cat([gate, up], 0)).to(dt))
            self.w_down[e].copy_(down.to(dt))

    def hf_dict(self) -> dict:
        """The hub's per-expert layout (inverse of :meth:`load_hf`); fp8 experts as their
        dequantised weights rounded to bf16, MXFP4 experts as their dequantised weights (exact)."""
        pre, names = (("block_sparse_moe.", ("w1", "w3", "w2")) if self.mixtral_keys else
                      ("mlp.", ("gate_proj", "up_proj", "down_proj")))
        sd = {pre + "gate.weight": self.gate.weight[:self.num_experts]}
        if self.shared_size:
            sh = self.shared_expert
            gu = sh.gate_up_proj.weight
            if sh.fused_swiglu:
                gu = ops.swiglu_deinterleave(gu)
            gate, up = gu.split([self.shared_size, self.shared_size], 0)
            sd.update({pre + "shared_expert_gate.weight": self.gate.weight[self.num_experts:],
                       pre + "shared_expert.gate_proj.weight": gate,
                       pre + "shared_expert.up_proj.weight": up,
                       pre + "shared_expert.down_proj.weight": sh.down_proj.weight})
        I = self.intermediate_size
        gate_up, down = self.experts("w_gate_up"), self.experts("w_down")
        for e in range(self.num_experts):
            gate, up = ops.swiglu_deinterleave(gate_up.dequantize(e)).split([I, I], 0)
            for n, w in zip(names, (gate, up, down.dequantize(e))):
                sd[f"{pre}experts.{e}.{n}.weight"] = w
        return sd


class LlamaDecoderLayer(nn.Module):
    """One decoder layer; ``layer_idx`` is the GLOBAL layer index (as in the reference)."""

    def __init__(self, spec: ModelSpec, layer_idx: int, device=None, dtype=torch.bfloat16):
        super().__init__()
        self.layer_idx = layer_idx
        self.hidden_size = spec.hidden_size
        self.self_attn = LlamaAttention(spec, layer_idx, device, dtype)
        # sparse MoE (Qwen3-MoE, Mixtral, Qwen2-MoE's sparse layers): the layer always takes the
        # generic body below.  A dense layer of a mixed stack is an ordinary dense layer, with
        # every dense fast path
        self.is_moe = spec.is_sparse_layer(layer_idx)
        self.mlp = MoEMLP(spec, device, dtype) if self.is_moe else LlamaMLP(spec, device, dtype)
        self.input_layernorm = RMSNorm(spec.hidden_size, spec.rms_norm_eps, device, dtype)
        self.post_attention_layernorm = RMSNorm(spec.hidden_size, spec.rms_norm_eps, device, dtype)

    def forward(self, hidden, residual: Optional[torch.Tensor], meta: AttnMetadata,
                k_cache: torch.Tensor, v_cache: torch.Tensor, cos_sin: torch.Tensor,
                defer_out: bool = False):
        """``defer_out``: the returned hidden state may be ``ops.SplitKPartials`` (the next
        layer's input RMSNorm reduces them); the O projection's partials always go straight
        into the post-attention RMSNorm."""
        if self._gemv_norms(hidden):
            return self._forward_gemv(hidden, residual, meta, k_cache, v_cache, cos_sin, defer_out)
        if self.self_attn.qkv_proj.is_fp8 and not self._fp8_small(hidden):
            return self._forward_fp8(hidden, residual, meta, k_cache, v_cache, cos_sin, defer_out)
        first = residual is None
        if first:
            # first layer of the stage: the input IS the residual; never modify it in place (it
            # may be a hipGraph's static input buffer that warmup / capture replays re-read)
            residual = hidden
            normed, _ = self.input_layernorm(hidden)
        else:
            normed, residual = self.input_layernorm(hidden, residual)
        attn = self.self_attn(normed, meta, k_cache, v_cache, cos_sin, defer_reduce=True)
        normed, residual = self.post_attention_layernorm(
            attn, residual, residual_out=torch.empty_like(residual) if first else None)
        return self.mlp(normed, defer_reduce=defer_out), residual

    def _gemv_norms(self, hidden) -> bool:
        """1-2 decode rows whose four projections all run on the weight-streaming GEMV: the two
        RMSNorms then run inside the QKV and gate|up GEMVs (``_forward_gemv``)."""
        if (self.is_moe or not isinstance(hidden, torch.Tensor) or not hidden.is_cuda
                or hidden.dim() != 2 or hidden.dtype != torch.bfloat16 or not hidden.is_contiguous()
                or not (ops.policy().gemv and ops.policy().gemv_norm)):
            return False
        M = hidden.shape[0]
        a, m = self.self_attn, self.mlp
        return (M * self.hidden_size * 2 <= 65536 and m.fused_swiglu
                and a.qkv_proj.gemv_ok(M) and a.o_proj.gemv_ok(M)
                and m.gate_up_proj.gemv_ok(M, swiglu=True) and m.down_proj.gemv_ok(M))

    def _fp8_small(self, hidden) -> bool:
        """3 to KernelPolicy.fp8_small_m bf16 rows whose four fp8 projections all run on the
        weight-streaming MFMA kernel (Linear.fp8_small_ok): the layer then takes the generic body
        (bf16 RMSNorms, no row quantiser) instead of ``_forward_fp8``.  Shapes, dtype and policy
        only, so the CPU takes the same branch."""
        if (self.is_moe or not ops.policy().fp8_small_m or not isinstance(hidden, torch.Tensor)
                or hidden.dim() != 2 or hidden.dtype != torch.bfloat16):
            return False
        a, m, M = self.self_attn, self.mlp, hidden.shape[0]
        return (a.qkv_proj.fp8_small_rows(M) and a.o_proj.fp8_small_rows(M)
                and m.gate_up_proj.fp8_small_rows(M) and m.down_proj.fp8_small_rows(M))

    def _forward_gemv(self, hidden, residual, meta, k_cache, v_cache, cos_sin, defer_out=False):
        """1-2 decode rows: input RMSNorm fused into the QKV GEMV, post-attention RMSNorm into the
        gate|up GEMV (which also applies SwiGLU): per layer QKV, RoPE/KV, attention, O, gate|up,
        down -- two launches fewer than the unfused order, same normalised rows (bit-identical
        norm arithmetic, gemv.hip).  The residual stream moves to fresh buffers (the GEMV writes
        it once while every workgroup still reads the old one)."""
        ln1, ln2 = self.input_layernorm, self.post_attention_layernorm
        if residual is None:   # first layer of the stage: the input IS the residual
            n1, res = ops.RowNorm(ln1.weight, ln1.eps), hidden
        else:
            res = torch.empty_like(residual)
            n1 = ops.RowNorm(ln1.weight, ln1.eps, residual, res)
        attn = self.self_attn(hidden, meta, k_cache, v_cache, cos_sin, norm=n1)
        res2 = torch.empty_like(res)
        n2 = ops.RowNorm(ln2.weight, ln2.eps, res, res2)
        return self.mlp(attn, norm=n2, defer_reduce=defer_out), res2

    def _forward_fp8(self, hidden, residual, meta, k_cache, v_cache, cos_sin, defer_out=False):
        """fp8 weights: every RMSNorm is fused with the fp8 quantisation of the GEMM input that
        follows it (quant.hip), so the bf16 normalised activation never touches HBM."""
        ln1, ln2 = self.input_layernorm, self.post_attention_layernorm
        first = residual is None
        if first:  # input is the residual; never modify it in place (graph static input)
            residual = hidden
            xq = ops.quant_rowwise(hidden, norm_w=ln1.weight, eps=ln1.eps)
        else:
            xq = ops.quant_rowwise(hidden, residual, ln1.weight, ln1.eps)
        # the O projection's split-K partials (tile path) are summed inside the quantiser
        attn = self.self_attn(None, meta, k_cache, v_cache, cos_sin, x_q=xq, defer_reduce=True)
        res_out = torch.empty_like(residual) if first else residual
        xq = ops.quant_rowwise(attn, residual, ln2.weight, ln2.eps, residual_out=res_out)
        # defer_out: the down projection's split-K partials go into the next layer's quantiser
        return self.mlp(None, x_q=xq, defer_reduce=defer_out), res_out

    # ------------------------------------------------------------------ weights
    def load_hf_state_dict(self, sd: dict) -> None:
        """Load a HF ``LlamaDecoderLayer`` state dict (keys relative to ``model.layers.{i}.``),
        fusing q|k|v and gate|up into the single GEMM weights."""
        def g(k):
            if k not in sd:
                raise KeyError(f"parameter {k} not found in state dict for layer {self.layer_idx}")
            return sd[k]
        dt = self.input_layernorm.weight.dtype
        with torch.no_grad():
            qkv = torch.cat([g("self_attn.q_proj.weight"), g("self_attn.k_proj.weight"),
                             g("self_attn.v_proj.weight")], 0)
            self.self_attn.qkv_proj.weight.copy_(qkv.to(dt))
            self.self_attn.o_proj.weight.copy_(g("self_attn.o_proj.weight").to(dt))
            if self.self_attn.qkv_proj.bias is not None:   # Llama attention_bias, Qwen2
                self.self_attn.qkv_proj.bias.copy_(torch.cat(
                    [g("self_attn.q_proj.bias"), g("self_attn.k_proj.bias"),
                     g("self_attn.v_proj.bias")], 0).to(dt))
            if self.self_attn.o_proj.bias is not None:     # Llama attention_bias (not Qwen2)
                self.self_attn.o_proj.bias.copy_(g("self_attn.o_proj.bias").to(dt))
            if self.self_attn.qk_norm:                     # Qwen3 per-head q/k RMSNorm
                self.self_attn.q_norm.weight.copy_(g("self_attn.q_norm.weight").to(dt))
                self.self_attn.k_norm.weight.copy_(g("self_attn.k_norm.weight").to(dt))
            if self.is_moe:
                self.mlp.load_hf(g, sd, dt)
            else:
                gu = torch.cat([g("mlp.gate_proj.weight"), g("mlp.up_proj.weight")], 0)
                if self.mlp.fused_swiglu:
                    gu = ops.swiglu_interleave(gu)
                self.mlp.gate_up_proj.weight.copy_(gu.to(dt))
                self.mlp.down_proj.weight.copy_(g("mlp.down_proj.weight").to(dt))
                if self.mlp.gate_up_proj.bias is not None:     # Llama mlp_bias
                    self.mlp.gate_up_proj.bias.copy_(torch.cat(
                        [g("mlp.gate_proj.bias"), g("mlp.up_proj.bias")], 0).to(dt))
                    self.mlp.down_proj.bias.copy_(g("mlp.down_proj.bias").to(dt))
            self.input_layernorm.weight.copy_(g("input_layernorm.weight").to(dt))
            self.post_attention_layernorm.weight.copy_(g("post_attention_layernorm.weight").to(dt))

    def hf_state_dict(self) -> dict:
        """Inverse of :meth:`load_hf_state_dict` (used to write checkpoints / test parity)."""
        a, m = self.self_attn, self.mlp
        q, k, v = a.qkv_proj.weight.split([a.num_heads * a.head_dim,
                                           a.num_kv_heads * a.head_dim,
                                           a.num_kv_heads * a.head_dim], 0)
        sd = {
            "self_attn.q_proj.weight": q, "self_attn.k_proj.weight": k,
            "self_attn.v_proj.weight": v, "self_attn.o_proj.weight": a.o_proj.weight,
            "input_layernorm.weight": self.input_layernorm.weight,
            "post_attention_layernorm.weight": self.post_attention_layernorm.weight,
        }
        if self.is_moe:
            sd.update(m.hf_dict())
        else:
            gu = m.gate_up_proj.weight
            if m.fused_swiglu:
                gu = ops.swiglu_deinterleave(gu)
            gate, up = gu.split([m.intermediate_size, m.intermediate_size], 0)
            sd.update({"mlp.gate_proj.weight": gate, "mlp.up_proj.weight": up,
                       "mlp.down_proj.weight": m.down_proj.weight})
        if a.qkv_proj.bias is not None:
            qb, kb, vb = a.qkv_proj.bias.split([a.num_heads * a.head_dim,
                                                a.num_kv_heads * a.head_dim,
                                                a.num_kv_heads * a.head_dim], 0)
            sd.update({"self_attn.q_proj.bias": qb, "self_attn.k_proj.bias": kb,
                       "self_attn.v_proj.bias": vb})
        if a.o_proj.bias is not None:
            sd["self_attn.o_proj.bias"] = a.o_proj.bias
        if a.qk_norm:
            sd.update({"self_attn.q_norm.weight": a.q_norm.weight,
                       "self_attn.k_norm.weight": a.k_norm.weight})
        if not self.is_moe and m.gate_up_proj.bias is not None:
            gb, ub = m.gate_up_proj.bias.split([m.intermediate_size, m.intermediate_size], 0)
            sd.update({"mlp.gate_proj.bias": gb, "mlp.up_proj.bias": ub,
                       "mlp.down_proj.bias": m.down_proj.bias})
        return sd
