"""Building blocks shared by the model families (Llama, GPT-2).

* :class:`Linear` — bf16 weights (hand-written tile GEMM / GEMV for decode, hipBLASLt otherwise),
  fp8-e4m3 weights with per-output-channel scales and per-token dynamic activation scales (the
  MI355X-native 8-bit default), or LLM.int8 weights with the reference's outlier ``threshold``
  (int8 MFMA + bf16 outlier columns) — the replacements of the reference's bitsandbytes
  ``Linear8bitLt`` (utils/model.py:93-113).
* :class:`AttnMetadata` — per-batch device metadata consumed by the attention / cache kernels
  (positions, slot mapping, block tables, sequence lengths, varlen offsets, window policy).  It
  replaces the reference's dense additive causal/padding mask (model.py:78-143): causality,
  padding and windows are all derived in-kernel from these small int tensors.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class _Mxfp4Scratch:
    """The bf16 buffers MXFP4 weights are dequantised into for the products the fp4 GEMV does not
    take.  One flat buffer per (device, stream), sized to the largest MXFP4 weight quantised so
    far; :meth:`reserve` (called by ``Linear.quantize_mxfp4``) is the only place that allocates,
    so the engine's KV-pool sizing sees the buffer and a forward -- in particular one under
    hipGraph capture -- only ever reads a pointer that already exists.  A forward on a stream
    that never reserved one (a graph warm-up / capture stream) borrows the device's buffer and,
    outside capture, orders itself behind the stream that used it last: reuse stays
    stream-ordered (a captured graph is ordered by its replay stream)."""

    def __init__(self):
        self.bufs = {}   # (device index, stream id) -> flat bf16 buffer
        self.last = {}   # buffer address -> stream that used it last

    def reserve(self, device: torch.device, numel: int) -> None:
        if device.type != "cuda":
            return
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, torch.cuda.current_stream(idx).cuda_stream)
        if key not in self.bufs or self.bufs[key].numel() < numel:
            self.bufs.pop(key, None)   # the smaller one goes back to the allocator first
            self.bufs[key] = torch.empty(numel, dtype=torch.bfloat16, device=device)

    def get(self, device: torch.device, numel: int) -> torch.Tensor:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        stream = torch.cuda.current_stream(idx)
        buf = self.bufs.get((idx, stream.cuda_stream))
        if buf is None:
            buf = next((b for (d, _), b in self.bufs.items() if d == idx), None)
        if buf is None or buf.numel() < numel:
            raise RuntimeError("MXFP4 dequantise scratch missing or too small: weights must be "
                               "converted with Linear.quantize_mxfp4 on their device")
        prev = self.last.get(buf.data_ptr())
        if prev is None or prev.cuda_stream != stream.cuda_stream:
            if prev is not None and not torch.cuda.is_current_stream_capturing():
                stream.wait_stream(prev)
            self.last[buf.data_ptr()] = stream
        return buf

    def nbytes(self, device=None) -> int:
        return sum(b.numel() * 2 for (d, _), b in self.bufs.items()
                   if device is None or torch.device("cuda", d) == torch.device(device))


MXFP4_SCRATCH = _Mxfp4Scratch()


class Linear(nn.Module):
    """``y = x W^T (+ b)`` with W stored [out, in]; optional fp8 / LLM.int8 / MXFP4 weights."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False,
                 dtype: torch.dtype = torch.bfloat16, device=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features, dtype=dtype,
                                               device=device), requires_grad=False)
        self.bias = (nn.Parameter(torch.zeros(out_features, dtype=dtype, device=device),
                                  requires_grad=False) if bias else None)
        self.register_buffer("weight_fp8", None, persistent=False)
        self.register_buffer("weight_scale", None, persistent=False)
        self.register_buffer("weight_int8", None, persistent=False)
        self.register_buffer("weight_int8_t", None, persistent=False)
        # MXFP4: e2m1 nibbles [out, in / 2] + e8m0 block exponents [out, in / 32]
        self.register_buffer("weight_fp4", None, persistent=False)
        self.register_buffer("weight_block_scale", None, persistent=False)
        self.int8_threshold = 0.0
        # which projection of its layer this is ("qkv" / "o" / "gate_up" / "down", set by the
        # model): KernelPolicy.fp8_gemm4 routes fp8 products per role
        self.role = ""

    @property
    def is_fp8(self) -> bool:
        return self.weight_fp8 is not None

    @property
    def is_int8(self) -> bool:
        return self.weight_int8 is not None

    @property
    def is_fp4(self) -> bool:
        return self.weight_fp4 is not None

    def quantize_mxfp4(self, keep_bf16: bool = False) -> None:
        """Quantise W to MXFP4 (OCP MX: 4-bit e2m1 elements, one e8m0 scale per 32 input
        features; ops.quantize_weight_mxfp4).  Frees the bf16 copy unless asked not to, and
        reserves the dequantise scratch of this device / stream (see :class:`_Mxfp4Scratch`)."""
        if self.in_features % ops.MXFP4_BLOCK:
            raise ValueError(f"MXFP4 needs in_features % {ops.MXFP4_BLOCK} == 0, "
                             f"got {self.in_features}")
        self.weight_fp4, self.weight_block_scale = ops.quantize_weight_mxfp4(self.weight.data)
        MXFP4_SCRATCH.reserve(self.weight_fp4.device, self.out_features * self.in_features)
        if not keep_bf16:
            self.weight = nn.Parameter(torch.empty(0, dtype=self.weight.dtype,
                                                   device=self.weight.device), requires_grad=False)

    def dense_weight(self) -> torch.Tensor:
        """The bf16 [out, in] weight the bf16 kernels read: the parameter itself, or for MXFP4
        weights their dequantisation (GPU: dequant_mxfp4_kernel into the persistent scratch,
        valid until the next MXFP4 product on this stream; CPU: the torch reference)."""
        if self.weight_fp4 is None:
            return self.weight
        if not self.weight_fp4.is_cuda:
            return ops.dequantize_mxfp4(self.weight_fp4, self.weight_block_scale)
        buf = MXFP4_SCRATCH.get(self.weight_fp4.device, self.out_features * self.in_features)
        return ops.dequantize_mxfp4(self.weight_fp4, self.weight_block_scale, out=buf)

    def quantize_int8(self, threshold: float = 6.0, keep_bf16: bool = False) -> None:
        """LLM.int8 weights (reference utils/model.py:93-113, bitsandbytes ``Linear8bitLt(threshold)``):
        per-channel absmax int8 + bf16 outlier-column decomposition at run time."""
        q, s = ops.quantize_weight_int8(self.weight.data)
        self.weight_int8, self.weight_scale = q, s
        # Optional (KernelPolicy.int8_transposed): a transposed [K, N] copy so the per-product outlier
        # weight-column gather reads contiguous rows (int8_outlier.hip gather_wt): 1.6 vs 2.9
        # ms/step on the 70B --int8 bench (+2.5 % tok/s), but it costs a second byte per weight,
        # i.e. the memory LLM.int8 exists to save (70B PP=1: KV blocks 9413 -> 6323, -33 %
        # concurrent sequences).  Off by default; opt in when KV capacity is not the limit.
        self.weight_int8_t = (q.t().contiguous() if q.is_cuda and ops.policy().int8_transposed
                              else None)
        self.int8_threshold = float(threshold)
        if not keep_bf16:
            self.weight = nn.Parameter(torch.empty(0, dtype=self.weight.dtype,
                                                   device=self.weight.device), requires_grad=False)

    def quantize_fp8(self, keep_bf16: bool = False) -> None:
        """Quantise W to fp8 e4m3 (per output channel).  Frees the bf16 copy unless asked not to."""
        q, s = ops.quantize_weight_fp8(self.weight.data)
        self.weight_fp8, self.weight_scale = q, s
        if not keep_bf16:
            self.weight = nn.Parameter(torch.empty(0, dtype=self.weight.dtype,
                                                   device=self.weight.device), requires_grad=False)

    def stream_weights(self):
        """(weight, per-row scale or None, bias or None) in the format the weight-streaming
        kernels read: bf16 [N, K], fp8 e4m3 [N, K] or int8 [N, K] with fp32 scales [N], or
        MXFP4 nibbles [N, K / 2] with e8m0 block exponents [N, K / 32] (uint8; ``is_fp4`` tells
        them apart)."""
        if self.weight_fp4 is not None:
            return self.weight_fp4, self.weight_block_scale, self.bias
        if self.weight_fp8 is not None:
            return self.weight_fp8, self.weight_scale.reshape(-1), self.bias
        if self.weight_int8 is not None:
            return self.weight_int8, self.weight_scale.reshape(-1), self.bias
        return self.weight, None, self.bias

    def tile_splits(self, x: torch.Tensor) -> int:
        """Split-K factor if ``gemm_tile`` takes this product on the GPU, else 0."""
        if (self.bias is not None or not x.is_cuda or x.dim() != 2 or x.dtype != torch.bfloat16
                or not x.is_contiguous() or self.weight_fp8 is not None
                or self.weight_int8 is not None):
            return 0
        return ops.tile_gemm_splits(x.shape[0], self.out_features, self.in_features)

    def fp4_mfma_ok(self, x: Optional[torch.Tensor]) -> bool:
        """Whether the product of ``x`` with these MXFP4 weights runs on the MFMA-native fp4 tile
        GEMM (``KernelPolicy.fp4_mfma``; ops.gemm_fp4_mx on MX-quantised rows) instead of the
        dequantise path.  Shapes and policy only, never the device: the CPU takes the same
        branch, so its torch arithmetic is the oracle of the GPU kernels."""
        if (self.weight_fp4 is None or not ops.policy().fp4_mfma or x is None or x.dim() != 2
                or self.in_features % 128 or self.out_features % 256):
            return False
        rows = x.shape[0]
        if rows < 1 or (rows <= ops.SKINNY_DISPATCH_M and ops.policy().gemv):
            return False   # 1-2 decode rows stay on the weight-streaming GEMV
        max_m = ops.policy().tile_gemm_max_m
        return max_m == 0 or rows <= max_m

    def fp4_small_ok(self, x: Optional[torch.Tensor]) -> bool:
        """Whether the product of ``x`` with these MXFP4 weights runs on the weight-streaming
        MFMA kernel for 3 to ``KernelPolicy.fp4_small_m`` bf16 rows (ops.small_gemm_fp4).  Like
        :meth:`fp4_mfma_ok`, shapes, dtype and policy only, never the device."""
        max_m = ops.policy().fp4_small_m
        if (self.weight_fp4 is None or not max_m or x is None or x.dim() != 2
                or x.dtype != torch.bfloat16 or self.in_features % 128
                or self.out_features % 16):
            return False
        return 3 <= x.shape[0] <= min(max_m, ops.FP4_SMALL_MAX_M)

    def fp8_small_ok(self, x: Optional[torch.Tensor]) -> bool:
        """Whether the product of ``x`` with these fp8 weights runs on the weight-streaming MFMA
        kernel for 3 to ``KernelPolicy.fp8_small_m`` bf16 rows (ops.small_gemm_fp8).  Like
        :meth:`fp4_small_ok`, shapes, dtype and policy only, never the device."""
        if x is None or x.dim() != 2 or x.dtype != torch.bfloat16:
            return False
        return self.fp8_small_rows(x.shape[0])

    def fp8_small_rows(self, rows: int) -> bool:
        """:meth:`fp8_small_ok` for ``rows`` 2-D bf16 rows that do not exist yet (a layer asking
        for the projections further down)."""
        max_m = ops.policy().fp8_small_m
        if (self.weight_fp8 is None or not max_m or self.in_features % 128
                or self.out_features % 16):
            return False
        return 3 <= rows <= min(max_m, ops.FP8_SMALL_MAX_M)

    def gemv_ok(self, rows: int, swiglu: bool = False, bf16_rows: bool = True) -> bool:
        """Whether :meth:`gemv` takes a product of ``rows`` GPU rows (bf16 rows, or with
        ``bf16_rows=False`` the fused quantiser's fp8 rows for fp8 weights)."""
        if not 1 <= rows <= ops.SKINNY_DISPATCH_M:
            return False
        if swiglu and (self.bias is not None or self.out_features % 32):
            return False
        if self.weight_fp4 is not None:
            return bf16_rows and ops.policy().gemv
        if self.weight_int8 is not None:
            return bf16_rows and self.in_features % 16 == 0 and ops.policy().gemv
        if self.weight_fp8 is not None:
            return self.in_features % 16 == 0 and ops.policy().gemv
        return bf16_rows and self.in_features % 8 == 0 and ops.policy().gemv

    def gemv(self, x: Optional[torch.Tensor], x_q: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
             swiglu: bool = False, norm: Optional["ops.RowNorm"] = None) -> Optional[torch.Tensor]:
        """The weight-streaming GEMV (1-2 decode rows on the GPU) of this Linear, with its
        optional fused epilogue (``swiglu``: this is a swiglu_interleave'd gate|up projection,
        silu(gate) * up is returned) and fused prologue (``norm``: x is the un-normalised row and
        the GEMV applies the input RMSNorm itself).  None when the GEMV does not take the
        product (more rows, CPU, shapes it does not cover) -- the caller falls back."""
        src = x if x is not None else (x_q[0] if x_q is not None else None)
        if (src is None or not src.is_cuda or src.dim() != 2 or isinstance(x_q, ops.MxFp8)
                or not self.gemv_ok(src.shape[0], swiglu, bf16_rows=x is not None)):
            return None
        if x is not None and (x.dtype != torch.bfloat16 or not x.is_contiguous()):
            return None
        if norm is not None and x is None:
            return None
        if self.weight_fp4 is not None:
            return ops.skinny_gemm_fp4(x, self.weight_fp4, self.weight_block_scale, self.bias,
                                       swiglu=swiglu, norm=norm)
        if self.weight_int8 is not None:
            return ops.skinny_gemm_int8(x, self.weight_int8, self.weight_scale, self.bias,
                                        swiglu=swiglu, norm=norm)
        if self.weight_fp8 is not None:
            if norm is not None or (x_q is None and x is not None):
                return ops.skinny_gemm_fp8(x, self.weight_fp8, self.weight_scale, None, self.bias,
                                           swiglu=swiglu, norm=norm)
            xq, xs = x_q if x_q is not None else ops.quant_rowwise(x)
            return ops.skinny_gemm_fp8(xq, self.weight_fp8, self.weight_scale, xs, self.bias,
                                       swiglu=swiglu)
        return ops.skinny_gemm(x, self.weight, self.bias, swiglu=swiglu, norm=norm)

    def gemv_qkv_rope(self, x: torch.Tensor, meta: "AttnMetadata", k_cache: torch.Tensor,
                      v_cache: torch.Tensor, cos_sin: torch.Tensor, nh: int, nkv: int,
                      head_dim: int, norm: Optional["ops.RowNorm"] = None
                      ) -> Optional[torch.Tensor]:
        """This Linear as the fused QKV projection of 1-2 decode rows with RoPE and the paged
        KV write in the GEMV's epilogue (see :func:`ops.skinny_gemm_qkv_rope`): returns q
        [M, nh, D], or None when that path does not apply (window mode's sink query, more rows,
        CPU) -- the caller then runs the GEMV and rope_cache separately."""
        if (x is None or not x.is_cuda or x.dim() != 2 or x.dtype != torch.bfloat16
                or not self.gemv_ok(x.shape[0]) or meta.want_sink or meta.custom_mask is not None
                or self.out_features != (nh + 2 * nkv) * head_dim):
            return None
        if self.weight_fp4 is not None:
            return ops.skinny_gemm_qkv_rope(x, self.weight_fp4, None, self.bias, meta.positions,
                                            meta.slot_mapping, cos_sin, nh, nkv, head_dim,
                                            k_cache, v_cache, meta.k_scale, meta.v_scale,
                                            norm=norm, block_scale=self.weight_block_scale)
        if self.weight_int8 is not None:
            w, ws = self.weight_int8, self.weight_scale
        elif self.weight_fp8 is not None:
            w, ws = self.weight_fp8, self.weight_scale
        else:
            w, ws = self.weight, None
        return ops.skinny_gemm_qkv_rope(x, w, ws, self.bias, meta.positions, meta.slot_mapping,
                                        cos_sin, nh, nkv, head_dim, k_cache, v_cache,
                                        meta.k_scale, meta.v_scale, norm=norm)

    def gemv_swiglu(self, x: Optional[torch.Tensor],
                    x_q: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                    ) -> Optional[torch.Tensor]:
        """silu(gate) * up straight from the GEMV's epilogue (see :meth:`gemv`)."""
        return self.gemv(x, x_q, swiglu=True)

    def forward(self, x: Optional[torch.Tensor],
                x_q: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                defer_reduce: bool = False):
        """``x_q`` = (fp8 rows, scales) already quantised by a fused producer kernel; then ``x`` may
        be None (fp8 weights only).  ``defer_reduce``: a split-K tile GEMM returns its fp32
        partials (``ops.SplitKPartials``) for an RMSNorm consumer to reduce."""
        if self.weight_int8 is not None:
            if (x.is_cuda and x.dim() == 2 and 1 <= x.shape[0] <= ops.SKINNY_DISPATCH_M
                    and x.dtype == torch.bfloat16 and self.in_features % 16 == 0
                    and ops.policy().gemv):
                # 1-2 row decode: int8 weight-streaming GEMV on the bf16 rows (the weights are
                # the whole cost; bf16 activations need no outlier decomposition)
                return ops.skinny_gemm_int8(x, self.weight_int8, self.weight_scale, self.bias)
            y = ops.llm_int8_linear(x.reshape(-1, self.in_features), self.weight_int8,
                                    self.weight_scale, self.int8_threshold,
                                    wq_t=self.weight_int8_t,
                                    defer_reduce=defer_reduce and self.bias is None)
            if isinstance(y, ops.SplitKPartials):   # the consumer reduces (rms_norm / rope_cache)
                return y
            y = y.reshape(*x.shape[:-1], self.out_features)
            return y + self.bias if self.bias is not None else y
        if self.fp4_small_ok(x):
            # MXFP4 weights, 3 to fp4_small_m rows: the weight streamed once and widened in
            # registers (csrc/kernels/gemm_fp4_small.hip); a plain bf16 tensor, nothing deferred
            return ops.small_gemm_fp4(x, self.weight_fp4, self.weight_block_scale, self.bias)
        if self.fp4_mfma_ok(x):
            # MXFP4 weights, more than 2 rows: rows quantised to MX fp8, then the fp4 x fp8
            # block-scaled MFMA tile GEMM (csrc/kernels/gemm_fp4.hip) -- no dequantised weight
            sp = ops.tile_gemm_splits_fp4(x.shape[0], self.out_features, self.in_features)
            y = ops.gemm_fp4_mx(ops.quant_mx(x), self.weight_fp4, self.weight_block_scale, sp,
                                defer_reduce=(defer_reduce and self.bias is None
                                              and sp <= ops.TILE_MAX_SPLITS))
            return y + self.bias if self.bias is not None else y
        if self.weight_fp8 is None:
            if (x.is_cuda and x.dim() == 2 and 1 <= x.shape[0] <= ops.SKINNY_DISPATCH_M
                    and x.dtype == torch.bfloat16 and x.is_contiguous()
                    and self.in_features % 8 == 0 and ops.policy().gemv):
                # 1-2 row decode batches: weight-streaming HIP kernel (csrc/kernels/gemv.hip)
                if self.weight_fp4 is not None:
                    return ops.skinny_gemm_fp4(x, self.weight_fp4, self.weight_block_scale,
                                               self.bias)
                return ops.skinny_gemm(x, self.weight, self.bias)
            # MXFP4: every other product dequantises into the persistent scratch and runs the
            # bf16 path below on it, unchanged
            w = self.dense_weight()
            sp = self.tile_splits(x)
            if sp:  # decode micro-batches: 256x256 MFMA tile kernel (csrc/kernels/gemm_tile.hip)
                return ops.gemm_tile(x, w, splits=sp, defer_reduce=defer_reduce)
            return F.linear(x, w, self.bias)
        if isinstance(x_q, ops.MxFp8):
            # MX activations from the fp8 SwiGLU epilogue: their e8m0 block scales go to the
            # block-scaled MFMA (gemm_tile.hip kFp8Mx); the MLP only hands these over when the
            # product is tileable (LlamaMLP.forward)
            sp = ops.tile_gemm_splits_fp8(x_q.q.shape[0], self.out_features, self.in_features)
            y = ops.gemm_tile_fp8_mx(x_q, self.weight_fp8, self.weight_scale, sp or 1,
                                     defer_reduce=defer_reduce and self.bias is None,
                                     gemm4=ops.policy().fp8_on_gemm4(self.role))
            if self.bias is not None:
                y = y + self.bias
            return y
        if x_q is None and self.fp8_small_ok(x):
            # fp8 weights, 3 to fp8_small_m bf16 rows: the weight streamed once and widened in
            # registers (csrc/kernels/gemm_fp8_small.hip), no row quantisation; a plain bf16
            # tensor, nothing deferred
            return ops.small_gemm_fp8(x, self.weight_fp8, self.weight_scale, self.bias)
        if (x_q is None and x is not None and x.is_cuda and x.dim() == 2
                and 1 <= x.shape[0] <= ops.SKINNY_DISPATCH_M and x.dtype == torch.bfloat16
                and self.in_features % 16 == 0 and ops.policy().gemv):
            # 1-2 row decode: fp8 weight-streaming GEMV on the bf16 rows (no quantisation pass;
            # KernelPolicy.gemv=False quantises the rows as a batch of >= 3 would --
            # docs/parity.md C11)
            return ops.skinny_gemm_fp8(x, self.weight_fp8, self.weight_scale, None, self.bias)
        if x_q is None:
            x_q = ops.quant_rowwise(x)
        xq, xs = x_q
        if (xq.is_cuda and xq.dim() == 2 and 1 <= xq.shape[0] <= ops.SKINNY_DISPATCH_M
                and self.in_features % 16 == 0 and ops.policy().gemv):
            # 1-2 row decode on the fused quantiser's fp8 rows: half the weight bytes of bf16
            # streamed by the GEMV kernel (hipBLASLt's fp8 GEMM at M = 1 streamed them slower
            # than the bf16 GEMV: Llama-3.1-70B batch-1 decode ran at the bf16 speed)
            return ops.skinny_gemm_fp8(xq, self.weight_fp8, self.weight_scale, xs, self.bias)
        if xq.is_cuda and self.bias is None and xq.dim() == 2:
            sp = ops.tile_gemm_splits_fp8(xq.shape[0], self.out_features, self.in_features)
            if sp:  # long-K fp8 products: block-scaled MFMA tile kernel (csrc/kernels/gemm_tile.hip)
                return ops.gemm_tile_fp8(xq, xs, self.weight_fp8, self.weight_scale, sp,
                                         defer_reduce=defer_reduce,
                                         gemm4=ops.policy().fp8_on_gemm4(self.role))
        if xq.is_cuda:
            y = torch._scaled_mm(xq, self.weight_fp8.t(), scale_a=xs, scale_b=self.weight_scale,
                                 out_dtype=torch.bfloat16)
        else:  # CPU: dequantised reference
            y = ((xq.float() * xs) @ (self.weight_fp8.float() * self.weight_scale.t()).t()
                 ).to(torch.bfloat16)
        if self.bias is not None:
            y = y + self.bias
        return y

    def extra_repr(self) -> str:
        return (f"in={self.in_features}, out={self.out_features}, bias={self.bias is not None}, "
                f"fp8={self.is_fp8}, int8={self.is_int8}, fp4={self.is_fp4}")


@dataclass
class AttnMetadata:
    """Device metadata of one forward batch (varlen: T tokens from B sequences)."""

    num_tokens: int
    num_seqs: int
    is_decode: bool                  # every sequence contributes exactly one new token
    positions: torch.Tensor          # [T] int32 rope positions
    slot_mapping: torch.Tensor       # [T] int64 physical cache slot (-1: don't write)
    block_tables: torch.Tensor       # [B, max_blocks] int32
    seq_lens: torch.Tensor           # [B] int32 (absolute length incl. new tokens)
    q_start: torch.Tensor            # [B+1] int32 token offsets
    max_q: int
    num_splits: int = 1
    workspace: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
    # attention-sink window policy (all zero for a full cache)
    n_sink: int = 0
    sink_pad: int = 0
    ring: int = 0
    window: int = 0
    # fp8 KV cache scales (stored = x / scale); 1.0 for bf16 caches
    k_scale: float = 1.0
    v_scale: float = 1.0
    # prefill work list [n_tiles, 2] (sequence, token tile) for the attention kernel, or None
    tile_map: Optional[torch.Tensor] = None
    # rows (token index) whose hidden state feeds the LM head, or None = all rows
    logits_rows: Optional[torch.Tensor] = None
    # caller-supplied pre-inverted additive 4-D mask [B, 1|nh, T, >= L] (LlamaBlock.forward's
    # reference-compatible path): replaces the in-kernel causal mask
    custom_mask: Optional[torch.Tensor] = None

    @property
    def windowed(self) -> bool:
        return self.ring > 0

    @property
    def want_sink(self) -> bool:
        return self.ring > 0 and self.n_sink > 0


def seeded_normal_(t: torch.Tensor, seed: int, std: float) -> torch.Tensor:
    """Deterministic N(0, std) init independent of device placement order (so a PP=8 split and a
    PP=1 model built from the same seed hold identical weights)."""
    g = torch.Generator(device=t.device)
    g.manual_seed(seed & 0x7FFFFFFFFFFFFFFF)
    with torch.no_grad():
        if t.dtype in (torch.float32, torch.float64):
            t.normal_(0.0, std, generator=g)
        else:
            # generate in chunks to bound the fp32 temporary
            flat = t.view(-1)
            step = 1 << 26
            for i in range(0, flat.numel(), step):
                chunk = flat[i:i + step]
                tmp = torch.empty(chunk.shape, dtype=torch.float32, device=t.device)
                tmp.normal_(0.0, std, generator=g)
                chunk.copy_(tmp)
    return t


def param_seed(base: int, layer_idx: int, name: str) -> int:
    h = 1469598103934665603
    for ch in f"{layer_idx}:{name}".encode():
        h = ((h ^ ch) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return (h ^ (base * 0x9E3779B97F4A7C15)) & 0x7FFFFFFFFFFFFFFF
