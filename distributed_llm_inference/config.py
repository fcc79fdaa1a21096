"""Model / stage / serving configuration.

The reference takes its model description straight from ``transformers.AutoConfig``
(``/root/reference/distributed_llm_inference/utils/model.py:83``) and reads a handful of
``LlamaConfig`` fields (``models/llama/model.py:19-23``, ``modules.py:44-45``).  This framework
owns its model code, so it parses the HF ``config.json`` itself into a small, frozen
:class:`ModelSpec` that every layer (kernels, KV pool sizing, pipeline planner) shares.  No
network access and no HF import are needed at runtime.

Unlike the reference (bug B9 in SURVEY.md) ``rms_norm_eps`` is honoured.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

# head sizes the fused q/k RMSNorm takes (csrc/kernels/rope_cache.hip: a head's head_dim / 16
# lanes must be a power of two)
QK_NORM_HEAD_DIMS = (32, 64, 128, 256)
# sparse MoE limits (csrc/kernels/moe.hip: a wave ranks <= 256 router logits, <= 8 slots per token)
MOE_MAX_EXPERTS = 256
MOE_MAX_TOPK = 8


@dataclass(frozen=True)
class ModelSpec:
    """Architecture description shared by every stage of a pipeline."""

    arch: str = "llama"  # "llama" | "gpt2"
    vocab_size: int = 128256
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    rms_norm_eps: float = 1e-5
    rope_theta: float = 500000.0
    rope_scaling: Optional[Tuple[Tuple[str, Any], ...]] = None  # frozen dict items
    max_position_embeddings: int = 8192
    tie_word_embeddings: bool = False
    pad_token_id: Optional[int] = None
    bos_token_id: Optional[int] = 128000
    eos_token_id: Optional[int] = 128001
    hidden_act: str = "silu"
    pretraining_tp: int = 1
    attention_bias: bool = False
    mlp_bias: bool = False
    name: str = "custom"
    # Llama-family variants: "llama" | "mistral" | "qwen2" | "qwen3" | "qwen3_moe" | "mixtral" |
    # "qwen2_moe" (the HF model_type)
    model_type: str = "llama"
    # bias on o_proj; None = same as attention_bias (Llama).  Qwen2 has q/k/v bias only.
    o_proj_bias: Optional[bool] = None
    # Mistral-style sliding-window attention length (None = full causal attention)
    sliding_window: Optional[int] = None
    # HF config.output_hidden_states: what LlamaBlock.forward does when its argument is None
    # (reference models/llama/model.py:35-37)
    output_hidden_states: bool = False
    # Qwen3: every q and k head is RMS-normalised over head_dim (learned weights q_norm / k_norm)
    # between the projection and RoPE
    qk_norm: bool = False
    # sparse mixture-of-experts MLP ("qwen3_moe", "mixtral", "qwen2_moe"): num_experts routed
    # experts of width moe_intermediate_size, num_experts_per_tok of them per token, the top-k
    # router weights optionally renormalised by their sum.  num_experts == 0: dense MLP
    num_experts: int = 0
    num_experts_per_tok: int = 0
    moe_intermediate_size: int = 0
    norm_topk_prob: bool = False
    # "qwen2_moe": every token of a sparse layer also goes through one dense SwiGLU expert of this
    # width, scaled by sigmoid(shared_expert_gate(x)) (a Linear H -> 1).  0: no shared expert
    shared_expert_intermediate_size: int = 0
    # "qwen2_moe": layer i is sparse when i is not in mlp_only_layers and (i + 1) %
    # decoder_sparse_step == 0 (is_sparse_layer); every other layer is a dense MLP of width
    # intermediate_size
    decoder_sparse_step: int = 1
    mlp_only_layers: Tuple[int, ...] = ()

    def __post_init__(self):
        if self.num_experts == 0:
            if self.shared_expert_intermediate_size:
                raise ValueError("shared_expert_intermediate_size needs a sparse MoE model "
                                 "(num_experts > 0)")
            return
        object.__setattr__(self, "mlp_only_layers",
                           tuple(sorted({int(i) for i in self.mlp_only_layers})))
        s = self.shared_expert_intermediate_size
        if s < 0 or s % 128:
            raise ValueError(f"shared_expert_intermediate_size={s}: a positive multiple of 128 "
                             "(or 0: no shared expert)")
        if any(not 0 <= i < self.num_layers for i in self.mlp_only_layers):
            raise ValueError(f"mlp_only_layers={list(self.mlp_only_layers)}: entries must lie in "
                             f"[0, {self.num_layers})")
        if self.decoder_sparse_step < 1 or not any(
                self.is_sparse_layer(i) for i in range(self.num_layers)):
            raise ValueError(f"decoder_sparse_step={self.decoder_sparse_step}, mlp_only_layers="
                             f"{list(self.mlp_only_layers)} leave no sparse layer among "
                             f"{self.num_layers}: describe the model as a dense one")
        e, k, h, i = (self.num_experts, self.num_experts_per_tok, self.hidden_size,
                      self.moe_intermediate_size)
        if self.arch != "llama" or e < 0:
            raise ValueError("sparse MoE layers need the llama architecture and num_experts > 0")
        if e > MOE_MAX_EXPERTS:
            raise ValueError(f"num_experts={e}: at most {MOE_MAX_EXPERTS} experts are supported")
        if not 1 <= k <= min(MOE_MAX_TOPK, e):
            raise ValueError(f"num_experts_per_tok={k}: 1..{MOE_MAX_TOPK} (and <= num_experts) "
                             "is supported")
        if h % 128 or i <= 0 or i % 128:
            raise ValueError(f"sparse MoE needs hidden_size ({h}) and the expert width ({i}) to "
                             "be multiples of 128 (csrc/kernels/moe.hip)")
        if self.mlp_bias:
            raise ValueError("sparse MoE experts with mlp_bias are not supported")

    @property
    def rope_type(self) -> Optional[str]:
        rs = self.rope_scaling_dict
        return None if not rs else rs.get("rope_type", rs.get("type"))

    @property
    def has_o_proj_bias(self) -> bool:
        return self.attention_bias if self.o_proj_bias is None else self.o_proj_bias

    # ------------------------------------------------------------------ derived
    @property
    def group_size(self) -> int:
        return self.num_heads // self.num_kv_heads

    @property
    def q_size(self) -> int:
        return self.num_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.num_kv_heads * self.head_dim

    @property
    def qkv_size(self) -> int:
        return self.q_size + 2 * self.kv_size

    @property
    def rope_scaling_dict(self) -> Optional[Dict[str, Any]]:
        return dict(self.rope_scaling) if self.rope_scaling is not None else None

    def is_sparse_layer(self, i: int) -> bool:
        """Whether layer ``i`` carries the sparse MoE MLP (HF ``Qwen2MoeDecoderLayer``'s rule);
        False for every layer of a model without experts."""
        return (self.num_experts > 0 and i not in self.mlp_only_layers
                and (i + 1) % self.decoder_sparse_step == 0)

    def layer_param_count(self, layer_idx: Optional[int] = None) -> int:
        """Parameters of layer ``layer_idx``; without an index, of a sparse layer for a model
        with experts (every layer of an all-sparse stack), else of the model's one layer kind."""
        h, i = self.hidden_size, self.intermediate_size
        if self.arch == "gpt2":
            return 4 * h * h + 4 * h + 2 * h * i + i + h + 4 * h
        qk = 2 * self.head_dim if self.qk_norm else 0
        bias = 0
        if self.num_experts:   # models with experts count exactly (Qwen2-MoE's q/k/v bias); the
            # dense models' figure, which leaves the bias vectors out, is kept as it was
            bias = (self.qkv_size if self.attention_bias else 0) + (
                h if self.has_o_proj_bias else 0)
        mlp = 3 * h * i
        sparse = self.num_experts > 0 if layer_idx is None else self.is_sparse_layer(layer_idx)
        if sparse:   # the router + every expert's gate, up and down (+ the shared expert, its gate)
            mlp = h * self.num_experts + self.expert_param_count()
            if self.shared_expert_intermediate_size:
                mlp += 3 * h * self.shared_expert_intermediate_size + h
        return h * self.qkv_size + self.q_size * h + mlp + 2 * h + qk + bias

    def expert_param_count(self, layer_idx: Optional[int] = None) -> int:
        """Per layer: every routed expert's gate, up and down (0 for a dense model and for a
        dense layer of a mixed stack)."""
        if layer_idx is not None and not self.is_sparse_layer(layer_idx):
            return 0
        return self.num_experts * 3 * self.hidden_size * self.moe_intermediate_size

    def param_count(self) -> int:
        emb = self.vocab_size * self.hidden_size
        head = 0 if self.tie_word_embeddings else emb
        if self.arch == "gpt2":
            return self.num_layers * self.layer_param_count() + emb + head + self.hidden_size
        layers = sum(self.layer_param_count(i) for i in range(self.num_layers))
        return layers + emb + head + self.hidden_size

    def kv_bytes_per_token_per_layer(self, dtype_bytes: int = 2) -> int:
        return 2 * self.num_kv_heads * self.head_dim * dtype_bytes

    def replace(self, **kw) -> "ModelSpec":
        return dataclasses.replace(self, **kw)

    def to_dict(self) -> Dict[str, Any]:
        d = dataclasses.asdict(self)
        d["rope_scaling"] = self.rope_scaling_dict
        return d

    # ------------------------------------------------------------------ parsing
    @classmethod
    def from_hf_config(cls, cfg: Any) -> "ModelSpec":
        """Build from a HF ``config.json`` path / directory / dict / ``PretrainedConfig``."""
        if isinstance(cfg, (str, os.PathLike)):
            p = str(cfg)
            if os.path.isdir(p):
                p = os.path.join(p, "config.json")
            with open(p) as f:
                cfg = json.load(f)
        elif not isinstance(cfg, dict):
            cfg = cfg.to_dict()
        mt = cfg.get("model_type", "llama")
        if mt == "gpt2":
            h = cfg.get("n_embd", 768)
            nh = cfg.get("n_head", 12)
            return cls(
                arch="gpt2",
                vocab_size=cfg.get("vocab_size", 50257),
                hidden_size=h,
                intermediate_size=cfg.get("n_inner") or 4 * h,
                num_layers=cfg.get("n_layer", 12),
                num_heads=nh,
                num_kv_heads=nh,
                head_dim=h // nh,
                rms_norm_eps=cfg.get("layer_norm_epsilon", 1e-5),
                rope_theta=0.0,
                max_position_embeddings=cfg.get("n_positions", 1024),
                tie_word_embeddings=True,
                pad_token_id=cfg.get("pad_token_id"),
                bos_token_id=cfg.get("bos_token_id", 50256),
                eos_token_id=cfg.get("eos_token_id", 50256),
                hidden_act=cfg.get("activation_function", "gelu_new"),
                attention_bias=True,
                mlp_bias=True,
                name=cfg.get("_name_or_path", "gpt2") or "gpt2",
            )
        if mt not in ("llama", "mistral", "qwen2", "qwen3", "qwen3_moe", "mixtral", "qwen2_moe"):
            raise ValueError(f"unsupported model_type {mt!r} (supported: llama, mistral, qwen2, "
                             "qwen3, qwen3_moe, mixtral, qwen2_moe, gpt2)")
        # Qwen2: q/k/v projections always carry a bias, o_proj never does (no config key)
        # (Qwen2-MoE: the same attention)
        qwen2 = mt in ("qwen2", "qwen2_moe")
        # Qwen3: per-head q/k RMSNorm; attention_bias from the config, for q/k/v and o_proj alike
        # (Qwen3-MoE: the same attention)
        qwen3 = mt in ("qwen3", "qwen3_moe")
        moe: Dict[str, Any] = {}
        if mt in ("qwen3_moe", "qwen2_moe") and cfg.get("num_experts") is None:
            # transformers 5.x serialises Qwen3MoeConfig.num_experts under Mixtral's name
            cfg = dict(cfg, num_experts=cfg.get("num_local_experts"))
        need = {"qwen3_moe": ("num_experts", "num_experts_per_tok", "moe_intermediate_size"),
                "qwen2_moe": ("num_experts", "num_experts_per_tok", "moe_intermediate_size",
                              "shared_expert_intermediate_size"),
                "mixtral": ("num_local_experts", "num_experts_per_tok", "intermediate_size")}
        lacking = [k for k in need.get(mt, ()) if cfg.get(k) is None]
        if lacking:
            raise ValueError(f"{mt}: the config lacks {', '.join(lacking)}")
        if mt == "qwen3_moe":
            # every layer sparse: HF makes layer i sparse when i is not in mlp_only_layers and
            # (i + 1) % decoder_sparse_step == 0
            if cfg.get("decoder_sparse_step", 1) != 1 or cfg.get("mlp_only_layers"):
                raise ValueError(
                    "qwen3_moe: decoder_sparse_step != 1 or a non-empty mlp_only_layers mixes "
                    "dense and sparse layers; only all-sparse stacks are supported")
            moe = dict(num_experts=cfg["num_experts"],
                       num_experts_per_tok=cfg["num_experts_per_tok"],
                       moe_intermediate_size=cfg["moe_intermediate_size"],
                       norm_topk_prob=bool(cfg.get("norm_topk_prob", False)))
        elif mt == "qwen2_moe":
            # a shared expert in every sparse layer, and HF's rule for which layers are sparse
            # (ModelSpec.is_sparse_layer); the spec's own checks refuse what is not supported
            moe = dict(num_experts=cfg["num_experts"],
                       num_experts_per_tok=cfg["num_experts_per_tok"],
                       moe_intermediate_size=cfg["moe_intermediate_size"],
                       norm_topk_prob=bool(cfg.get("norm_topk_prob", False)),
                       shared_expert_intermediate_size=cfg["shared_expert_intermediate_size"],
                       decoder_sparse_step=int(cfg.get("decoder_sparse_step", 1) or 1),
                       mlp_only_layers=tuple(cfg.get("mlp_only_layers") or ()))
            if moe["shared_expert_intermediate_size"] <= 0:
                raise ValueError("qwen2_moe: shared_expert_intermediate_size="
                                 f"{moe['shared_expert_intermediate_size']}: a positive multiple "
                                 "of 128 is supported")
        elif mt == "mixtral":
            # the expert width is intermediate_size; the top-k weights are always renormalised
            moe = dict(num_experts=cfg["num_local_experts"],
                       num_experts_per_tok=cfg["num_experts_per_tok"],
                       moe_intermediate_size=cfg["intermediate_size"], norm_topk_prob=True)
        sw = cfg.get("sliding_window")
        if (qwen2 or qwen3) and not cfg.get("use_sliding_window", False):
            sw = None
        nh = cfg["num_attention_heads"]
        h = cfg["hidden_size"]
        if qwen3:
            mwl = cfg.get("max_window_layers")
            if sw and mwl is not None and mwl < cfg["num_hidden_layers"]:
                raise ValueError(
                    f"{mt}: use_sliding_window with max_window_layers={mwl} < "
                    f"{cfg['num_hidden_layers']} layers mixes windowed and full-attention layers; "
                    "one window per model is supported")
            hd = cfg.get("head_dim") or h // nh
            if hd not in QK_NORM_HEAD_DIMS:
                raise ValueError(f"{mt}: head_dim {hd} is not supported by the fused q/k norm "
                                 f"(supported: {', '.join(map(str, QK_NORM_HEAD_DIMS))})")
        # transformers 4.x: rope_theta + rope_scaling; transformers 5.x: rope_parameters
        rp = cfg.get("rope_parameters") or {}
        rope_theta = cfg.get("rope_theta", rp.get("rope_theta", 10000.0))
        rs = cfg.get("rope_scaling") or ({k: v for k, v in rp.items() if k != "rope_theta"}
                                         if rp else None)
        if rs is not None and rs.get("rope_type", rs.get("type")) in (None, "default"):
            rs = None
        eos = cfg.get("eos_token_id")
        if isinstance(eos, list):
            eos = eos[0]
        return cls(
            arch="llama",
            vocab_size=cfg["vocab_size"],
            hidden_size=h,
            intermediate_size=cfg["intermediate_size"],
            num_layers=cfg["num_hidden_layers"],
            num_heads=nh,
            num_kv_heads=cfg.get("num_key_value_heads") or nh,
            head_dim=cfg.get("head_dim") or h // nh,
            rms_norm_eps=cfg.get("rms_norm_eps", 1e-6),
            rope_theta=float(rope_theta),
            rope_scaling=tuple(sorted(rs.items())) if rs else None,
            max_position_embeddings=cfg.get("max_position_embeddings", 4096),
            tie_word_embeddings=bool(cfg.get("tie_word_embeddings", False)),
            pad_token_id=cfg.get("pad_token_id"),
            bos_token_id=cfg.get("bos_token_id"),
            eos_token_id=eos,
            hidden_act=cfg.get("hidden_act", "silu"),
            pretraining_tp=cfg.get("pretraining_tp", 1) or 1,
            # (Qwen2-MoE spells its q/k/v bias switch qkv_bias; on unless the config says otherwise)
            attention_bias=(bool(cfg.get("qkv_bias", True)) if mt == "qwen2_moe" else
                            True if qwen2 else bool(cfg.get("attention_bias", False))),
            mlp_bias=bool(cfg.get("mlp_bias", False)),
            name=cfg.get("_name_or_path", mt) or mt,
            model_type=mt,
            o_proj_bias=False if qwen2 else None,
            sliding_window=int(sw) if sw else None,
            output_hidden_states=bool(cfg.get("output_hidden_states", False)),
            qk_norm=qwen3,
            **moe,
        )

    def to_hf_dict(self) -> Dict[str, Any]:
        """Inverse of :meth:`from_hf_config` (used to write ``config.json`` for random-init dirs)."""
        if self.arch == "gpt2":
            return dict(
                model_type="gpt2", vocab_size=self.vocab_size, n_embd=self.hidden_size,
                n_inner=self.intermediate_size, n_layer=self.num_layers, n_head=self.num_heads,
                layer_norm_epsilon=self.rms_norm_eps, n_positions=self.max_position_embeddings,
                activation_function=self.hidden_act, bos_token_id=self.bos_token_id,
                eos_token_id=self.eos_token_id,
            )
        arch_name = {"llama": "LlamaForCausalLM", "mistral": "MistralForCausalLM",
                     "qwen2": "Qwen2ForCausalLM", "qwen3": "Qwen3ForCausalLM",
                     "qwen3_moe": "Qwen3MoeForCausalLM", "qwen2_moe": "Qwen2MoeForCausalLM",
                     "mixtral": "MixtralForCausalLM"}[self.model_type]
        extra: Dict[str, Any] = {}
        if self.model_type in ("mistral", "mixtral"):
            extra["sliding_window"] = self.sliding_window
        if self.model_type == "mixtral":
            extra.update(num_local_experts=self.num_experts,
                         num_experts_per_tok=self.num_experts_per_tok)
        if self.model_type == "qwen3_moe":
            extra.update(num_experts=self.num_experts,
                         num_experts_per_tok=self.num_experts_per_tok,
                         moe_intermediate_size=self.moe_intermediate_size,
                         norm_topk_prob=self.norm_topk_prob, decoder_sparse_step=1,
                         mlp_only_layers=[])
        if self.model_type == "qwen2_moe":
            extra.update(num_experts=self.num_experts,
                         num_experts_per_tok=self.num_experts_per_tok,
                         moe_intermediate_size=self.moe_intermediate_size,
                         shared_expert_intermediate_size=self.shared_expert_intermediate_size,
                         norm_topk_prob=self.norm_topk_prob, qkv_bias=self.attention_bias,
                         decoder_sparse_step=self.decoder_sparse_step,
                         mlp_only_layers=list(self.mlp_only_layers))
        if self.model_type in ("qwen2", "qwen3", "qwen3_moe", "qwen2_moe"):
            extra.update(use_sliding_window=self.sliding_window is not None,
                         sliding_window=self.sliding_window)
        if self.model_type in ("qwen3", "qwen3_moe") and self.sliding_window is not None:
            extra["max_window_layers"] = self.num_layers   # every layer windowed
        return dict(
            extra, model_type=self.model_type, architectures=[arch_name],
            vocab_size=self.vocab_size,
            hidden_size=self.hidden_size, intermediate_size=self.intermediate_size,
            num_hidden_layers=self.num_layers, num_attention_heads=self.num_heads,
            num_key_value_heads=self.num_kv_heads, head_dim=self.head_dim,
            rms_norm_eps=self.rms_norm_eps, rope_theta=self.rope_theta,
            rope_scaling=self.rope_scaling_dict,
            max_position_embeddings=self.max_position_embeddings,
            tie_word_embeddings=self.tie_word_embeddings, pad_token_id=self.pad_token_id,
            bos_token_id=self.bos_token_id, eos_token_id=self.eos_token_id,
            hidden_act=self.hidden_act, pretraining_tp=self.pretraining_tp,
            attention_bias=self.attention_bias, mlp_bias=self.mlp_bias,
            output_hidden_states=self.output_hidden_states,
        )


_LLAMA3_ROPE = (("factor", 8.0), ("high_freq_factor", 4.0), ("low_freq_factor", 1.0),
                ("original_max_position_embeddings", 8192), ("rope_type", "llama3"))

PRESETS: Dict[str, ModelSpec] = {
    "llama-3-8b": ModelSpec(name="llama-3-8b"),
    "llama-3-70b": ModelSpec(
        name="llama-3-70b", hidden_size=8192, intermediate_size=28672, num_layers=80,
        num_heads=64, num_kv_heads=8),
    "llama-3.1-8b": ModelSpec(name="llama-3.1-8b", rope_scaling=_LLAMA3_ROPE,
                              max_position_embeddings=131072),
    "llama-3.1-70b": ModelSpec(
        name="llama-3.1-70b", hidden_size=8192, intermediate_size=28672, num_layers=80,
        num_heads=64, num_kv_heads=8, rope_scaling=_LLAMA3_ROPE, max_position_embeddings=131072),
    "llama-2-7b": ModelSpec(
        name="llama-2-7b", vocab_size=32000, hidden_size=4096, intermediate_size=11008,
        num_layers=32, num_heads=32, num_kv_heads=32, rope_theta=10000.0, rms_norm_eps=1e-5,
        max_position_embeddings=4096, bos_token_id=1, eos_token_id=2),
    "gpt2": ModelSpec(
        name="gpt2", arch="gpt2", vocab_size=50257, hidden_size=768, intermediate_size=3072,
        num_layers=12, num_heads=12, num_kv_heads=12, head_dim=64, rms_norm_eps=1e-5,
        rope_theta=0.0, max_position_embeddings=1024, tie_word_embeddings=True,
        bos_token_id=50256, eos_token_id=50256, hidden_act="gelu_new", attention_bias=True,
        mlp_bias=True),
    "mistral-7b": ModelSpec(
        name="mistral-7b", model_type="mistral", vocab_size=32000, hidden_size=4096,
        intermediate_size=14336, num_layers=32, num_heads=32, num_kv_heads=8, head_dim=128,
        rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768, bos_token_id=1,
        eos_token_id=2, sliding_window=4096),
    "qwen2-7b": ModelSpec(
        name="qwen2-7b", model_type="qwen2", vocab_size=152064, hidden_size=3584,
        intermediate_size=18944, num_layers=28, num_heads=28, num_kv_heads=4, head_dim=128,
        rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=32768,
        bos_token_id=151643, eos_token_id=151645, attention_bias=True, o_proj_bias=False),
    # Qwen3 (per-head q/k RMSNorm, explicit head_dim, no attention bias).  These three were
    # written down without access to the published config.json files: they serve as shapes; a
    # real checkpoint's config.json is parsed (from_hf_config), never looked up here.
    "qwen3-8b": ModelSpec(
        name="qwen3-8b", model_type="qwen3", qk_norm=True, vocab_size=151936, hidden_size=4096,
        intermediate_size=12288, num_layers=36, num_heads=32, num_kv_heads=8, head_dim=128,
        rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=40960,
        bos_token_id=151643, eos_token_id=151645),
    "qwen3-32b": ModelSpec(
        name="qwen3-32b", model_type="qwen3", qk_norm=True, vocab_size=151936, hidden_size=5120,
        intermediate_size=25600, num_layers=64, num_heads=64, num_kv_heads=8, head_dim=128,
        rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=40960,
        bos_token_id=151643, eos_token_id=151645),
    "qwen3-0.6b": ModelSpec(
        name="qwen3-0.6b", model_type="qwen3", qk_norm=True, vocab_size=151936, hidden_size=1024,
        intermediate_size=3072, num_layers=28, num_heads=16, num_kv_heads=8, head_dim=128,
        rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=40960,
        tie_word_embeddings=True, bos_token_id=151643, eos_token_id=151645),
    # sparse MoE (written down like the Qwen3 presets above: shapes, not looked-up configs)
    "qwen3-30b-a3b": ModelSpec(
        name="qwen3-30b-a3b", model_type="qwen3_moe", qk_norm=True, vocab_size=151936,
        hidden_size=2048, intermediate_size=6144, num_layers=48, num_heads=32, num_kv_heads=4,
        head_dim=128, rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=40960,
        bos_token_id=151643, eos_token_id=151645, num_experts=128, num_experts_per_tok=8,
        moe_intermediate_size=768, norm_topk_prob=True),
    "mixtral-8x7b": ModelSpec(
        name="mixtral-8x7b", model_type="mixtral", vocab_size=32000, hidden_size=4096,
        intermediate_size=14336, num_layers=32, num_heads=32, num_kv_heads=8, head_dim=128,
        rms_norm_eps=1e-5, rope_theta=1000000.0, max_position_embeddings=32768, bos_token_id=1,
        eos_token_id=2, num_experts=8, num_experts_per_tok=2, moe_intermediate_size=14336,
        norm_topk_prob=True),
    # Qwen2-MoE: Qwen2 attention, a shared expert beside the routed ones in every sparse layer
    # (shapes, like the presets above; both published models make every layer sparse)
    "qwen1.5-moe-a2.7b": ModelSpec(
        name="qwen1.5-moe-a2.7b", model_type="qwen2_moe", vocab_size=151936, hidden_size=2048,
        intermediate_size=5632, num_layers=24, num_heads=16, num_kv_heads=16, head_dim=128,
        rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=8192,
        bos_token_id=151643, eos_token_id=151643, attention_bias=True, o_proj_bias=False,
        num_experts=60, num_experts_per_tok=4, moe_intermediate_size=1408,
        shared_expert_intermediate_size=5632, norm_topk_prob=False),
    "qwen2-57b-a14b": ModelSpec(
        name="qwen2-57b-a14b", model_type="qwen2_moe", vocab_size=151936, hidden_size=3584,
        intermediate_size=18944, num_layers=28, num_heads=28, num_kv_heads=4, head_dim=128,
        rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=32768,
        bos_token_id=151643, eos_token_id=151643, attention_bias=True, o_proj_bias=False,
        num_experts=64, num_experts_per_tok=8, moe_intermediate_size=2560,
        shared_expert_intermediate_size=20480, norm_topk_prob=False),
    # tiny configs for CPU tests / smoke
    "tiny-llama": ModelSpec(
        name="tiny-llama", vocab_size=512, hidden_size=128, intermediate_size=256, num_layers=4,
        num_heads=4, num_kv_heads=2, head_dim=32, max_position_embeddings=2048,
        rope_theta=10000.0, bos_token_id=1, eos_token_id=2),
    # 8 layers: one per rank in the 8-rank CPU rehearsals of the PP=8 paths
    "tiny-llama-8l": ModelSpec(
        name="tiny-llama-8l", vocab_size=512, hidden_size=128, intermediate_size=256, num_layers=8,
        num_heads=4, num_kv_heads=2, head_dim=32, max_position_embeddings=2048,
        rope_theta=10000.0, bos_token_id=1, eos_token_id=2),
    "tiny-gpt2": ModelSpec(
        name="tiny-gpt2", arch="gpt2", vocab_size=512, hidden_size=128, intermediate_size=512,
        num_layers=4, num_heads=4, num_kv_heads=4, head_dim=32, max_position_embeddings=512,
        rope_theta=0.0, tie_word_embeddings=True, bos_token_id=1, eos_token_id=2,
        hidden_act="gelu_new", attention_bias=True, mlp_bias=True),
}


def refuse_moe_quantization(spec: ModelSpec, mode: Any) -> None:
    """Whole-model weight quantisation of a sparse-MoE model is an error, not a fallback: the
    grouped expert GEMM (csrc/kernels/moe.hip) takes bf16 expert weights, or fp8 ones under the
    mode of its own, "fp8_experts", or MXFP4 ones under "mxfp4_experts", which leave everything
    but the experts bf16 -- and which a model without experts cannot take."""
    if mode in ("fp8_experts", "mxfp4_experts") and not spec.num_experts:
        raise ValueError(f"{mode} needs a sparse MoE model; {spec.name} ({spec.model_type}) "
                         "has no experts")
    if spec.num_experts and mode not in (False, None, "none", "bf16", "fp8_experts",
                                         "mxfp4_experts"):
        mode = "fp8" if mode is True else mode
        raise ValueError(f"{mode} weights are not supported for sparse MoE layers "
                         f"({spec.model_type}, {spec.name}): the grouped expert GEMM takes bf16 "
                         "expert weights, or fp8 expert weights as mode fp8_experts "
                         "(--fp8-experts), or MXFP4 expert weights as mode mxfp4_experts "
                         "(--fp4-experts)")


def resolve_model(model: Any) -> ModelSpec:
    """Accept a preset name, a ``config.json`` path/dir, a dict, a HF config or a ModelSpec."""
    if isinstance(model, ModelSpec):
        return model
    if isinstance(model, str):
        key = model.lower().replace("meta-llama/", "").replace("_", "-")
        key = key.replace("meta-llama-3", "llama-3")
        if key in PRESETS:
            return PRESETS[key]
        if os.path.exists(model):
            return ModelSpec.from_hf_config(model)
        raise ValueError(f"unknown model {model!r}: not a preset ({sorted(PRESETS)}) nor a path")
    return ModelSpec.from_hf_config(model)


# ---------------------------------------------------------------------------------------------
# Stage placement (pipeline planner).  The reference's server stub wants to "choose optimal block
# ids" (server/server.py:7-8) and the worker owns [block_index_start, block_index_end)
# (server/worker.py:13-14).  On one MI355X node every GPU is identical and fully connected, so the
# optimal placement is the contiguous, cost-balanced split below.  The first stage also pays the
# embedding gather and the last stage the LM head, so their layer counts are trimmed by the
# equivalent layer cost.
# ---------------------------------------------------------------------------------------------
def plan_stages(spec: ModelSpec, num_stages: int,
                weights: Optional[Sequence[float]] = None,
                head_rotation: bool = False) -> List[Tuple[int, int]]:
    """Split ``spec.num_layers`` into ``num_stages`` contiguous ``[start, end)`` ranges.

    ``weights`` (optional, one per stage) expresses relative stage speed (e.g. for a degraded GPU
    during rebalancing); the default is uniform hardware.  ``head_rotation``: the decode steps'
    LM head runs on every rank in turn (runtime/head.py), so its cost is shared evenly instead of
    trimming the last stage.

    Stages are balanced by layer count, also for a stack that mixes dense and sparse-MoE layers
    (``ModelSpec.is_sparse_layer``): a sparse layer's decode cost follows the experts it hits,
    not the bytes it holds, and nobody has measured the two layer kinds against each other, so
    no weighting is guessed here.
    """
    L = spec.num_layers
    if num_stages < 1:
        raise ValueError("num_stages must be >= 1")
    if num_stages > L:
        raise ValueError(f"cannot split {L} layers into {num_stages} stages")
    w = list(weights) if weights is not None else [1.0] * num_stages
    if len(w) != num_stages or min(w) <= 0:
        raise ValueError("weights must be positive, one per stage")
    # LM head (+ final norm + sampling) in layer-equivalents of decode time.  By bytes/FLOPs the
    # head is vocab*hidden / layer_params (1.22 layers for Llama-3-70B), but its single wide GEMM
    # runs far more efficiently than a layer (which also carries attention, norms, activation):
    # measured on MI355X at 512 rows, head + sampling 0.78 ms vs 1.06 ms per layer
    # (profiles/pp1_bf16_b512_decode_breakdown.txt) -> factor 0.6.
    head_cost = 0.6 * spec.vocab_size * spec.hidden_size / max(1, spec.layer_param_count())
    extra = [0.0] * num_stages
    if num_stages > 1:
        if head_rotation:
            extra = [head_cost / num_stages] * num_stages
        else:
            extra[-1] += head_cost
    total = (L + sum(extra))
    tw = sum(w)
    # start below the proportional target, then hand out the remaining layers one at a time to
    # the stage whose time after taking it is smallest: this minimises the slowest stage, which
    # sets the pipeline's throughput
    targets = [total * wi / tw - ei for wi, ei in zip(w, extra)]
    counts = [max(1, int(math.floor(t))) for t in targets]
    while sum(counts) > L:
        i = max((k for k in range(num_stages) if counts[k] > 1),
                key=lambda k: (counts[k] + extra[k]) / w[k])
        counts[i] -= 1
    while sum(counts) < L:
        i = min(range(num_stages), key=lambda k: ((counts[k] + 1 + extra[k]) / w[k], k))
        counts[i] += 1
    out, s = [], 0
    for c in counts:
        out.append((s, s + c))
        s += c
    return out


@dataclass
class CacheConfig:
    """KV-cache policy for one stage.

    ``window_length``/``num_sink_tokens`` mirror ``PartialLlamaSinkCache(window_length,
    num_sink_tokens)`` (reference ``models/llama/cache.py:11``).  ``window_length=0`` means a full
    (non-evicting) cache sized from HBM.
    """

    block_size: int = 64
    num_blocks: Optional[int] = None  # None -> sized from free HBM
    gpu_memory_utilization: float = 0.90
    window_length: int = 0
    num_sink_tokens: int = 0
    max_chunk: int = 512  # extra ring headroom so a prefill chunk never evicts keys it needs
    dtype: str = "bf16"   # "bf16" | "fp8" (e4m3fn: half the decode-attention bytes, 2x tokens)
    k_scale: float = 1.0  # fp8 cache stores k / k_scale and v / v_scale
    v_scale: float = 1.0

    def __post_init__(self):
        if self.dtype not in ("bf16", "fp8"):
            raise ValueError(f"KV cache dtype must be 'bf16' or 'fp8', got {self.dtype!r}")

    @property
    def windowed(self) -> bool:
        return self.window_length > 0

    @property
    def torch_dtype(self):
        import torch
        return torch.float8_e4m3fn if self.dtype == "fp8" else torch.bfloat16

    @property
    def dtype_bytes(self) -> int:
        return 1 if self.dtype == "fp8" else 2


@dataclass
class KernelPolicy:
    """Which hand-written kernel takes each hot-path product (read by ``ops`` at every call, so a
    captured hipGraph keeps the choice it was captured with).  The defaults are the measured
    winners; the fields exist for the trade-offs that are real and for A/B runs.  Set from
    ``EngineConfig.kernels`` / ``distribute --kernels k=v,...`` / ``bench.py --kernels``; the
    ``DLI_KERNELS`` environment variable (same syntax) overrides them."""

    # bf16 decode projections on the one-wave-per-SIMD gemm4 kernel (else the 8-wave gemm_tile):
    # 70B decode step 75.0 vs 77.7 ms (profiles/r4/gemm4_step_ab.txt)
    gemm4: bool = True
    # fp8 decode projections on gemm4 (16x16x128 block-scaled MFMA, G4S8 k-loop; bit-identical
    # to gemm_tile) instead of gemm_tile: "all", "none", or a "+"-separated subset of qkv / o /
    # gate_up / down.  gate|up: 202 vs 219 us alone, +1.9 % tok/s in-step; the others win 2-7 %
    # alone but stay within noise in-step (profiles/r5/fp8_gemm4_16x16.md)
    fp8_gemm4: str = "gate_up"
    # bf16 gemm4 k-loop schedule at decode M (<= 2 row tiles of 256): 8 / 9 = 4 / 6 with the
    # weight stream non-temporal, or 4, 6 (csrc/kernels/gemm4.hip G4Sched; 8: +1.4 % tok/s over
    # 6 in-step, profiles/r5/gemm4_sched_nt.md)
    gemm4_decode_sched: int = 8
    # split-K partials of the deferred projections (QKV, O, down) stored as bf16 (else fp32);
    # consumers always sum in fp32 (profiles/bf16_partials_ab.txt, docs/parity.md C6)
    bf16_partials: bool = True
    # split-K partials summed by their consumer kernel (RMSNorm / RoPE / quantiser) instead of a
    # reduce pass; with fp32 partials both are bit-identical (the tests' reference path)
    defer_splitk: bool = True
    # fp8: SwiGLU / attention outputs handed to the next projection as MX (e8m0 per 128-column
    # block, quantised in the producer's epilogue) instead of bf16 + a per-row quantiser pass
    fp8_mx: bool = True
    # hand-written tile GEMMs for the decode projections at all (False: hipBLASLt everywhere)
    tile_gemms: bool = True
    # hipBLASLt for the products the tile kernels do not take well (M < 128, the LM head).  None = automatic: off when pipeline ranks share a GPU (DLI_SHARE_GPU), because its
    # stream-K kernels wait on each other's workgroups (README "What else couples streams")
    library_gemms: Optional[bool] = None
    # largest M that stays on the tile kernels when library GEMMs are on (0: no bound - large-M
    # prefill products run on gemm4 / gemm_tile too).  Above 2048 hipBLASLt stays: at the
    # headline's 16384-row prefill chunks it runs the 70B projections at 1.63 PF against gemm4's
    # 1.36 (rocprof, profiles/r6/pgemm/top_*.txt; prefill 25.5 vs 29.2 s).  A single-prompt TTFT
    # reads the other way (32k: 4.89 vs 5.55 s) only because the first request pays hipBLASLt's
    # lazy code-object loads for its new shapes - a one-time cost, not a per-request one.
    tile_gemm_max_m: int = 2048
    # ... and the executor runs each such projection once at start-up (StageExecutor.
    # warm_prefill_gemms), so the first long prompt does not pay hipBLASLt's code-object loads
    warm_library_gemms: bool = True
    # run the partial last wave of whole-K bf16 gemm_tile products stream-K (neutral in-step)
    stream_k_tail: bool = False
    # 1-2 decode rows on the weight-streaming GEMVs, with the input RMSNorm, RoPE/KV write and
    # SwiGLU fused into them (else the batch path)
    gemv: bool = True
    # ... with the RMSNorms fused into the QKV / gate|up GEMVs (bit-identical norm arithmetic)
    gemv_norm: bool = True
    # LLM.int8: a resident transposed int8 copy of every weight for the outlier-column gather
    # (1.6 vs 2.9 ms per 70B step, but one more byte per weight: a third less KV capacity)
    int8_transposed: bool = False
    # prefill attention on the 32x32x16-MFMA kernel (csrc/kernels/attn_prefill32.hip: 32 query
    # rows per wave, 64-key steps) wherever it applies (bf16 full cache, head_dim 128, any GQA
    # group incl. MHA, no custom mask); else attention.hip's 16x16x32 kernel
    prefill_m32: bool = True
    # MXFP4 weights: products of more than 2 rows on the MFMA-native fp4 x fp8 tile GEMM
    # (csrc/kernels/gemm_fp4.hip; activations quantised to MX fp8 first) instead of dequantising
    # the weight to bf16.  Experimental and off: it changes the numerics of those products (fp8
    # activation rounding; docs/kernels.md "MXFP4 weights")
    fp4_mfma: bool = False
    # MXFP4 weights: products of 3 to this many rows on the weight-streaming MFMA kernel
    # (csrc/kernels/gemm_fp4_small.hip: the weight read once at 17/32 byte and widened in
    # registers, bf16 activations -- the dequantise path's numerics) instead of dequantising the
    # weight to bf16; checked before fp4_mfma.  0 = off, else 3..32 (docs/kernels.md "MXFP4
    # weights" has the measured crossover)
    fp4_small_m: int = 0
    # fp8 weights: products of 3 to this many bf16 rows on the weight-streaming MFMA kernel
    # (csrc/kernels/gemm_fp8_small.hip: the weight read once and widened to bf16 in registers, the
    # activations never quantised -- the fp8 GEMV's numerics for bf16 rows) instead of quantising
    # the rows for torch._scaled_mm or the block-scaled tile GEMM.  0 = off, else 3..32
    # (docs/kernels.md "fp8 weights, 3-32 rows" has the measured crossover)
    fp8_small_m: int = 0
    # sparse MoE, bf16 experts: calls whose mean rows per expert T k / E reach this many run the
    # routed experts on the grouped MFMA tile GEMM (csrc/kernels/moe_tile.hip: 128-row tiles, a
    # weight byte read once per 128 rows) instead of the weight-streaming kernel's 32-row tiles.
    # 0 = off, else 32..1024 (docs/kernels.md "Sparse MoE: tile GEMM" has the measured
    # crossover); the CPU path ignores it, and fp8 / MXFP4 experts follow moe_tile_rows_q instead
    moe_tile_rows: int = 0
    # sparse MoE, fp8 / MXFP4 experts: the same switch for quantised experts (moe_tile.hip's fp8
    # and MXFP4 instantiations: the quantised bytes staged in LDS and widened to bf16 at
    # fragment-read time).  A knob of its own: the weight-streaming kernel reads a half or a
    # quarter of the bytes here, so the crossover is not the bf16 one.  0 = off, else 32..1024.
    # Suggested where prefill matters: 32, the smallest mean rows per expert at which both
    # Qwen3-30B-A3B and Mixtral-8x7B shapes were measured, and faster than the weight-streaming
    # kernel on both, in both formats (docs/kernels.md "Sparse MoE: tile GEMM, quantised
    # experts": 3.6-4.9x at 2048-8192 rows for fp8, 3.1-4.0x for MXFP4)
    moe_tile_rows_q: int = 0

    _FP8_SHAPES = ("qkv", "o", "gate_up", "down")

    def __post_init__(self):
        if self.fp4_small_m != 0 and not 3 <= self.fp4_small_m <= 32:
            raise ValueError(f"fp4_small_m={self.fp4_small_m}: 0 (off) or 3..32")
        if self.fp8_small_m != 0 and not 3 <= self.fp8_small_m <= 32:
            raise ValueError(f"fp8_small_m={self.fp8_small_m}: 0 (off) or 3..32")
        if self.moe_tile_rows != 0 and not 32 <= self.moe_tile_rows <= 1024:
            raise ValueError(f"moe_tile_rows={self.moe_tile_rows}: 0 (off) or 32..1024")
        if self.moe_tile_rows_q != 0 and not 32 <= self.moe_tile_rows_q <= 1024:
            raise ValueError(f"moe_tile_rows_q={self.moe_tile_rows_q}: 0 (off) or 32..1024")
        if self.gemm4_decode_sched not in (4, 6, 8, 9):
            raise ValueError(f"gemm4_decode_sched={self.gemm4_decode_sched}: 4, 6, 8 or 9")
        sel = self.fp8_gemm4
        if sel not in ("all", "none") and any(
                x not in self._FP8_SHAPES for x in sel.split("+")):
            raise ValueError(f"fp8_gemm4={sel!r}: 'all', 'none' or a '+' list of "
                             f"{'/'.join(self._FP8_SHAPES)}")

    def fp8_on_gemm4(self, shape: str) -> bool:
        return self.gemm4 and (self.fp8_gemm4 == "all" or shape in self.fp8_gemm4.split("+"))

    def with_overrides(self, spec: str) -> "KernelPolicy":
        """``"gemm4=0,library_gemms=auto"`` applied on top of this policy."""
        if not spec or not spec.strip():
            return self
        kw: Dict[str, Any] = {}
        names = {f.name: f for f in dataclasses.fields(self)}
        for item in spec.split(","):
            if not item.strip():
                continue
            k, _, v = item.partition("=")
            k, v = k.strip(), v.strip()
            if k not in names:
                raise ValueError(f"unknown kernel policy field {k!r} (known: {sorted(names)})")
            if k == "fp8_gemm4":
                kw[k] = v
            elif names[k].type in (int, "int"):
                kw[k] = int(v)
            elif k == "library_gemms" and v.lower() in ("auto", "none", ""):
                kw[k] = None
            elif v.lower() in ("1", "true", "on", "yes"):
                kw[k] = True
            elif v.lower() in ("0", "false", "off", "no"):
                kw[k] = False
            else:
                raise ValueError(f"kernel policy {k}={v!r}: expected 0/1")
        return dataclasses.replace(self, **kw)


@dataclass
class ServeConfig:
    max_batch_size: int = 256
    max_num_batched_tokens: int = 8192
    num_micro_batches: int = 0  # 0 -> num_stages (+0) for a full pipeline
    max_seq_len: int = 8192
    use_graphs: bool = True
    # decode steps' LM head + sampling on every pipeline rank in turn (runtime/head.py) instead of
    # the last stage only; env DLI_HEAD_ROTATION=0/1 overrides
    head_rotation: bool = True
    # rows of the sampling rank's penalty table (int32 [slots, vocab]) = running sequences that
    # can use repetition / presence / frequency penalties at once; 0 = no table, no penalty
    # kernels anywhere, and such requests are refused (min_p needs no slot)
    penalty_slots: int = 0
    graph_batch_sizes: List[int] = field(default_factory=lambda: [1, 2, 4, 8, 16, 32, 64, 96, 128,
                                                                  160, 192, 224, 256])
