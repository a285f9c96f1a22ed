"""MI355X-native Llama family (llama2 / llama3 dims).

This replaces the reference's external `ibm-fms` model zoo
(reference call sites: main_training_llama.py:7, :59-65). The architecture
is the standard pre-norm transformer with RMSNorm, rotary GQA attention and
SwiGLU MLP; every hot op dispatches through `fms_fsdp_amd.ops`, which routes
to hand-written CDNA4 HIP kernels on a GPU and to plain fp32-upcast PyTorch
reference implementations on CPU (used by the CPU test suite as the
numerics oracle).

Convention notes (deliberate deltas from ibm-fms internals):
- RoPE uses the half-rotation layout (HF convention), so the HF export
  (fms_to_hf_llama.py parity) needs no q/k interleave permutation
  (reference: fms_to_hf_llama.py:104-124 exists only because fms uses the
  interleaved layout).
- QKV is one fused projection; gate/up is one fused projection — a single
  hipBLASLt GEMM each instead of 2-3 (reference fms keeps them fused too:
  fms_to_hf_llama.py:69-76, :89-95).
"""

import math
import os
from dataclasses import dataclass


import torch
import torch.nn as nn

from fms_fsdp_amd import ops


@dataclass
class LlamaConfig:
    src_vocab_size: int = 32000
    emb_dim: int = 4096
    nheads: int = 32
    kvheads: int = 0          # 0 -> = nheads (MHA)
    nlayers: int = 32
    hidden_grow_factor: float = 8 / 3
    multiple_of: int = 256
    max_expected_seq_len: int = 4096
    rope_theta: float = 10000.0
    norm_eps: float = 1e-6

    def __post_init__(self):
        if self.kvheads == 0:
            self.kvheads = self.nheads
        assert self.nheads % self.kvheads == 0
        assert self.emb_dim % self.nheads == 0

    @property
    def head_dim(self):
        return self.emb_dim // self.nheads

    @property
    def hidden_dim(self):
        h = int(self.emb_dim * self.hidden_grow_factor)
        # round up to multiple_of (matches llama reference arithmetic; the
        # registry's grow factors are exact so this is a no-op for them)
        return self.multiple_of * math.ceil(h / self.multiple_of)


class RMSNorm(nn.Module):
    """y = x / rms(x) * w — dispatches to the CDNA4 one-workgroup-per-row
    kernel on GPU (ops/hip/rmsnorm.hip)."""

    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x):
        return ops.rmsnorm(x, self.weight, self.eps)

    def reset_parameters(self):
        nn.init.ones_(self.weight)


class RotaryEmbedding(nn.Module):
    """Precomputed cos/sin tables (fp32), shared across layers.

    The table precompute replaces the reference's post-FSDP
    `rot_emb.compute_freqs_cis` warm-up (main_training_llama.py:92-96); we
    register it as a buffer so it moves with the model and is built once.
    """

    def __init__(self, head_dim, max_seq_len, theta):
        super().__init__()
        self.head_dim = head_dim
        self.max_seq_len = max_seq_len
        self.theta = theta
        cos, sin = self._build(max_seq_len)
        self.register_buffer("cos", cos, persistent=False)
        self.register_buffer("sin", sin, persistent=False)

    def _build(self, seqlen):
        inv_freq = 1.0 / (
            self.theta ** (torch.arange(0, self.head_dim, 2, dtype=torch.float32) / self.head_dim)
        )
        t = torch.arange(seqlen, dtype=torch.float32)
        freqs = torch.outer(t, inv_freq)          # (S, D/2)
        return freqs.cos(), freqs.sin()

    def get(self, seqlen, device):
        if seqlen > self.cos.shape[0]:
            cos, sin = self._build(seqlen)
            self.cos, self.sin = cos.to(device), sin.to(device)
        return self.cos[:seqlen], self.sin[:seqlen]

    def reset_parameters(self):
        # rebuild the tables — required after a meta-device to_empty(),
        # which leaves the buffers allocated but uninitialized
        cos, sin = self._build(self.max_seq_len)
        with torch.no_grad():
            self.cos.copy_(cos)
            self.sin.copy_(sin)


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.nheads = cfg.nheads
        self.kvheads = cfg.kvheads
        self.head_dim = cfg.head_dim
        qkv_out = (cfg.nheads + 2 * cfg.kvheads) * cfg.head_dim
        self.qkv = nn.Linear(cfg.emb_dim, qkv_out, bias=False)
        self.proj = nn.Linear(cfg.emb_dim, cfg.emb_dim, bias=False)
        # wgrads accumulate straight into the sharded runtime's flat grad
        # buffer when wrapped (ops.linear_flat; no-op for plain models)
        self.qkv.weight._direct_wgrad = True
        self.proj.weight._direct_wgrad = True

    def _project_out(self, o2, residual, b, s):
        """Output projection; residual add fused into the GEMM epilogue.
        TP (_disable_fused_residual) must go through the proj MODULE —
        its all-reduce hook is registered on it."""
        if getattr(self, "_disable_fused_residual", False):
            out = self.proj(o2.reshape(b * s, -1)).view(b, s, -1)
            return out if residual is None else out + residual
        return ops.linear_flat(o2.view(b, s, -1), self.proj.weight, residual)

    def forward(self, x, cos, sin, cache=None, residual=None, doc_mask=None):
        """doc_mask (ops.DocMask): attention stays inside each document of a
        packed row. The KV-cache decode path ignores it."""
        b, s, _ = x.shape
        if getattr(self, "_disable_fused_residual", False):
            qkv = self.qkv(x)
        else:
            qkv = ops.linear_flat(x, self.qkv.weight)
        if (cache is None and qkv.is_cuda and s % 128 == 0
                and self.head_dim in (64, 128)
                and qkv.dtype == torch.bfloat16
                and os.environ.get("FMS_AMD_ALLOW_TORCH_SDPA") != "1"
                and os.environ.get("FMS_AMD_DISABLE_FUSED_QKV") != "1"):
            # fused split+RoPE+attention: strided kernels read q/k/v
            # straight from the fused projection; backward fills one
            # fused dqkv buffer (no cat/copies)
            o = ops.qkv_rope_attention(qkv, cos, sin, self.nheads,
                                       self.kvheads, self.head_dim,
                                       doc_mask=doc_mask)
            return self._project_out(o.reshape(b, s, -1), residual, b, s)
        q, k, v = qkv.split(
            [self.nheads * self.head_dim,
             self.kvheads * self.head_dim,
             self.kvheads * self.head_dim], dim=-1)
        q = q.view(b, s, self.nheads, self.head_dim)
        k = k.view(b, s, self.kvheads, self.head_dim)
        v = v.view(b, s, self.kvheads, self.head_dim)
        if isinstance(cache, ops.KVCache):
            # preallocated cache (generate()): q/k/v stay slices of the
            # fused projection; RoPE and the append are one kernel, the
            # attention a decode kernel over the cache (ops.attention_cached)
            o = ops.attention_cached(q, k, v, cache, cos, sin)
            return self._project_out(o.reshape(b, s, -1), residual, b, s)
        q, k = ops.rope_apply(q, k, cos, sin)
        if cache is not None:
            # plain dict cache: the former route, K/V grown by torch.cat
            # and torch SDPA (generate() passes an ops.KVCache instead)
            import torch.nn.functional as F
            if cache.get("k") is not None:
                k = torch.cat([cache["k"], k], dim=1)
                v = torch.cat([cache["v"], v], dim=1)
            cache["k"], cache["v"] = k, v
            o = F.scaled_dot_product_attention(
                q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                is_causal=(s == k.shape[1]),
                enable_gqa=(self.kvheads != self.nheads)).transpose(1, 2)
        else:
            o = ops.attention_causal(q, k, v, doc_mask=doc_mask)   # (b,s,h,d)
        return self._project_out(o.reshape(b, s, -1), residual, b, s)

    def reset_parameters(self):
        for lin in (self.qkv, self.proj):
            nn.init.trunc_normal_(lin.weight, mean=0.0, std=0.02)


class SwiGLU(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.hidden_dim = cfg.hidden_dim
        self.wg1 = nn.Linear(cfg.emb_dim, 2 * cfg.hidden_dim, bias=False)  # fused gate|up
        self.w2 = nn.Linear(cfg.hidden_dim, cfg.emb_dim, bias=False)
        self.wg1.weight._direct_wgrad = True
        self.w2.weight._direct_wgrad = True

    def forward(self, x, residual=None):
        if getattr(self, "_disable_fused_residual", False):   # TP path
            gu = self.wg1(x)
            h = ops.swiglu(gu)
            out = self.w2(h)
            return out if residual is None else out + residual.view_as(out)
        gu = ops.linear_flat(x, self.wg1.weight)
        h = ops.swiglu(gu)                         # silu(g) * u, fused kernel
        return ops.linear_flat(h, self.w2.weight, residual)

    def reset_parameters(self):
        for lin in (self.wg1, self.w2):
            nn.init.trunc_normal_(lin.weight, mean=0.0, std=0.02)


class LlamaBlock(nn.Module):
    """One transformer block — the FSDP wrapping unit (the analog of the
    reference's LLaMABlock wrap target, fms_fsdp/policies/wrapping.py:6-14)."""

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.attn_norm = RMSNorm(cfg.emb_dim, cfg.norm_eps)
        self.attn = Attention(cfg)
        self.mlp_norm = RMSNorm(cfg.emb_dim, cfg.norm_eps)
        self.mlp = SwiGLU(cfg)
        # norm wgrads land in the sharded runtime's flat grad buffer from
        # the backward kernel itself (ops.rmsnorm; no-op for plain models)
        self.attn_norm.weight._direct_wgrad = True
        self.mlp_norm.weight._direct_wgrad = True

    def forward(self, x, cos, sin, cache=None, doc_mask=None):
        if cache is None and getattr(self, "_ac_enabled", False) \
                and torch.is_grad_enabled():
            return torch.utils.checkpoint.checkpoint(
                self._forward_impl, x, cos, sin, None, doc_mask,
                use_reentrant=False)
        return self._forward_impl(x, cos, sin, cache, doc_mask)

    def _forward_impl(self, x, cos, sin, cache=None, doc_mask=None):
        # both residual adds ride the projection GEMM epilogues (addmm);
        # the residual stream passes THROUGH each norm op, so in backward
        # its grad is added inside the norm's dx kernel
        n, x_res = ops.rmsnorm_residual(x, self.attn_norm.weight,
                                        self.attn_norm.eps)
        h = self.attn(n, cos, sin, cache, residual=x_res, doc_mask=doc_mask)
        n, h_res = ops.rmsnorm_residual(h, self.mlp_norm.weight,
                                        self.mlp_norm.eps)
        return self.mlp(n, residual=h_res)

    def reset_parameters(self):
        for m in (self.attn_norm, self.attn, self.mlp_norm, self.mlp):
            m.reset_parameters()


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.config = cfg
        self.embedding = nn.Embedding(cfg.src_vocab_size, cfg.emb_dim)
        self.rot_emb = RotaryEmbedding(cfg.head_dim, cfg.max_expected_seq_len, cfg.rope_theta)
        self.layers = nn.ModuleList([LlamaBlock(cfg) for _ in range(cfg.nlayers)])
        self.norm = RMSNorm(cfg.emb_dim, cfg.norm_eps)
        self.norm.weight._direct_wgrad = True
        self.lm_head = nn.Linear(cfg.emb_dim, cfg.src_vocab_size, bias=False)
        # token id that ends a document in packed rows; when set, forward()
        # masks attention at document boundaries (config knob `doc_mask`)
        self.doc_mask_token = None

    def forward(self, tokens, labels=None, include_embeds=False,
                doc_mask=None):
        """tokens (b, s) int64 -> logits (b, s, V); with labels also the
        mean CE loss via the chunked fused kernel (never materializes the
        fp32 softmax — SURVEY.md hard-part 6). include_embeds additionally
        returns the final hidden states (speculator training input,
        reference analog: EmbedLLaMA, train_speculator_utils.py:430-466).
        doc_mask (ops.DocMask) keeps attention inside each document of a
        packed row; with `doc_mask_token` set it is built from `tokens`,
        once, and shared by all layers. RoPE positions are not reset."""
        b, s = tokens.shape
        if doc_mask is None and self.doc_mask_token is not None:
            doc_mask = ops.doc_mask_from_tokens(tokens, self.doc_mask_token)
        x = self.embedding(tokens)
        cos, sin = self.rot_emb.get(s, x.device)
        for layer in self.layers:
            x = layer(x, cos, sin, doc_mask=doc_mask)
        x = self.norm(x)
        if labels is not None:
            loss = ops.linear_cross_entropy(x, self.lm_head.weight, labels)
            return (loss, x) if include_embeds else loss
        logits = self.lm_head(x)
        return (logits, x) if include_embeds else logits

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens, temperature=1.0,
                 do_sample=True, include_embeds=False):
        """KV-cached autoregressive generation, optionally returning the
        hidden state of each generated position (reference analog:
        speculator/train_speculator_utils.py:28-118 generate())."""
        b, s0 = input_ids.shape
        caches = None
        tokens = input_ids
        embeds = []
        cur = input_ids
        pos = 0
        for step in range(max_new_tokens):
            x = self.embedding(cur)
            if caches is None:
                # one preallocated cache per layer; head counts from the
                # module (tensor parallelism has already divided them)
                caches = [ops.KVCache(b, s0 + max_new_tokens,
                                      layer.attn.kvheads, layer.attn.head_dim,
                                      x.dtype, x.device)
                          for layer in self.layers]
            total = pos + cur.shape[1]
            cos, sin = self.rot_emb.get(total, x.device)
            cos_c, sin_c = cos[pos:total], sin[pos:total]
            for layer, cache in zip(self.layers, caches):
                x = layer(x, cos_c, sin_c, cache)
            x = self.norm(x)
            h_last = x[:, -1:]
            logits = self.lm_head(h_last)[:, -1]
            if do_sample:
                probs = torch.softmax(logits.float() / temperature, dim=-1)
                nxt = torch.multinomial(probs, 1)
            else:
                nxt = logits.argmax(-1, keepdim=True)
            embeds.append(h_last)
            tokens = torch.cat([tokens, nxt], dim=1)
            pos = total
            cur = nxt
        if include_embeds:
            return tokens, torch.cat(embeds, dim=1)
        return tokens

    def reset_root_parameters(self):
        """Init of the non-block params only — called alone by the
        streamed meta-device path (ShardedModel._materialize_from_meta)
        so the RNG draw order matches reset_parameters() exactly."""
        nn.init.trunc_normal_(self.embedding.weight, mean=0.0, std=0.02)
        nn.init.trunc_normal_(self.lm_head.weight, mean=0.0, std=0.02)
        self.norm.reset_parameters()

    def reset_parameters(self):
        self.reset_root_parameters()
        for layer in self.layers:
            layer.reset_parameters()

    def param_count(self):
        return sum(p.numel() for p in self.parameters())
