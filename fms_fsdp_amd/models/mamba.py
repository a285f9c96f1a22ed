"""Mamba2 (+hybrid attention) language model, MI355X-native.

Replaces the external `mamba_ssm` dependency of the reference
(main_training_mamba.py:8-10 there; config dict shape from
config_utils.py:162-185). The selective-scan uses the chunked SSD
formulation (state-space dual): the compute is dominated by batched
GEMMs (C@B^T, P@X, state updates) that run on hipBLASLt through torch,
with a short python recurrence over chunks; autograd provides the exact
backward. Hot elementwise pieces (softplus-dt, gated RMSNorm epilogue,
causal-conv1d) are fused HIP kernels where available.

Block layout matches mamba_ssm's Mamba2:
  in_proj: d -> 2*d_inner + 2*ngroups*d_state + nheads   (z | xBC | dt)
  causal depthwise conv (width d_conv) + silu over xBC
  SSD(x, dt, A, B, C) + D skip
  gated RMSNorm: norm(y * silu(z)), then out_proj
"""

import math
import os
from dataclasses import dataclass, field
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from fms_fsdp_amd import ops
from fms_fsdp_amd.models.llama import RMSNorm, RotaryEmbedding


@dataclass
class MambaConfig:
    d_model: int = 2560
    d_intermediate: int = 0
    n_layer: int = 64
    vocab_size: int = 50277
    ssm_cfg: dict = field(default_factory=dict)
    attn_layer_idx: List[int] = field(default_factory=list)
    attn_cfg: dict = field(default_factory=dict)
    rms_norm: bool = True
    residual_in_fp32: bool = True
    fused_add_norm: bool = True
    pad_vocab_size_multiple: int = 16
    tie_embeddings: bool = False

    # Mamba2 head geometry
    d_state: int = 128
    d_conv: int = 4
    expand: int = 2
    headdim: int = 64
    ngroups: int = 1
    chunk_size: int = 128

    def __post_init__(self):
        if self.vocab_size % self.pad_vocab_size_multiple != 0:
            self.vocab_size += (self.pad_vocab_size_multiple
                                - self.vocab_size % self.pad_vocab_size_multiple)

    @classmethod
    def from_dict(cls, d):
        known = {k: v for k, v in d.items() if k in cls.__dataclass_fields__}
        return cls(**known)


def segsum(x):
    """x (..., Q) -> (..., Q, Q) cumulative segment sums:
    out[.., i, j] = sum_{j < k <= i} x[.., k], -inf above diagonal."""
    Q = x.shape[-1]
    cs = x.cumsum(-1)
    out = cs[..., :, None] - cs[..., None, :]
    mask = torch.tril(torch.ones(Q, Q, dtype=torch.bool, device=x.device), 0)
    return out.masked_fill(~mask, -torch.inf)


def doc_chunk_keep(doc_start, chunk):
    """(b, l) document starts -> (b, nc, nc) bool over the inter-chunk
    decay matrix W: entry [z, c] (z >= c) carries the state chunk c hands
    on to the end of chunk z. It survives iff the last token of chunk z
    still belongs to the document of the last token of chunk c, i.e.
    start[(z+1)Q - 1] <= (c+1)Q - 1."""
    b, l = doc_start.shape
    last = torch.arange(chunk - 1, l, chunk, device=doc_start.device)  # (nc)
    return doc_start.long()[:, last][:, :, None] <= last[None, None, :]


def _doc_rel_start(doc_start, chunk):
    """(b, nc, Q): document start of every token relative to the first
    position of its chunk (negative: it began in an earlier chunk)."""
    b, l = doc_start.shape
    first = torch.arange(l, device=doc_start.device) // chunk * chunk
    return (doc_start.long() - first).view(b, l // chunk, chunk)


def ssd_chunked(x, dt, A, B, C, chunk, doc_start=None,
                return_final_state=False):
    """State-space dual scan (fp32 math).

    x (b,l,h,p), dt (b,l,h) [already softplus'ed], A (h) [negative],
    B/C (b,l,g,n). Returns y (b,l,h,p). Exact parallel-chunk algorithm:
    diagonal blocks via masked C B^T, inter-chunk state recurrence.

    doc_start (b,l) (ops.DocMask.start): the state is reset at every
    document start of a packed row, y_i = sum over start[i] <= j <= i.
    Four selects to exact 0 on the decay factors: the intra-chunk L, the
    decay into the chunk-final state (only the chunk's last document feeds
    it), the inter-chunk W (doc_chunk_keep) and the decay out of the
    carried state (only tokens whose document began before their chunk
    read it).

    return_final_state: also return the state after the last token, fp32
    (b, h, p, n): the row of the inter-chunk matrix the scan itself never
    needs (the decay of every chunk's state to the end of the sequence).
    """
    b, l, h, p = x.shape
    g, n = B.shape[2], B.shape[3]
    assert l % chunk == 0, f"seq len {l} must divide chunk {chunk}"
    nc = l // chunk
    rep = h // g

    xc = x.view(b, nc, chunk, h, p)
    dtc = dt.view(b, nc, chunk, h)
    Bc = B.view(b, nc, chunk, g, n)
    Cc = C.view(b, nc, chunk, g, n)

    dA = (dtc * A.view(1, 1, 1, h)).permute(0, 1, 3, 2).contiguous()
    # contiguous before the scan: cumsum on a strided last dim falls off
    # the vectorized path (measured ~25x slower)
    dA_cs = dA.cumsum(-1)                            # (b,nc,h,Q)

    # matmul-shaped work runs in bf16 with fp32 accumulation (MFMA rate;
    # mamba_ssm's own kernels take bf16 x/B/C the same way) — decay and
    # cumsum terms stay fp32. On CPU keep fp32 (bf16 matmul is slow there).
    mm_dtype = torch.bfloat16 if x.is_cuda else torch.float32
    Bm = Bc.to(mm_dtype)
    Cm = Cc.to(mm_dtype)

    # diagonal block: Y[i] = sum_{j<=i} C_i.B_j exp(dA[i]-dA[j]) dt_j x_j
    # scores C.B^T are PER GROUP (g << h; g = 1 for the registry
    # configs): computing them per query-head — or materializing
    # repeat_interleave'd (b,nc,Q,h,n) copies of B/C — wastes (h/g)x
    # flops and HBM. The (Q x Q)-sized L is emitted bf16 in ONE fused
    # kernel pass (ops/hip/ssd.hip).
    from fms_fsdp_amd.ops import segsum_exp
    L = segsum_exp(dA_cs).to(mm_dtype)               # (b,nc,h,Q,Q)
    if doc_start is not None:
        rel = _doc_rel_start(doc_start, chunk)       # (b,nc,Q)
        qpos = torch.arange(chunk, device=x.device)
        inside = qpos >= rel[..., None]              # (b,nc,Q,Q): j >= rel_i
        L = torch.where(inside[:, :, None], L, torch.zeros_like(L))
    scores_g = torch.einsum("bcqgn,bckgn->bcgqk", Cm, Bm)  # (b,nc,g,Q,Q)
    sL = scores_g.view(b, nc, g, 1, chunk, chunk) * \
        L.view(b, nc, g, rep, chunk, chunk)
    xdt = xc * dtc.unsqueeze(-1)                     # (b,nc,Q,h,p)
    xdt_m = xdt.to(mm_dtype)
    y_diag = torch.einsum(
        "bcgrqk,bckgrp->bcqgrp", sL,
        xdt_m.view(b, nc, chunk, g, rep, p)).float() \
        .reshape(b, nc, chunk, h, p)

    # chunk-final states: S_c = sum_j exp(dA_end - dA_j) B_j^T (dt_j x_j)
    # — the decay is per-head, so fold it into xdt instead of
    # materializing a decayed copy of B over all heads
    decay_states = torch.exp(dA_cs[..., -1:] - dA_cs)           # (b,nc,h,Q)
    if doc_start is not None:
        decay_states = torch.where((qpos >= rel[..., -1:])[:, :, None],
                                   decay_states,
                                   torch.zeros_like(decay_states))
    xdt_dec = xdt_m * decay_states.permute(0, 1, 3, 2) \
        .unsqueeze(-1).to(mm_dtype)
    states = torch.einsum(
        "bckgn,bckgrp->bcgrnp", Bm,
        xdt_dec.view(b, nc, chunk, g, rep, p)).float() \
        .reshape(b, nc, h, n, p)                                # (b,nc,h,n,p)

    # inter-chunk recurrence in closed form: prev[z] = sum_{c<z}
    # (prod_{c<k<z} D_k) S_c = (exp(segsum(log D)) @ S)[z-1] — one einsum
    # over the (nc x nc) chunk-decay matrix instead of a sequential
    # Python loop (which cost thousands of tiny kernel launches).
    G = dA_cs[..., -1].permute(0, 2, 1)                         # (b,h,nc)
    W = torch.exp(segsum(G))                                    # (b,h,nc,nc)
    if doc_start is not None:
        W = torch.where(doc_chunk_keep(doc_start, chunk)[:, None], W,
                        torch.zeros_like(W))
    # shift the tiny decay matrix, not the big states tensor
    Wsh = torch.cat([torch.zeros_like(W[:, :, :1]), W[:, :, :-1]], dim=2)
    prev_states = torch.einsum("bhzc,bchnp->bzhnp", Wsh, states)  # (b,nc,h,n,p)

    # off-diagonal: Y_off[i] = C_i exp(dA_cs[i]) S_{c-1} — C stays per
    # group; the per-(q,h) decay multiplies the GEMM OUTPUT (size h*p)
    # instead of a materialized decayed C copy (size h*n)
    state_decay = torch.exp(dA_cs)                              # (b,nc,h,Q)
    if doc_start is not None:
        state_decay = torch.where((rel < 0)[:, :, None], state_decay,
                                  torch.zeros_like(state_decay))
    y_off = torch.einsum(
        "bcqgn,bcgrnp->bcqgrp", Cm,
        prev_states.view(b, nc, g, rep, n, p).to(mm_dtype)).float() \
        .reshape(b, nc, chunk, h, p)
    y_off = y_off * state_decay.permute(0, 1, 3, 2).unsqueeze(-1)
    y = (y_diag + y_off).reshape(b, l, h, p)
    if return_final_state:
        final = torch.einsum("bhc,bchnp->bhnp", W[:, :, -1], states.float())
        return y, final.permute(0, 1, 3, 2).contiguous()
    return y


class Mamba2Mixer(nn.Module):
    def __init__(self, cfg: MambaConfig, layer_idx: int):
        super().__init__()
        self.d_model = cfg.d_model
        self.d_state = cfg.d_state
        self.d_conv = cfg.d_conv
        self.d_inner = cfg.expand * cfg.d_model
        self.headdim = cfg.headdim
        self.ngroups = cfg.ngroups
        self.nheads = self.d_inner // self.headdim
        self.chunk = cfg.chunk_size

        d_in_proj = 2 * self.d_inner + 2 * self.ngroups * self.d_state + self.nheads
        self.conv_dim = self.d_inner + 2 * self.ngroups * self.d_state
        self.in_proj = nn.Linear(self.d_model, d_in_proj, bias=False)
        self.conv_weight = nn.Parameter(
            torch.empty(self.conv_dim, self.d_conv))
        self.conv_bias = nn.Parameter(torch.zeros(self.conv_dim))
        self.dt_bias = nn.Parameter(torch.empty(self.nheads))
        self.A_log = nn.Parameter(torch.empty(self.nheads))
        self.D = nn.Parameter(torch.ones(self.nheads))
        self.norm = RMSNorm(self.d_inner, eps=1e-5)
        self.out_proj = nn.Linear(self.d_inner, self.d_model, bias=False)
        # wgrads land directly in the sharded runtime's flat grad buffer
        self.in_proj.weight._direct_wgrad = True
        self.out_proj.weight._direct_wgrad = True

    def reset_parameters(self):
        nn.init.trunc_normal_(self.in_proj.weight, std=0.02)
        nn.init.trunc_normal_(self.out_proj.weight, std=0.02)
        nn.init.uniform_(self.conv_weight, -(self.d_conv ** -0.5),
                         self.d_conv ** -0.5)
        nn.init.zeros_(self.conv_bias)
        # dt bias: softplus^-1 of dt ~ U(1e-3, 1e-1)  (mamba2 init)
        dt = torch.exp(torch.rand(self.nheads)
                       * (math.log(1e-1) - math.log(1e-3)) + math.log(1e-3))
        dt = dt.clamp(min=1e-4)
        with torch.no_grad():
            self.dt_bias.copy_(dt + torch.log(-torch.expm1(-dt)))
            # A in [1, 16)
            self.A_log.copy_(torch.log(
                torch.empty(self.nheads).uniform_(1, 16)))
        nn.init.ones_(self.D)
        self.norm.reset_parameters()

    def _scan_fused(self, b, l, x, dt, z, B, C, dtb, Alog, D_,
                    doc_start=None, doc_end=None, return_final_state=False):
        """GPU SSD scan: the elementwise chains run as fused HIP kernels
        (ops/hip/ssd.hip — prep/xdt/scores-decay/ygate, each with a
        custom backward); only the MFMA-shaped work (scores, y_diag,
        states, y_off einsums on hipBLASLt) and the tiny nc x nc
        inter-chunk recurrence stay as torch ops. Inputs x/dt/z/B/C are
        STRIDED slices of the fused projections — no contiguous copies.
        Returns the gated (b, l, d_inner) bf16 activations (pre-norm).
        doc_start/doc_end (a DocMask's arrays) reset the scan at every
        document start: masked xdt / scores-decay / ygate kernels plus a
        select on the inter-chunk matrix (see ssd_chunked).
        return_final_state: also the fp32 (b, h, p, n) state after the last
        token (see ssd_chunked)."""
        doc_mask = None if doc_start is None else ops.DocMask(doc_start,
                                                              doc_end)
        h, p = self.nheads, self.headdim
        g, n = self.ngroups, self.d_state
        Q = self.chunk
        nc = l // Q
        rep = h // g
        dt2 = dt.reshape(b * l, h)
        x2 = x.reshape(b * l, h * p)
        z2 = z.reshape(b * l, h * p)
        dtf, dacs = ops.ssd_prep(dt2, dtb, Alog, Q)        # (b*nc*h, Q) fp32
        # xdt/xdtd come out H-MAJOR (b,nc,h,Q,p): y_diag is then a plain
        # strided-batched bmm and no einsum materializes permuted copies
        xdt, xdtd = ops.ssd_xdt(x2, dtf, dacs, h, p, Q,    # bf16 pair
                                doc_mask=doc_mask)
        N = b * nc * h
        Bm = B.reshape(b, nc, Q, g, n)
        Cm = C.reshape(b, nc, Q, g, n)
        # scores per GROUP (g << h), decay folded in-kernel (L never
        # materialized; d_scores comes back from the fused backward)
        scores = torch.einsum("bcqgn,bckgn->bcgqk", Cm, Bm).contiguous()
        sL = ops.ssd_scores_decay(dacs, scores.view(b * nc * g, Q, Q), h, g,
                                  doc_mask=doc_mask)
        y_diag = torch.bmm(sL, xdt.view(N, Q, p))          # (N, Q, p) bf16
        # the whole inter-chunk state chain runs bf16 (W entries are
        # decays in [0,1], states are sums of bf16-rounded products with
        # fp32 GEMM accumulation) — halves the traffic of the biggest
        # remaining torch-side tensors. Only dacs' own chain stays fp32.
        states = torch.einsum(
            "bckgn,bcgrkp->bcgrnp", Bm,
            xdtd.view(b, nc, g, rep, Q, p)).reshape(b, nc, h, n, p)
        # inter-chunk recurrence in closed form (see ssd_chunked). The
        # one-chunk shift lives on the TINY (b,h,nc,nc) decay matrix
        # (zero first row) instead of a 167 MB cat on the states tensor.
        G = dacs.view(b, nc, h, Q)[..., -1].permute(0, 2, 1)
        W = torch.exp(segsum(G))
        if doc_start is not None:
            W = torch.where(doc_chunk_keep(doc_start, Q)[:, None], W,
                            torch.zeros_like(W))
        Wsh = torch.cat([torch.zeros_like(W[:, :, :1]), W[:, :, :-1]],
                        dim=2).to(torch.bfloat16)
        prev = torch.einsum("bhzc,bchnp->bzhnp", Wsh, states)
        # output ordering "bcgqrp" = the bmm-natural layout; the ygate
        # kernel reads it in place
        y_off = torch.einsum(
            "bcqgn,bcgrnp->bcgqrp", Cm,
            prev.view(b, nc, g, rep, n, p))
        out = ops.ssd_ygate(
            y_diag.reshape(b * l, h * p),
            y_off.contiguous().view(b * l, h * p),
            dacs, x2, D_, z2, h, g, p, Q, doc_mask=doc_mask)
        if return_final_state:
            final = torch.einsum("bhc,bchnp->bhnp", W[:, :, -1],
                                 states.float())
            return out.view(b, l, h * p), \
                final.permute(0, 1, 3, 2).contiguous()
        return out.view(b, l, h * p)

    def _fused_scan_ok(self, u):
        return u.is_cuda and u.dtype == torch.bfloat16 \
            and not getattr(self, "_force_torch_scan", False) \
            and os.environ.get("FMS_AMD_FORCE_TORCH_SCAN") != "1"

    def _forward_cached(self, u, cache):
        """l new tokens over an ops.MambaCache (inference only). in_proj
        and the conv run once over all l tokens. On a fresh cache the
        first l // chunk * chunk tokens take the chunked scan, which hands
        its final state to the cache; the remaining l % chunk tokens, and
        every token on a cache already in use (the single decode token as
        a rule), step the recurrence from the cached state with
        ops.ssd_state_update."""
        if torch.is_grad_enabled() and (
                u.requires_grad or self.in_proj.weight.requires_grad):
            raise RuntimeError(
                "the Mamba2 state cache has no backward: call the model "
                "under torch.no_grad()")
        b, l, _ = u.shape
        h, p, g, n = self.nheads, self.headdim, self.ngroups, self.d_state
        Q = self.chunk
        fresh = cache.len == 0
        zxbcdt = ops.linear_flat(u, self.in_proj.weight)
        z, xBC, dt = torch.split(
            zxbcdt, [self.d_inner, self.conv_dim, self.nheads], dim=-1)
        if fresh and l > 1:
            raw = xBC
            xBC = ops.causal_conv1d(raw, self.conv_weight, self.conv_bias)
            # the last W-1 raw rows; a shorter prompt keeps zeros in front
            k = min(l, self.d_conv - 1)
            cache.conv[:, self.d_conv - 1 - k:] = raw[:, l - k:]
        else:
            xBC = ops.causal_conv1d_update(cache.conv, xBC, self.conv_weight,
                                           self.conv_bias)
        x, B, C = torch.split(xBC, [self.d_inner, g * n, g * n], dim=-1)

        outs = []
        m = l // Q * Q if fresh else 0
        if m:
            xm, dtm, zm, Bm, Cm = (t[:, :m] for t in (x, dt, z, B, C))
            if self._fused_scan_ok(u):
                y, final = self._scan_fused(
                    b, m, xm, dtm, zm, Bm, Cm, self.dt_bias, self.A_log,
                    self.D, return_final_state=True)
            else:
                dtf = F.softplus(dtm.float() + self.dt_bias.float())
                xh = xm.reshape(b, m, h, p).float()
                y, final = ssd_chunked(
                    xh, dtf, -torch.exp(self.A_log.float()),
                    Bm.reshape(b, m, g, n).float(),
                    Cm.reshape(b, m, g, n).float(), Q,
                    return_final_state=True)
                y = y + xh * self.D.view(1, 1, -1, 1)
                y = y.reshape(b, m, self.d_inner).to(u.dtype) * F.silu(zm)
            cache.ssm.copy_(final)
            outs.append(y)
        if m < l:
            outs.append(ops.ssd_state_update(
                cache.ssm, x[:, m:], dt[:, m:], B[:, m:], C[:, m:], z[:, m:],
                self.dt_bias, self.A_log, self.D, h, g, p, n))
        cache.len += l
        y = outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
        return ops.linear_flat(self.norm(y), self.out_proj.weight)

    def forward(self, u, doc_mask=None, cache=None):
        """doc_mask (ops.DocMask): conv and SSM state restart at every
        document of a packed row. cache (ops.MambaCache): the tokens
        continue the cached sequence (_forward_cached); any length."""
        if cache is not None:
            if doc_mask is not None:
                raise ValueError("a state cache holds one sequence per row: "
                                 "cache and doc_mask do not combine")
            return self._forward_cached(u, cache)
        b, l, _ = u.shape
        zxbcdt = ops.linear_flat(u, self.in_proj.weight)
        z, xBC, dt = torch.split(
            zxbcdt, [self.d_inner, self.conv_dim, self.nheads], dim=-1)

        # causal depthwise conv + silu (fp32 math)
        xBC = ops.causal_conv1d(xBC, self.conv_weight, self.conv_bias,
                                doc_mask=doc_mask)
        # the mask's arrays are plain extra inputs of the checkpointed scan
        doc = () if doc_mask is None else (doc_mask.start, doc_mask.end)

        x, B, C = torch.split(
            xBC, [self.d_inner,
                  self.ngroups * self.d_state, self.ngroups * self.d_state],
            dim=-1)

        if u.is_cuda and u.dtype == torch.bfloat16 and l % self.chunk == 0 \
                and not getattr(self, "_force_torch_scan", False) \
                and os.environ.get("FMS_AMD_FORCE_TORCH_SCAN") != "1":
            args = (b, l, x, dt, z, B, C, self.dt_bias, self.A_log,
                    self.D) + doc
            if torch.is_grad_enabled() and self.training:
                y = torch.utils.checkpoint.checkpoint(
                    self._scan_fused, *args, use_reentrant=False)
            else:
                y = self._scan_fused(*args)
            y = self.norm(y)
            return ops.linear_flat(y, self.out_proj.weight)

        def _scan(x_, dt_, dtb, Alog, B_, C_, D_, doc_start=None,
                  doc_end=None):
            # fp32 SSD; recomputed in backward (the chunked intermediates
            # -- L, scores, states -- are large and cheap to rebuild)
            dtf = F.softplus(dt_.float() + dtb.float())
            A = -torch.exp(Alog.float())
            xh = x_.view(b, l, self.nheads, self.headdim).float()
            y_ = ssd_chunked(xh, dtf, A,
                             B_.view(b, l, self.ngroups, self.d_state).float(),
                             C_.view(b, l, self.ngroups, self.d_state).float(),
                             self.chunk, doc_start=doc_start)
            return y_ + xh * D_.view(1, 1, -1, 1)

        if torch.is_grad_enabled() and self.training:
            y = torch.utils.checkpoint.checkpoint(
                _scan, x, dt, self.dt_bias, self.A_log, B, C, self.D, *doc,
                use_reentrant=False)
        else:
            y = _scan(x, dt, self.dt_bias, self.A_log, B, C, self.D, *doc)
        y = y.reshape(b, l, self.d_inner).to(u.dtype)
        y = self.norm(y * F.silu(z))
        return ops.linear_flat(y, self.out_proj.weight)


class MambaAttnMixer(nn.Module):
    """Hybrid attention layer (mamba attn_cfg: causal MHA/GQA with partial
    rotary embedding of dim rotary_emb_dim)."""

    def __init__(self, cfg: MambaConfig, layer_idx: int):
        super().__init__()
        ac = cfg.attn_cfg
        self.nheads = ac.get("num_heads", 32)
        self.kvheads = ac.get("num_heads_kv", self.nheads)
        self.head_dim = ac.get("head_dim", cfg.d_model // self.nheads)
        self.rot_dim = ac.get("rotary_emb_dim", 0)
        qkv_out = (self.nheads + 2 * self.kvheads) * self.head_dim
        self.qkv = nn.Linear(cfg.d_model, qkv_out,
                             bias=ac.get("qkv_proj_bias", False))
        self.proj = nn.Linear(self.nheads * self.head_dim, cfg.d_model,
                              bias=ac.get("out_proj_bias", False))
        if self.rot_dim:
            self.rot_emb = RotaryEmbedding(self.rot_dim, 4096, 10000.0)
        if self.qkv.bias is None:
            self.qkv.weight._direct_wgrad = True
        if self.proj.bias is None:
            self.proj.weight._direct_wgrad = True

    def reset_parameters(self):
        nn.init.trunc_normal_(self.qkv.weight, std=0.02)
        nn.init.trunc_normal_(self.proj.weight, std=0.02)
        if self.qkv.bias is not None:
            nn.init.zeros_(self.qkv.bias)
        if self.proj.bias is not None:
            nn.init.zeros_(self.proj.bias)

    def forward(self, x, doc_mask=None, cache=None):
        """cache (ops.KVCache): the s tokens continue the cached sequence
        at positions [cache.len, cache.len + s)."""
        if cache is not None and doc_mask is not None:
            raise ValueError("a KV cache holds one sequence per row: cache "
                             "and doc_mask do not combine")
        b, s, _ = x.shape
        qkv = (self.qkv(x) if self.qkv.bias is not None
               else ops.linear_flat(x, self.qkv.weight))
        q, k, v = qkv.split(
            [self.nheads * self.head_dim, self.kvheads * self.head_dim,
             self.kvheads * self.head_dim], dim=-1)
        q = q.view(b, s, self.nheads, self.head_dim)
        k = k.view(b, s, self.kvheads, self.head_dim)
        v = v.view(b, s, self.kvheads, self.head_dim)
        if self.rot_dim:
            pos = 0 if cache is None else cache.len
            cos, sin = self.rot_emb.get(pos + s, x.device)
            if cache is not None:
                cos, sin = cos[pos:], sin[pos:]
            qr, kr = ops.rope_apply(q[..., :self.rot_dim].contiguous(),
                                    k[..., :self.rot_dim].contiguous(),
                                    cos, sin)
            q = torch.cat([qr, q[..., self.rot_dim:]], dim=-1)
            k = torch.cat([kr, k[..., self.rot_dim:]], dim=-1)
        if cache is not None:
            # q and k are rotated already: append only, no tables
            o = ops.attention_cached(q, k, v, cache)
        else:
            # rotary positions are not reset per document (as in Llama)
            o = ops.attention_causal(q.contiguous(), k.contiguous(),
                                     v.contiguous(), doc_mask=doc_mask)
        o2 = o.reshape(b, s, -1)
        if self.proj.bias is not None:
            return self.proj(o2)
        return ops.linear_flat(o2, self.proj.weight)


class GatedMLP(nn.Module):
    """d_intermediate MLP used between mixers when d_intermediate > 0."""

    def __init__(self, d_model, d_intermediate):
        super().__init__()
        self.wg1 = nn.Linear(d_model, 2 * d_intermediate, bias=False)
        self.w2 = nn.Linear(d_intermediate, d_model, bias=False)
        self.wg1.weight._direct_wgrad = True
        self.w2.weight._direct_wgrad = True

    def reset_parameters(self):
        nn.init.trunc_normal_(self.wg1.weight, std=0.02)
        nn.init.trunc_normal_(self.w2.weight, std=0.02)

    def forward(self, x):
        gu = ops.linear_flat(x, self.wg1.weight)
        return ops.linear_flat(ops.swiglu(gu), self.w2.weight)


class MambaBlock(nn.Module):
    """norm -> mixer (+ optional norm2 -> MLP), residual in fp32.
    The FSDP wrapping unit for the mamba path (reference wraps mamba_ssm
    Block, main_training_mamba.py:55)."""

    def __init__(self, cfg: MambaConfig, layer_idx: int):
        super().__init__()
        self.norm = RMSNorm(cfg.d_model, eps=1e-5)
        if layer_idx in cfg.attn_layer_idx:
            self.mixer = MambaAttnMixer(cfg, layer_idx)
        else:
            self.mixer = Mamba2Mixer(cfg, layer_idx)
        self.mlp = None
        if cfg.d_intermediate > 0:
            self.norm2 = RMSNorm(cfg.d_model, eps=1e-5)
            self.mlp = GatedMLP(cfg.d_model, cfg.d_intermediate)

    def reset_parameters(self):
        self.norm.reset_parameters()
        self.mixer.reset_parameters()
        if self.mlp is not None:
            self.norm2.reset_parameters()
            self.mlp.reset_parameters()

    def forward(self, x, doc_mask=None, cache=None):
        if cache is None and getattr(self, "_ac_enabled", False) \
                and torch.is_grad_enabled():
            return torch.utils.checkpoint.checkpoint(
                self._forward_impl, x, doc_mask, use_reentrant=False)
        return self._forward_impl(x, doc_mask, cache)

    def _forward_impl(self, x, doc_mask=None, cache=None):
        h = self.mixer(self.norm(x), doc_mask=doc_mask, cache=cache)
        if self.mlp is not None:
            # fused residual-add + norm (the reference's fused_add_norm,
            # config_utils.py:182 there)
            y2, s = ops.add_rmsnorm(x, h, self.norm2.weight, self.norm2.eps)
            return s + self.mlp(y2)
        return x + h


class MambaLMHeadModel(nn.Module):
    def __init__(self, cfg: MambaConfig):
        super().__init__()
        self.config = cfg
        self.embedding = nn.Embedding(cfg.vocab_size, cfg.d_model)
        self.layers = nn.ModuleList(
            [MambaBlock(cfg, i) for i in range(cfg.n_layer)])
        self.norm_f = RMSNorm(cfg.d_model, eps=1e-5)
        self.lm_head = nn.Linear(cfg.d_model, cfg.vocab_size, bias=False)
        if cfg.tie_embeddings:
            self.lm_head.weight = self.embedding.weight
        # token id that ends a packed document; when set, forward() keeps
        # conv, SSM state and attention inside each document (config knob
        # `doc_mask`)
        self.doc_mask_token = None

    def reset_parameters(self):
        nn.init.trunc_normal_(self.embedding.weight, std=0.02)
        if not self.config.tie_embeddings:
            nn.init.trunc_normal_(self.lm_head.weight, std=0.02)
        self.norm_f.reset_parameters()
        for l in self.layers:
            l.reset_parameters()

    def forward(self, tokens, labels=None, doc_mask=None, caches=None):
        """doc_mask (ops.DocMask) keeps every layer inside each document
        of a packed row: the causal conv and the SSM state restart at a
        document's first token and the hybrid's attention layers mask
        across documents. With `doc_mask_token` set it is built from
        `tokens`, once per forward, and shared by all layers.

        caches (allocate_cache()): `tokens` continue the sequence the
        caches hold, any number of them; inference only. A cached
        sequence is one document: an explicit doc_mask raises and
        `doc_mask_token` is not applied."""
        if caches is not None:
            if doc_mask is not None:
                raise ValueError("caches and doc_mask do not combine")
            if len(caches) != len(self.layers):
                raise ValueError(f"{len(self.layers)} layers need as many "
                                 f"caches, got {len(caches)}")
        elif doc_mask is None and self.doc_mask_token is not None:
            doc_mask = ops.doc_mask_from_tokens(tokens, self.doc_mask_token)
        x = self.embedding(tokens)
        if caches is not None:
            for layer, cache in zip(self.layers, caches):
                x = layer(x, cache=cache)
        else:
            for layer in self.layers:
                x = layer(x, doc_mask=doc_mask)
        x = self.norm_f(x)
        if labels is not None:
            return ops.linear_cross_entropy(x, self.lm_head.weight, labels)
        return self.lm_head(x)

    def allocate_cache(self, batch, max_len, dtype, device):
        """One cache per layer for a sequence of up to max_len tokens: an
        ops.MambaCache (constant size) for a Mamba2 layer, an ops.KVCache
        of max_len rows for an attention layer."""
        caches = []
        for layer in self.layers:
            mx = layer.mixer
            if isinstance(mx, MambaAttnMixer):
                caches.append(ops.KVCache(batch, max_len, mx.kvheads,
                                          mx.head_dim, dtype, device))
            else:
                caches.append(ops.MambaCache(
                    batch, mx.conv_dim, mx.d_conv, mx.nheads, mx.headdim,
                    mx.d_state, dtype, device))
        return caches

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens, temperature=1.0,
                 do_sample=True, include_embeds=False):
        """Autoregressive generation over the recurrent state (and the KV
        caches of a hybrid's attention layers): the prompt, of any length,
        is consumed in one forward, then one token per step at constant
        memory in the Mamba2 layers. Signature and return values of
        Llama.generate: tokens (b, s0 + max_new_tokens), with
        include_embeds also the final-norm hidden state of every
        generated position (b, max_new_tokens, d_model)."""
        b, s0 = input_ids.shape
        caches = None
        tokens = input_ids
        embeds = []
        cur = input_ids
        for _ in range(max_new_tokens):
            x = self.embedding(cur)
            if caches is None:
                caches = self.allocate_cache(b, s0 + max_new_tokens, x.dtype,
                                             x.device)
            for layer, cache in zip(self.layers, caches):
                x = layer(x, cache=cache)
            h_last = self.norm_f(x[:, -1:])
            logits = self.lm_head(h_last)[:, -1]
            if do_sample:
                probs = torch.softmax(logits.float() / temperature, dim=-1)
                nxt = torch.multinomial(probs, 1)
            else:
                nxt = logits.argmax(-1, keepdim=True)
            embeds.append(h_last)
            tokens = torch.cat([tokens, nxt], dim=1)
            cur = nxt
        if include_embeds:
            return tokens, torch.cat(embeds, dim=1)
        return tokens

    def param_count(self):
        return sum(p.numel() for p in self.parameters())
