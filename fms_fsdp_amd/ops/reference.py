"""Plain-PyTorch fp32 reference implementations of every hot op.

These are (a) the CPU execution path for the gloo-backed test suite and
(b) the numerics oracle the HIP kernels are validated against
("numerics tests compare against a plain PyTorch fp32
reference of the same op").
"""

import torch
import torch.nn.functional as F


def rmsnorm(x, weight, eps):
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (y * weight.float()).to(x.dtype)


def rope_apply(q, k, cos, sin):
    """q (b,s,h,d), k (b,s,kvh,d); cos/sin (s, d/2) fp32. Half-rotation
    (HF) convention: (x1, x2) -> (x1*cos - x2*sin, x2*cos + x1*sin) with
    x1 = x[..., :d/2], x2 = x[..., d/2:]."""
    def rot(t):
        tf = t.float()
        d2 = tf.shape[-1] // 2
        t1, t2 = tf[..., :d2], tf[..., d2:]
        c = cos.view(1, -1, 1, d2)
        s = sin.view(1, -1, 1, d2)
        return torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], dim=-1).to(t.dtype)
    return rot(q), rot(k)


def doc_mask_matrix(doc_start):
    """(b, s) first position of each token's document -> (b, s, s) bool,
    [b, i, j] = query i sees key j = doc_start[b, i] <= j <= i."""
    s = doc_start.shape[1]
    pos = torch.arange(s, device=doc_start.device)
    return ((pos[None, None, :] <= pos[None, :, None])
            & (pos[None, None, :] >= doc_start[:, :, None]))


def attention_causal(q, k, v, doc_mask=None):
    """q (b,s,h,d), k/v (b,s,kvh,d) -> (b,s,h,d). Causal, GQA broadcast.
    doc_mask (ops.DocMask): attention stays inside each document."""
    b, s, h, d = q.shape
    kvh = k.shape[2]
    qt = q.transpose(1, 2).float()
    kt = k.transpose(1, 2).float()
    vt = v.transpose(1, 2).float()
    if doc_mask is None:
        o = F.scaled_dot_product_attention(qt, kt, vt, is_causal=True,
                                           enable_gqa=(kvh != h))
    else:
        mask = doc_mask_matrix(doc_mask.start.to(q.device))[:, None]
        o = F.scaled_dot_product_attention(qt, kt, vt, attn_mask=mask,
                                           enable_gqa=(kvh != h))
    return o.transpose(1, 2).to(q.dtype)


def kv_cache_append(kcache, vcache, pos, q, k, v, cos=None, sin=None):
    """Rotate q and k by the tables of the positions being written (none:
    learned positions, nothing to rotate), store k and raw v in cache rows
    [pos, pos + s) in place and return q. Caches (b, capacity, kvh, d)."""
    if cos is not None:
        q, k = rope_apply(q, k, cos, sin)
    s = k.shape[1]
    kcache[:, pos:pos + s] = k
    vcache[:, pos:pos + s] = v
    return q


def attention_cached(q, k, v):
    """q (b,s,h,d) = the LAST s positions of the k/v (b,n,kvh,d) it attends
    to, n >= s: query i sees keys j <= n - s + i (causal, aligned bottom
    right). s == n is causal attention, s == 1 decode (no mask at all)."""
    b, s, h, d = q.shape
    n, kvh = k.shape[1], k.shape[2]
    qt = q.transpose(1, 2).float()
    kt = k.transpose(1, 2).float()
    vt = v.transpose(1, 2).float()
    if s == n:
        o = F.scaled_dot_product_attention(qt, kt, vt, is_causal=True,
                                           enable_gqa=(kvh != h))
    elif s == 1:
        o = F.scaled_dot_product_attention(qt, kt, vt, enable_gqa=(kvh != h))
    else:
        mask = torch.ones(s, n, dtype=torch.bool, device=q.device) \
            .tril(diagonal=n - s)
        o = F.scaled_dot_product_attention(qt, kt, vt, attn_mask=mask,
                                           enable_gqa=(kvh != h))
    return o.transpose(1, 2).to(q.dtype)


def attention_decode(q, kcache, vcache, kv_len):
    """q (b,1,h,d) against cache rows [0, kv_len); the newest key is
    already inside, so nothing is masked."""
    return attention_cached(q, kcache[:, :kv_len], vcache[:, :kv_len])


def swiglu(gu):
    """gu (..., 2H) fused gate|up -> silu(g) * u, (..., H)."""
    g, u = gu.float().chunk(2, dim=-1)
    return (F.silu(g) * u).to(gu.dtype)


def linear_cross_entropy(x, weight, labels, ignore_index=-100):
    """x (b,s,e), weight (V,e), labels (b,s) -> mean CE over non-ignored."""
    logits = F.linear(x.float(), weight.float())
    return F.cross_entropy(logits.view(-1, logits.shape[-1]), labels.view(-1),
                           ignore_index=ignore_index)


def causal_conv1d(x, weight, bias, doc_mask=None):
    """Depthwise causal conv + silu (mamba xBC conv). x (b, l, C),
    weight (C, W), bias (C). Computes in fp32, or in float64 when given
    float64. doc_mask (ops.DocMask): tap x[r] of output t counts iff
    r >= start[t], i.e. the conv restarts at every document."""
    b, l, C = x.shape
    W = weight.shape[1]
    if doc_mask is not None:
        # by definition the plain conv of every document's slice (the
        # library conv is not bit-stable across lengths, so nothing else
        # could equal that exactly). Reads the boundaries on the host: an
        # oracle and the CPU path, not a hot path.
        pos = torch.arange(l, device=doc_mask.start.device)
        rows = []
        for r in range(b):
            opens = pos[doc_mask.start[r] == pos].tolist()
            cuts = sorted(set([0] + opens)) + [l]
            rows.append(torch.cat(
                [causal_conv1d(x[r:r + 1, s:e], weight, bias)
                 for s, e in zip(cuts, cuts[1:])], dim=1))
        return torch.cat(rows, dim=0)
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    xt = x.transpose(1, 2).to(ct)
    y = F.conv1d(F.pad(xt, (W - 1, 0)), weight.to(ct).unsqueeze(1),
                 bias.to(ct), groups=C)
    return F.silu(y).transpose(1, 2).to(x.dtype)


# --------------------------------------------------------------------------
# Oracles of the four fused SSD pieces (ops/hip/ssd.hip), in the layouts
# and group mapping of Mamba2Mixer._scan_fused. They compute in the dtype
# they are given (float64 in the tests); backward comes from autograd.
# Row index of the (N, Q) tensors: n = bc*H + h with bc = b*nc + c.
#
# doc_mask (ops.DocMask of the (b, l) rows the chunks were cut from)
# resets the scan at every document start: position i depends on j iff
# start[i] <= j <= i. Over the chunked algorithm that is three selects to
# exact 0 (docs/kernels.md "Document mask"), all on the chunk-relative
# start of a token's document; the fourth, on the inter-chunk matrix,
# lives with the model (models/mamba.py doc_chunk_keep).
# --------------------------------------------------------------------------
def doc_rel_start(doc_mask, Q, device):
    """(bc, Q) int64: start of each token's document relative to the first
    position of its chunk; negative = it began in an earlier chunk."""
    start = doc_mask.start.to(device).long()
    b, l = start.shape
    first = torch.arange(l, device=device) // Q * Q
    return (start - first).reshape(b * (l // Q), Q)


def ssd_prep(dt2d, dt_bias, A_log, Q):
    """dt2d (b*l, H) -> dtf, dacs (N, Q): dtf = softplus(dt + bias),
    dacs = chunk-local cumsum of dtf * -exp(A_log)."""
    rows, H = dt2d.shape
    dtf = torch.logaddexp(dt2d + dt_bias, torch.zeros_like(dt2d))
    dtf = dtf.reshape(rows // Q, Q, H).transpose(1, 2)       # (bc, H, Q)
    dacs = (dtf * -torch.exp(A_log).view(1, H, 1)).cumsum(-1)
    return dtf.reshape(-1, Q), dacs.reshape(-1, Q)


def ssd_xdt(x2d, dtf, dacs, H, P, Q, doc_mask=None):
    """x2d (b*l, H*P) -> xdt = x*dtf and xdtd = xdt*exp(dacs_end - dacs),
    both h-major (bc, H, Q, P) flattened to (b*l, H*P). doc_mask: xdtd is
    0 before the start of the chunk's last document (only that document
    feeds the state the chunk hands on)."""
    rows = x2d.shape[0]
    bc = rows // Q
    xh = x2d.reshape(bc, Q, H, P).permute(0, 2, 1, 3)        # (bc, H, Q, P)
    cs = dacs.view(bc, H, Q)
    xdt = xh * dtf.view(bc, H, Q, 1)
    xdtd = xdt * torch.exp(cs[..., -1:] - cs).unsqueeze(-1)
    if doc_mask is not None:
        rel = doc_rel_start(doc_mask, Q, x2d.device)
        keep = torch.arange(Q, device=x2d.device) >= rel[:, -1:]   # (bc, Q)
        xdtd = torch.where(keep.view(bc, 1, Q, 1), xdtd,
                           torch.zeros_like(xdtd))
    return xdt.reshape(rows, H * P), xdtd.reshape(rows, H * P)


def ssd_scores_decay(dacs, scores3d, H, G, doc_mask=None):
    """sL[n, i, j] = scores[m, i, j] * exp(dacs[n, i] - dacs[n, j]) for
    j <= i, else 0; scores per group: m = bc*G + h // (H // G). doc_mask:
    additionally 0 where j lies before the start of i's document."""
    N, Q = dacs.shape
    rep = H // G
    diff = dacs[:, :, None] - dacs[:, None, :]
    mask = torch.tril(torch.ones(Q, Q, dtype=torch.bool, device=dacs.device))
    if doc_mask is not None:
        rel = doc_rel_start(doc_mask, Q, dacs.device)             # (bc, Q)
        inside = torch.arange(Q, device=dacs.device) >= rel[:, :, None]
        mask = (mask & inside).repeat_interleave(H, dim=0)        # (N, Q, Q)
    L = torch.exp(diff.masked_fill(~mask, -torch.inf))
    s = scores3d.view(N // H, G, 1, Q, Q).expand(-1, -1, rep, -1, -1)
    return s.reshape(N, Q, Q) * L


def ssd_ygate(ydiag, yoff, dacs, x2d, D, z2d, H, G, P, Q, doc_mask=None):
    """out = (ydiag + yoff*exp(dacs) + x*D) * silu(z), (b*l, H*P).
    ydiag h-major (bc, H, Q, P); yoff (bc, G, Q, rep, P). doc_mask: the
    yoff term counts only for tokens whose document began before their
    chunk."""
    rows = x2d.shape[0]
    bc = rows // Q
    rep = H // G
    yd = ydiag.reshape(bc, H, Q, P).permute(0, 2, 1, 3)      # (bc, Q, H, P)
    yo = yoff.reshape(bc, G, Q, rep, P).permute(0, 2, 1, 3, 4) \
        .reshape(bc, Q, H, P)
    if doc_mask is not None:
        off = doc_rel_start(doc_mask, Q, x2d.device) < 0          # (bc, Q)
        yo = torch.where(off.view(bc, Q, 1, 1), yo, torch.zeros_like(yo))
    sd = torch.exp(dacs.view(bc, H, Q)).permute(0, 2, 1).unsqueeze(-1)
    xh = x2d.reshape(bc, Q, H, P)
    zh = z2d.reshape(bc, Q, H, P)
    y = yd + yo * sd + xh * D.view(1, 1, H, 1)
    return (y * zh * torch.sigmoid(zh)).reshape(rows, H * P)


# --------------------------------------------------------------------------
# Recurrent decode (ops/hip/ssd_step.hip, cconv_update_kernel): the oracles
# of _C.ssd_step and _C.cconv_update, same signatures, states updated in
# place. float64 inputs compute in float64, everything else in fp32.
# --------------------------------------------------------------------------
def causal_conv1d_update(conv_state, x, weight, bias):
    """T new rows x (b, T, C) behind conv_state (b, W-1, C), the last W-1
    raw inputs, oldest first (zeros = a fresh sequence): returns
    silu(conv + bias) over [state | x] for the new rows and leaves the
    last W-1 rows of [state | x] in conv_state."""
    W = weight.shape[1]
    full = torch.cat([conv_state.to(x.dtype), x], dim=1)
    y = causal_conv1d(full, weight, bias)[:, W - 1:]
    conv_state.copy_(full[:, full.shape[1] - (W - 1):])
    return y


def ssd_state_update(state, x, dt, B, C, z, dt_bias, A_log, D, H, G, P, N):
    """The SSD recurrence over T >= 1 tokens from `state` (b, H, P, N),
    which ends as the state after the last token. x/z (b, T, H*P), B/C
    (b, T, G*N), dt (b, T, H) raw; dt_bias/A_log/D (H). Per token:
      dtf = softplus(dt + dt_bias); a = exp(dtf * -exp(A_log))
      s = a*s + (dtf*x) B^T; y = s C + D*x; out = y * silu(z)
    Returns out (b, T, H*P) in x's dtype."""
    b, T, _ = x.shape
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    rep = H // G
    xh = x.to(ct).reshape(b, T, H, P)
    zh = z.to(ct).reshape(b, T, H, P)
    Bh = B.to(ct).reshape(b, T, G, N).repeat_interleave(rep, dim=2)
    Ch = C.to(ct).reshape(b, T, G, N).repeat_interleave(rep, dim=2)
    xs = dt.to(ct) + dt_bias.to(ct)
    dtf = torch.logaddexp(xs, torch.zeros_like(xs))            # (b, T, H)
    a = torch.exp(dtf * -torch.exp(A_log.to(ct)))
    Dh = D.to(ct).view(1, H, 1)
    s = state.to(ct)
    ys = []
    for t in range(T):
        xdt = dtf[:, t, :, None] * xh[:, t]                    # (b, H, P)
        s = a[:, t, :, None, None] * s \
            + xdt[..., None] * Bh[:, t, :, None, :]
        ys.append((s * Ch[:, t, :, None, :]).sum(-1) + Dh * xh[:, t])
    state.copy_(s)
    y = torch.stack(ys, dim=1)                                 # (b, T, H, P)
    return (y * zh * torch.sigmoid(zh)).reshape(b, T, H * P).to(x.dtype)


def adamw_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    """In-place fp32 AdamW on flat tensors (the shard update)."""
    p.mul_(1 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v / bc2).sqrt_().add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
