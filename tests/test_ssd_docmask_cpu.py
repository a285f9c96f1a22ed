"""Document mask of the Mamba2 path on the CPU: the state and the conv
restart at every document start of a packed row.

The sequential float64 recurrence with a reset (written here) is the
ground truth. Against it: the torch path `ssd_chunked(..., doc_start)`,
and the masked float64 oracles of ops/reference.py composed exactly as
Mamba2Mixer._scan_fused composes the masked HIP kernels -- so the oracles
that judge those kernels on the GPU cannot be wrong in the kernels' own
way. Then the conv oracle against per-document slices, the inter-chunk
rule on its own, and the model (isolation of documents, mask source)."""

import pytest
import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.models.mamba import (MambaConfig, MambaLMHeadModel,
                                       doc_chunk_keep, segsum, ssd_chunked)
from fms_fsdp_amd.ops import reference

DD = torch.float64


def starts_to_doc_start(rows, l):
    """rows: per row the sorted first positions of its documents (0 first)
    -> (b, l) int64, start[b, i] = first position of i's document."""
    out = torch.zeros(len(rows), l, dtype=torch.int64)
    for r, starts in enumerate(rows):
        assert starts[0] == 0 and list(starts) == sorted(set(starts))
        for s in starts:
            out[r, s:] = s
    return out


def naive_ssd_reset(x, dt, A, B, C, doc_start):
    """S_t = a_t S_{t-1} + dt_t B_t (x) x_t, y_t = C_t . S_t with
    a_t = exp(dt_t A), and a_t := 0 wherever doc_start[t] == t."""
    b, l, h, p = x.shape
    g, n = B.shape[2], B.shape[3]
    rep = h // g
    Bh = B.repeat_interleave(rep, dim=2).double()
    Ch = C.repeat_interleave(rep, dim=2).double()
    S = torch.zeros(b, h, n, p, dtype=DD)
    ys = []
    for t in range(l):
        decay = torch.exp(dt[:, t].double() * A.double())           # (b, h)
        opens = (doc_start[:, t] == t)[:, None]
        decay = torch.where(opens, torch.zeros_like(decay), decay)
        S = decay[:, :, None, None] * S + torch.einsum(
            "bhn,bhp->bhnp", Bh[:, t] * dt[:, t, :, None].double(),
            x[:, t].double())
        ys.append(torch.einsum("bhn,bhnp->bhp", Ch[:, t], S))
    return torch.stack(ys, dim=1)


# ---------------------------------------------------------------------
# torch path against the recurrence
# ---------------------------------------------------------------------
@pytest.mark.parametrize("l,chunk", [(64, 16), (128, 32), (96, 96)])
def test_ssd_chunked_doc_matches_recurrence(l, chunk):
    torch.manual_seed(0)
    b, h, p, g, n = 3, 4, 8, 2, 16
    if 4 * chunk <= l:
        rows = [[0, 1, 2, chunk], [0, chunk + 5, 4 * chunk - 1], [0]]
    else:   # one chunk: everything is intra-chunk
        rows = [[0, 1, 2, 40], [0, 17, l - 1], [0]]
    doc_start = starts_to_doc_start(rows, l)
    x = torch.randn(b, l, h, p)
    dt = torch.rand(b, l, h) * 0.5
    A = -torch.rand(h) * 2
    B = torch.randn(b, l, g, n)
    C = torch.randn(b, l, g, n)
    y = ssd_chunked(x, dt, A, B, C, chunk, doc_start=doc_start)
    ref = naive_ssd_reset(x, dt, A, B, C, doc_start)
    err = (y - ref).abs().max() / ref.abs().max()
    assert err < 1e-4, err.item()
    # the mask matters: the unmasked scan is far from the reset recurrence
    y0 = ssd_chunked(x, dt, A, B, C, chunk)
    assert (y0 - ref).abs().max() / ref.abs().max() > 1e-2
    # row 2 is one document: the masked path changes nothing there
    assert torch.equal(y[2], y0[2])


# ---------------------------------------------------------------------
# masked oracles, composed as _scan_fused composes the kernels
# ---------------------------------------------------------------------
def scan_from_oracles_doc(b, l, x, dt, z, B, C, dtb, Alog, D_, h, p, g, n, Q,
                          doc_mask):
    nc = l // Q
    rep = h // g
    N = b * nc * h
    dt2 = dt.reshape(b * l, h)
    x2 = x.reshape(b * l, h * p)
    z2 = z.reshape(b * l, h * p)
    dtf, dacs = reference.ssd_prep(dt2, dtb, Alog, Q)
    xdt, xdtd = reference.ssd_xdt(x2, dtf, dacs, h, p, Q, doc_mask)
    Bm = B.reshape(b, nc, Q, g, n)
    Cm = C.reshape(b, nc, Q, g, n)
    scores = Cm.permute(0, 1, 3, 2, 4) @ Bm.permute(0, 1, 3, 4, 2)
    sL = reference.ssd_scores_decay(
        dacs, scores.reshape(b * nc * g, Q, Q), h, g, doc_mask)
    y_diag = sL @ xdt.view(N, Q, p)
    states = (Bm.permute(0, 1, 3, 4, 2).unsqueeze(3)
              @ xdtd.view(b, nc, g, rep, Q, p)).reshape(b, nc, h, n, p)
    G = dacs.view(b, nc, h, Q)[..., -1].permute(0, 2, 1)
    W = torch.exp(segsum(G))
    W = torch.where(doc_chunk_keep(doc_mask.start, Q)[:, None], W,
                    torch.zeros_like(W))
    Wsh = torch.cat([torch.zeros_like(W[:, :, :1]), W[:, :, :-1]], dim=2)
    prev = (Wsh @ states.permute(0, 2, 1, 3, 4).reshape(b, h, nc, n * p)) \
        .view(b, h, nc, n, p).permute(0, 2, 1, 3, 4)
    pv = prev.reshape(b, nc, g, rep, n, p).permute(0, 1, 2, 4, 3, 5) \
        .reshape(b, nc, g, n, rep * p)
    y_off = Cm.permute(0, 1, 3, 2, 4) @ pv          # (b, nc, g, Q, rep*p)
    out = reference.ssd_ygate(
        y_diag.reshape(b * l, h * p), y_off.reshape(b * l, h * p), dacs,
        x2, D_, z2, h, g, p, Q, doc_mask)
    return out.view(b, l, h * p)


@pytest.mark.parametrize("Q,h,g,p", [(64, 6, 2, 8), (16, 4, 4, 8),
                                     (32, 4, 1, 16)])
def test_masked_oracles_compose_to_recurrence(Q, h, g, p):
    torch.manual_seed(0)
    b, n, nc = 3, 16, 5
    l = nc * Q
    doc_start = starts_to_doc_start(
        [[0, 1, 2, Q], [0, Q + 5, 4 * Q - 1], [0]], l)
    doc_mask = ops.doc_mask_from_starts(doc_start)

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, dtype=DD) * scale).requires_grad_()

    x, z = leaf(b, l, h * p), leaf(b, l, h * p)
    dt = leaf(b, l, h, scale=2.0)
    B, C = leaf(b, l, g * n), leaf(b, l, g * n)
    dtb = leaf(h)
    # |A| from 0.02 to 4: the slow heads would carry state across all the
    # chunks (and across every boundary, were it not reset)
    Alog = torch.linspace(-4.0, 1.4, h, dtype=DD).requires_grad_()
    D_ = leaf(h)
    leaves = (x, dt, z, B, C, dtb, Alog, D_)
    names = ("x", "dt", "z", "B", "C", "dt_bias", "A_log", "D")

    out = scan_from_oracles_doc(b, l, x, dt, z, B, C, dtb, Alog, D_,
                                h, p, g, n, Q, doc_mask)

    xh = x.view(b, l, h, p)
    dtf = torch.nn.functional.softplus(dt + dtb, threshold=1e9)
    y = naive_ssd_reset(xh, dtf, -torch.exp(Alog), B.view(b, l, g, n),
                        C.view(b, l, g, n), doc_start)
    assert y.dtype == DD
    y = y + xh * D_.view(1, 1, h, 1)
    ref = y.reshape(b, l, h * p) * torch.nn.functional.silu(z)

    torch.testing.assert_close(out, ref, rtol=1e-9, atol=1e-12)
    cot = torch.randn_like(ref)
    got_g = torch.autograd.grad(out, leaves, cot)
    ref_g = torch.autograd.grad(ref, leaves, cot)
    for nm, a, r in zip(names, got_g, ref_g):
        torch.testing.assert_close(a, r, rtol=1e-9, atol=1e-12,
                                   msg=lambda m, nm=nm: f"d{nm}: {m}")
    # and the mask is not a no-op at this tolerance
    with torch.no_grad():
        one = ops.doc_mask_from_starts(torch.zeros_like(doc_start))
        out1 = scan_from_oracles_doc(b, l, x, dt, z, B, C, dtb, Alog, D_,
                                     h, p, g, n, Q, one)
        assert (out1[:2] - ref[:2]).abs().max() > 1e-3
        torch.testing.assert_close(out1[2], ref[2], rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------
# conv oracle: exactly the unmasked conv of every document's slice
# ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, DD])
@pytest.mark.parametrize("W", [2, 3, 4])
def test_conv_oracle_equals_slices(W, dtype):
    torch.manual_seed(W)
    L, C = 100, 24
    rows = [[0, 1, 2, 7, 8, 9, 50, 99], [0]]
    doc_start = starts_to_doc_start(rows, L)
    x = torch.randn(2, L, C, dtype=dtype)
    w = torch.randn(C, W, dtype=dtype)
    bias = torch.randn(C, dtype=dtype)
    y = reference.causal_conv1d(x, w, bias, ops.doc_mask_from_starts(doc_start))
    assert y.dtype == dtype
    for r, starts in enumerate(rows):
        for s, e in zip(starts, starts[1:] + [L]):
            ys = reference.causal_conv1d(x[r:r + 1, s:e], w, bias)
            assert torch.equal(y[r:r + 1, s:e], ys), (r, s, e)
    # no mask: today's bits
    assert torch.equal(reference.causal_conv1d(x, w, bias)[1], y[1])
    # the rule itself, tap by tap: x[r] counts for output t iff
    # r >= start[t] (r = t - (W-1) + wi)
    z = bias.double().expand(2, L, C).clone()
    t = torch.arange(L)
    for wi in range(W):
        r = t - (W - 1) + wi
        ok = (r[None, :] >= doc_start) & (r[None, :] >= 0)
        tap = x.double()[:, r.clamp(min=0)] * w.double()[:, wi]
        z += torch.where(ok[..., None], tap, torch.zeros_like(tap))
    torch.testing.assert_close(y.double(), z * torch.sigmoid(z),
                               rtol=1e-5 if dtype == torch.float32 else 1e-12,
                               atol=1e-5 if dtype == torch.float32 else 1e-12)


# ---------------------------------------------------------------------
# the inter-chunk rule
# ---------------------------------------------------------------------
def test_chunk_keep_rule_brute_force():
    Q, nc = 8, 6
    l = Q * nc
    rows = [[0, 1, 2, Q], [0, Q + 5, 4 * Q - 1], [0], [0, 3 * Q],
            [0, 2 * Q - 1, 2 * Q, 5 * Q + 3]]
    doc_start = starts_to_doc_start(rows, l)
    keep = doc_chunk_keep(doc_start, Q)
    assert keep.shape == (len(rows), nc, nc) and keep.dtype == torch.bool
    for r in range(len(rows)):
        for z in range(nc):
            for c in range(z + 1):
                # positions from the last token of chunk c to the last
                # token of chunk z all lie in one document
                lo, hi = (c + 1) * Q - 1, (z + 1) * Q - 1
                same = len({int(doc_start[r, t]) for t in range(lo, hi + 1)}) == 1
                assert bool(keep[r, z, c]) == same, (r, z, c)


# ---------------------------------------------------------------------
# model
# ---------------------------------------------------------------------
EOS = 5


def hybrid_cfg():
    return MambaConfig(
        d_model=32, n_layer=3, vocab_size=64, d_state=16, headdim=8,
        chunk_size=16, attn_layer_idx=[1], d_intermediate=48,
        attn_cfg={"num_heads": 2, "num_heads_kv": 1, "head_dim": 16,
                  "rotary_emb_dim": 8})


def packed_tokens(seed, cut):
    """(2, 64) tokens without EOS except at cut-1 of row 0 and 40 of row 1."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(EOS + 1, 64, (2, 64), generator=g)
    t[0, cut - 1] = EOS
    t[1, 40] = EOS
    return t


@pytest.mark.parametrize("cut", [16, 23])   # on a chunk start, mid-chunk
def test_model_documents_are_isolated(cut):
    torch.manual_seed(0)
    m = MambaLMHeadModel(hybrid_cfg()).eval()
    m.reset_parameters()
    assert any(hasattr(b.mixer, "qkv") for b in m.layers) and \
        m.layers[0].mlp is not None
    tok = packed_tokens(1, cut)
    other = tok.clone()
    other[0, :cut - 1] = packed_tokens(2, cut)[0, :cut - 1]
    assert not torch.equal(tok[0, :cut - 1], other[0, :cut - 1])
    with torch.no_grad():
        m.doc_mask_token = EOS
        a, b_ = m(tok), m(other)
        assert torch.equal(a[0, cut:], b_[0, cut:])
        assert torch.equal(a[1], b_[1])
        assert not torch.equal(a[0, :cut], b_[0, :cut])
        m.doc_mask_token = None
        a0, b0 = m(tok), m(other)
        assert (a0[0, cut:] - b0[0, cut:]).abs().max() > 1e-4
        # and the mask changes what the second document computes
        assert (a0[0, cut:] - a[0, cut:]).abs().max() > 1e-4


def test_model_mask_source_and_backward():
    torch.manual_seed(0)
    m = MambaLMHeadModel(hybrid_cfg())
    m.reset_parameters()
    tok = packed_tokens(3, 23)
    explicit = m(tok, doc_mask=ops.doc_mask_from_tokens(tok, EOS))
    plain = m(tok)
    m.doc_mask_token = EOS
    built = m(tok)
    assert torch.equal(built, explicit)
    assert not torch.equal(built, plain)
    # training mode goes through the checkpointed scan with the mask's
    # arrays as extra inputs
    m.train()
    loss = m(tok, labels=tok)
    loss.backward()
    for n_, p_ in m.named_parameters():
        assert p_.grad is not None and torch.isfinite(p_.grad).all(), n_


def test_entry_point_sets_doc_mask_token():
    import inspect
    import main_training_mamba
    src = inspect.getsource(main_training_mamba)
    assert "doc_mask_token = cfg.eos_token" in src
