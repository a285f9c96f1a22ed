"""The document-masked (`_doc`) SSD and conv kernels.

Every masked output, forward and backward, is held elementwise to the
masked float64 oracle of ops/reference.py (tied to the recurrence with
reset by test_ssd_docmask_cpu.py) under tests/oracle_rule.py, with the R,
A and widened terms test_ssd_kernels_gpu.py / test_ops_edges_gpu.py use
for the unmasked kernel; a masked summand simply leaves the sum behind
`mag`, so where the mask makes the oracle 0 the rule demands exact 0.
Beside the rule: one document per row reproduces the unmasked kernel's
bits, boundaries on chunk starts (conv: any boundaries, against the
document's slice) do so too, and overwriting the first document never
moves a bit of a later one."""

import pytest
import torch
import torch.nn.functional as F

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_ssd_kernels_gpu import col_slice, dev, ext, make_dacs, randn

pytestmark = pytest.mark.gpu

DD = torch.float64
A_RED, A_CH = rule.A_REDUCE, rule.A_CHAIN
B, NC = 3, 5
BC = B * NC


def ssd_rows(Q):
    """Row 0: two one-token documents, a boundary on a chunk start and one
    document over four whole chunks. Row 1: a document from mid-chunk
    across two whole chunks that ends on a chunk's last token, then one
    that starts there. Row 2: one document."""
    return [[0, 1, 2, Q], [0, Q + 5, 4 * Q - 1], [0]]


def mask_of(rows, l):
    start = torch.zeros(len(rows), l, dtype=torch.int64)
    for r, starts in enumerate(rows):
        for s in starts:
            start[r, s:] = s
    return ops.doc_mask_from_starts(start.to(dev()))


def later_positions(rows, l):
    """(b*l) bool: flat positions outside the first document of their row."""
    later = torch.zeros(len(rows), l, dtype=torch.bool)
    for r, starts in enumerate(rows):
        if len(starts) > 1:
            later[r, starts[1]:] = True
    return later.reshape(-1).to(dev())


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def other_where(t, sel, seed):
    """Copy of t with the selected elements replaced by other finite values."""
    g = torch.Generator(device=t.device).manual_seed(seed)
    noise = (torch.randn(t.shape, device=t.device, generator=g) * 3).to(t.dtype)
    return torch.where(sel, noise, t)


# layouts -> flat position first
def pos_hmajor(t, H, Q, P):          # (rows, H*P) holding (bc, H, Q, P)
    return t.view(-1, H, Q, P).permute(0, 2, 1, 3).reshape(-1, H, P)


def pos_nq(t, H, Q):                 # (N, Q), n = bc*H + h
    return t.view(-1, H, Q).permute(0, 2, 1).reshape(-1, H)


def pos_yoff(t, G, Q, rep, P):       # (rows, H*P) holding (bc, G, Q, rep, P)
    return t.view(-1, G, Q, rep, P).permute(0, 2, 1, 3, 4).reshape(-1, G * rep, P)


# ... and back: a (rows,) selection of flat positions as a bool tensor in
# the layout
def sel_rows(pos_sel, HP):
    return pos_sel[:, None].expand(-1, HP)


def sel_hmajor(pos_sel, H, Q, P):
    return pos_sel.view(-1, 1, Q, 1).expand(-1, H, Q, P).reshape(-1, H * P)


def sel_yoff(pos_sel, G, Q, rep, P):
    return pos_sel.view(-1, 1, Q, 1, 1).expand(-1, G, Q, rep, P) \
        .reshape(-1, G * rep * P)


def rel_start(dm, Q):
    return reference.doc_rel_start(dm, Q, dev())          # (bc, Q)


# ---------------------------------------------------------------------
# xdt
# ---------------------------------------------------------------------
@pytest.mark.parametrize("Q", [64, 128])
@pytest.mark.parametrize("P", [8, 64])
def test_ssd_xdt_doc(P, Q):
    torch.manual_seed(P * 1000 + Q)
    H = 4
    l = NC * Q
    rows, N = BC * Q, BC * H
    dm = mask_of(ssd_rows(Q), l)
    x = col_slice(rows, H * P)
    dtf = (torch.rand(N, Q, device=dev()) * 2).float()
    dacs = make_dacs(N, Q)
    g1, g2 = randn(rows, H * P), randn(rows, H * P)
    tag = f"[P={P},Q={Q}]"
    C = ext()

    xdt, xdtd = C.ssd_xdt_fwd_doc(x, dtf, dacs, H, P, Q, dm.start, l)
    x64 = x.double().requires_grad_()
    f64 = dtf.double().requires_grad_()
    c64 = dacs.double().requires_grad_()
    xdt_r, xdtd_r = reference.ssd_xdt(x64, f64, c64, H, P, Q, dm)
    keep = (torch.arange(Q, device=dev()) >= rel_start(dm, Q)[:, -1:])  # (bc,Q)
    assert not keep.all() and keep.any()
    rule.check("ssd_xdt_fwd_doc.xdt" + tag, xdt, xdt_r, xdt_r.abs(), A_CH)
    rule.check("ssd_xdt_fwd_doc.xdtd" + tag, xdtd, xdtd_r, xdtd_r.abs(), A_CH)
    assert (bits(pos_hmajor(xdtd, H, Q, P))[~keep.reshape(-1)] == 0).all()

    dx, ddtf, sdec = C.ssd_xdt_bwd_doc(g1, g2, x, dtf, dacs, H, P, Q,
                                       dm.start, l)
    dx_r, ddtf_r, ddacs_r = torch.autograd.grad(
        (xdt_r, xdtd_r), (x64, f64, c64), (g1.double(), g2.double()))
    with torch.no_grad():
        k4 = keep.view(BC, 1, Q, 1).double()
        a1 = g1.double().abs().view(BC, H, Q, P)
        a2 = g2.double().abs().view(BC, H, Q, P) * k4
        xh = x.double().view(BC, Q, H, P).permute(0, 2, 1, 3)
        f = f64.view(BC, H, Q, 1)
        cs = c64.view(BC, H, Q)
        dec = torch.exp(cs[..., -1:] - cs).unsqueeze(-1)
        m_dx = ((a1 + a2 * dec) * f).permute(0, 2, 1, 3).reshape(rows, H * P)
        m_ddtf = ((a1 + a2 * dec) * xh.abs()).sum(-1).view(N, Q)
        s_terms = g2.double().view(BC, H, Q, P) * k4 * xh * f * dec
        sdec_r = s_terms.sum(-1).view(N, Q)
        m_sdec = s_terms.abs().sum(-1).view(N, Q)
        m_ddacs = m_sdec.clone()
        m_ddacs[:, -1] += m_sdec.sum(-1)
    rule.check("ssd_xdt_bwd_doc.dx" + tag, dx, dx_r, m_dx, A_CH)
    rule.check("ssd_xdt_bwd_doc.ddtf" + tag, ddtf, ddtf_r, m_ddtf, A_RED)
    rule.check("ssd_xdt_bwd_doc.sdec" + tag, sdec, sdec_r, m_sdec, A_RED)

    dacs_w = dacs.clone().requires_grad_()
    o1, o2 = ops.ssd_xdt(x, dtf, dacs_w, H, P, Q, doc_mask=dm)
    assert same_bits(o1, xdt) and same_bits(o2, xdtd)
    (ddacs,) = torch.autograd.grad((o1, o2), dacs_w, (g1, g2))
    rule.check("ssd_xdt doc wrapper.ddacs" + tag, ddacs, ddacs_r, m_ddacs,
               A_RED)

    # one document per row: the unmasked kernel's bits
    one = mask_of([[0]] * B, l)
    for a, b_ in zip(C.ssd_xdt_fwd_doc(x, dtf, dacs, H, P, Q, one.start, l)
                     + C.ssd_xdt_bwd_doc(g1, g2, x, dtf, dacs, H, P, Q,
                                         one.start, l),
                     C.ssd_xdt_fwd(x, dtf, dacs, H, P, Q)
                     + C.ssd_xdt_bwd(g1, g2, x, dtf, dacs, H, P, Q)):
        assert same_bits(a, b_)

    # isolation: other values in every row's first document
    later = later_positions(ssd_rows(Q), l)
    first_h = sel_hmajor(~later, H, Q, P)
    x2 = other_where(x, sel_rows(~later, H * P), 1)
    g1b, g2b = other_where(g1, first_h, 2), other_where(g2, first_h, 3)
    xdt2, xdtd2 = C.ssd_xdt_fwd_doc(x2, dtf, dacs, H, P, Q, dm.start, l)
    dx2, ddtf2, sdec2 = C.ssd_xdt_bwd_doc(g1b, g2b, x2, dtf, dacs, H, P, Q,
                                          dm.start, l)
    assert not same_bits(xdt2, xdt)
    for a, b_ in ((xdt, xdt2), (xdtd, xdtd2)):
        assert same_bits(pos_hmajor(a, H, Q, P)[later],
                         pos_hmajor(b_, H, Q, P)[later])
    assert same_bits(dx[later], dx2[later])
    assert same_bits(pos_nq(ddtf, H, Q)[later], pos_nq(ddtf2, H, Q)[later])
    assert same_bits(pos_nq(sdec, H, Q)[later], pos_nq(sdec2, H, Q)[later])


# ---------------------------------------------------------------------
# scores * decay
# ---------------------------------------------------------------------
def _sl_case(Q, H, G, seed):
    torch.manual_seed(seed)
    N, M = BC * H, BC * G
    return make_dacs(N, Q), randn(M, Q, Q, scale=2.0), randn(N, Q, Q)


@pytest.mark.parametrize("H,G", [(4, 1), (6, 2)])
@pytest.mark.parametrize("Q", [64, 128])
def test_ssd_sl_doc(Q, H, G):
    N, M, rep = BC * H, BC * G, H // G
    l = NC * Q
    dm = mask_of(ssd_rows(Q), l)
    dacs, scores, g = _sl_case(Q, H, G, Q * 10 + H + G)
    tag = f"[Q={Q},H={H},G={G}]"
    C = ext()

    sL = C.ssd_sl_fwd_doc(dacs, scores, H, G, dm.start, l)
    c64 = dacs.double().requires_grad_()
    s64 = scores.double().requires_grad_()
    sL_r = reference.ssd_scores_decay(c64, s64, H, G, dm)
    rule.check("ssd_sl_fwd_doc.sL" + tag, sL, sL_r, sL_r.abs(), A_CH)
    qq = torch.arange(Q, device=dev())
    lower = qq[None, :] <= qq[:, None]
    inside = qq[None, None, :] >= rel_start(dm, Q)[:, :, None]      # (bc,Q,Q)
    kept = (inside & lower).repeat_interleave(H, dim=0)             # (N,Q,Q)
    cut = (~inside & lower).repeat_interleave(H, dim=0)
    assert cut.any()
    assert (bits(sL)[~kept] == 0).all(), "masked sL is not +0"

    dsh, dcs = C.ssd_sl_bwd_doc(g, scores, dacs, H, G, dm.start, l)
    dcs_r, dsc_r = torch.autograd.grad(sL_r, (c64, s64), g.double())
    with torch.no_grad():
        L = reference.ssd_scores_decay(
            c64, torch.ones(M, Q, Q, dtype=DD, device=dev()), H, G, dm)
        dsh_r = g.double() * L
        prod = (g.double() * sL_r).abs()
        m_dcs = prod.sum(2) + prod.sum(1)
    rule.check("ssd_sl_bwd_doc.dsh" + tag, dsh, dsh_r, dsh_r.abs(), A_CH)
    assert (bits(dsh)[cut] == 0).all(), "masked dsh is not +0"
    assert (dsh[~kept] == 0).all()
    rule.check("ssd_sl_bwd_doc.dcs" + tag, dcs, dcs_r, m_dcs, A_RED)

    dacs_w = dacs.clone().requires_grad_()
    sc_w = scores.clone().requires_grad_()
    out = ops.ssd_scores_decay(dacs_w, sc_w, H, G, doc_mask=dm)
    assert same_bits(out, sL)
    dcs_w, dsc_w = torch.autograd.grad(out, (dacs_w, sc_w), g)
    assert same_bits(dcs_w, dcs)
    with torch.no_grad():
        m_dsc = dsh_r.abs().view(BC, G, rep, Q, Q).sum(2).view(M, Q, Q)
        if rep > 1:   # bf16 per-head summands, as in the unmasked test
            m_dsc = rule.widen(m_dsc, 2.0 ** -8 * m_dsc, A_RED)
    rule.check("ssd_scores_decay doc wrapper.dscores" + tag, dsc_w, dsc_r,
               m_dsc, A_RED)

    # isolation: other scores / g wherever the row or the column of the
    # entry lies in the first document
    later = later_positions(ssd_rows(Q), l).view(BC, Q)
    touch = ~(later[:, :, None] & later[:, None, :])                # (bc,Q,Q)
    sc2 = other_where(scores, touch.repeat_interleave(G, dim=0), 5)
    g2 = other_where(g, touch.repeat_interleave(H, dim=0), 6)
    sL2 = C.ssd_sl_fwd_doc(dacs, sc2, H, G, dm.start, l)
    dsh2, dcs2 = C.ssd_sl_bwd_doc(g2, sc2, dacs, H, G, dm.start, l)
    lat_n = later.repeat_interleave(H, dim=0)                       # (N,Q)
    assert not same_bits(sL2, sL)
    assert same_bits(sL[lat_n], sL2[lat_n])
    assert same_bits(dsh[lat_n], dsh2[lat_n])
    assert same_bits(dcs[lat_n], dcs2[lat_n])


@pytest.mark.parametrize("Q", [64, 128])
def test_ssd_sl_doc_unmasked_bits(Q):
    """One document per row, and boundaries on chunk starts only: nothing
    inside a chunk is masked, so every bit is the unmasked kernel's."""
    H, G = 6, 2
    l = NC * Q
    dacs, scores, g = _sl_case(Q, H, G, Q + 77)
    C = ext()
    ref = (C.ssd_sl_fwd(dacs, scores, H, G),) + C.ssd_sl_bwd(g, scores, dacs,
                                                             H, G)
    for rows in ([[0]] * B, [[0, Q, 3 * Q], [0, 2 * Q], [0, 4 * Q]]):
        dm = mask_of(rows, l)
        got = (C.ssd_sl_fwd_doc(dacs, scores, H, G, dm.start, l),) \
            + C.ssd_sl_bwd_doc(g, scores, dacs, H, G, dm.start, l)
        for a, b_ in zip(got, ref):
            assert same_bits(a, b_)


# ---------------------------------------------------------------------
# ygate
# ---------------------------------------------------------------------
def _ygate_case(P, Q, H, seed):
    torch.manual_seed(seed)
    rows, N, HP = BC * Q, BC * H, H * P
    fused = randn(rows, 2 * HP + 40)
    z, x = fused[:, 8:8 + HP], fused[:, 16 + HP:16 + 2 * HP]
    ydiag, yoff = randn(rows, HP), randn(rows, HP)
    dacs = make_dacs(N, Q)
    dacs[::2] *= 0.01      # slow rows: exp(dacs) keeps the yoff term visible
    D = randn(H, dtype=torch.float32)
    return ydiag, yoff, dacs, x, D, z, randn(rows, HP)


@pytest.mark.parametrize("H,G", [(4, 1), (6, 2)])
@pytest.mark.parametrize("Q", [64, 128])
@pytest.mark.parametrize("P", [8, 64])
def test_ssd_ygate_doc(P, Q, H, G):
    rep = H // G
    l = NC * Q
    rows, N, HP = BC * Q, BC * H, H * P
    dm = mask_of(ssd_rows(Q), l)
    ydiag, yoff, dacs, x, D, z, dout = _ygate_case(P, Q, H, P * 1000 + Q + H)
    tag = f"[P={P},Q={Q},H={H},G={G}]"
    C = ext()
    off = rel_start(dm, Q) < 0                                      # (bc, Q)
    assert off.any() and not off.all()

    out = C.ssd_ygate_fwd_doc(ydiag, yoff, dacs, x, D, z, H, G, P, Q,
                              dm.start, l)
    leaves = [t.double().requires_grad_()
              for t in (ydiag, yoff, dacs, x, D, z)]
    yd64, yo64, c64, x64, D64, z64 = leaves
    out_r = reference.ssd_ygate(yd64, yo64, c64, x64, D64, z64, H, G, P, Q,
                                dm)
    with torch.no_grad():
        o4 = off.view(BC, Q, 1, 1).double()
        ydq = yd64.view(BC, H, Q, P).permute(0, 2, 1, 3)
        yoq = yo64.view(BC, G, Q, rep, P).permute(0, 2, 1, 3, 4) \
            .reshape(BC, Q, H, P) * o4
        sd = torch.exp(c64.view(BC, H, Q)).permute(0, 2, 1).unsqueeze(-1)
        xq = x64.view(BC, Q, H, P)
        zq = z64.view(BC, Q, H, P)
        Dq = D64.view(1, 1, H, 1)
        sg = torch.sigmoid(zq)
        m_y = ydq.abs() + yoq.abs() * sd + xq.abs() * Dq.abs()
        m_out = (m_y * (zq * sg).abs()).reshape(rows, HP)
    rule.check("ssd_ygate_fwd_doc.out" + tag, out, out_r, m_out, A_CH)

    got = C.ssd_ygate_bwd_doc(dout, ydiag, yoff, dacs, x, D, z, H, G, P, Q,
                              dm.start, l)
    dydiag, dyoff, ddacs, dx, dD_rows, dz = got
    dyd_r, dyo_r, dc_r, dx_r, dD_r, dz_r = torch.autograd.grad(
        out_r, leaves, dout.double())
    with torch.no_grad():
        gy = dout.double().view(BC, Q, H, P)
        dy = gy * zq * sg
        dDrows_r = (dy * xq).sum(-1).reshape(rows, H)
        m_dDrows = (dy * xq).abs().sum(-1).reshape(rows, H)
        m_dD = m_dDrows.sum(0)
        m_ddacs = (dy * yoq * sd).abs().sum(-1).permute(0, 2, 1).reshape(N, Q)
        m_dz = (gy.abs() * m_y * sg * (1 + zq.abs() * (1 - sg))) \
            .reshape(rows, HP)
    rule.check("ssd_ygate_bwd_doc.dydiag" + tag, dydiag, dyd_r, dyd_r.abs(),
               A_CH)
    rule.check("ssd_ygate_bwd_doc.dyoff" + tag, dyoff, dyo_r, dyo_r.abs(),
               A_CH)
    assert (bits(pos_yoff(dyoff, G, Q, rep, P))[~off.reshape(-1)] == 0).all()
    rule.check("ssd_ygate_bwd_doc.dx" + tag, dx, dx_r, dx_r.abs(), A_CH)
    rule.check("ssd_ygate_bwd_doc.dz" + tag, dz, dz_r, m_dz, A_CH)
    rule.check("ssd_ygate_bwd_doc.ddacs" + tag, ddacs, dc_r, m_ddacs, A_RED)
    rule.check("ssd_ygate_bwd_doc.dD_rows" + tag, dD_rows, dDrows_r, m_dDrows,
               A_RED)

    D_w = D.clone().requires_grad_()
    o = ops.ssd_ygate(ydiag, yoff, dacs, x, D_w, z, H, G, P, Q, doc_mask=dm)
    assert same_bits(o, out)
    (dD,) = torch.autograd.grad(o, D_w, dout)
    rule.check("ssd_ygate doc wrapper.dD" + tag, dD, dD_r, m_dD, A_RED)

    # isolation: other values at every position of the first documents
    later = later_positions(ssd_rows(Q), l)
    fr = sel_rows(~later, HP)
    yd2 = other_where(ydiag, sel_hmajor(~later, H, Q, P), 11)
    yo2 = other_where(yoff, sel_yoff(~later, G, Q, rep, P), 12)
    x2, z2 = other_where(x, fr, 13), other_where(z, fr, 14)
    do2 = other_where(dout, fr, 15)
    out2 = C.ssd_ygate_fwd_doc(yd2, yo2, dacs, x2, D, z2, H, G, P, Q,
                               dm.start, l)
    got2 = C.ssd_ygate_bwd_doc(do2, yd2, yo2, dacs, x2, D, z2, H, G, P, Q,
                               dm.start, l)
    assert not same_bits(out2, out)
    assert same_bits(out[later], out2[later])
    views = (lambda t: pos_hmajor(t, H, Q, P),
             lambda t: pos_yoff(t, G, Q, rep, P),
             lambda t: pos_nq(t, H, Q), lambda t: t, lambda t: t, lambda t: t)
    for a, b_, v in zip(got, got2, views):
        assert same_bits(v(a)[later], v(b_)[later])


@pytest.mark.parametrize("Q", [64, 128])
def test_ssd_ygate_doc_unmasked_bits(Q):
    """One document per row, and boundaries on chunk starts only, with
    yoff fed zeros where a document starts (what the masked inter-chunk
    matrix hands the kernel there): the unmasked kernel's bits, except
    dyoff on those chunks, which the mask makes 0."""
    P, H, G = 8, 6, 2
    rep = H // G
    l = NC * Q
    ydiag, yoff, dacs, x, D, z, dout = _ygate_case(P, Q, H, Q + 5)
    C = ext()
    for rows in ([[0]] * B, [[0, Q, 3 * Q], [0, 2 * Q], [0, 4 * Q]]):
        dm = mask_of(rows, l)
        opens = ~(rel_start(dm, Q) < 0).reshape(-1)     # flat positions
        yo = torch.where(sel_yoff(opens, G, Q, rep, P),
                         torch.zeros_like(yoff), yoff)
        ref = (C.ssd_ygate_fwd(ydiag, yo, dacs, x, D, z, H, G, P, Q),
               *C.ssd_ygate_bwd(dout, ydiag, yo, dacs, x, D, z, H, G, P, Q))
        got = (C.ssd_ygate_fwd_doc(ydiag, yo, dacs, x, D, z, H, G, P, Q,
                                   dm.start, l),
               *C.ssd_ygate_bwd_doc(dout, ydiag, yo, dacs, x, D, z, H, G, P,
                                    Q, dm.start, l))
        for i, (a, b_) in enumerate(zip(got, ref)):
            if i == 2:                                  # dyoff
                pa, pb = (pos_yoff(t, G, Q, rep, P) for t in (a, b_))
                assert same_bits(pa[~opens], pb[~opens])
                assert (bits(pa)[opens] == 0).all()
            else:
                assert same_bits(a, b_), i


# ---------------------------------------------------------------------
# causal conv1d
# ---------------------------------------------------------------------
CONV_ROWS = [[0, 1, 2, 7, 8, 9, 50, 99], [0]]
CONV_L, CONV_C = 100, 264


def _cuts(starts, L):
    return list(zip(starts, starts[1:] + [L]))


def _conv_lin(x, w, bias):
    W = w.shape[1]
    return F.conv1d(F.pad(x.transpose(1, 2), (W - 1, 0)), w.unsqueeze(1),
                    bias, groups=w.shape[0]).transpose(1, 2)


def _conv_lin_doc(x, w, bias, rows):
    """Pre-activation of the masked conv: the plain conv of every
    document's slice."""
    L = x.shape[1]
    return torch.cat([torch.cat([_conv_lin(x[r:r + 1, s:e], w, bias)
                                 for s, e in _cuts(st, L)], dim=1)
                      for r, st in enumerate(rows)], dim=0)


@pytest.mark.parametrize("W", [2, 3, 4])
def test_causal_conv1d_doc(W):
    torch.manual_seed(W * 1000 + 7)
    L, Cc, b = CONV_L, CONV_C, len(CONV_ROWS)
    dm = mask_of(CONV_ROWS, L)
    x, w, dy = randn(b, L, Cc), randn(Cc, W, scale=0.5), randn(b, L, Cc)
    bias = randn(Cc, dtype=torch.float32)
    C = ext()
    y = C.cconv_fwd_doc(x, w, bias, dm.start)
    dx, dw, db = C.cconv_bwd_doc(dy, x, w, bias, dm.start, dm.end)

    x64 = x.double().requires_grad_()
    w64 = w.double().requires_grad_()
    b64 = bias.double().requires_grad_()
    y_r = reference.causal_conv1d(x64, w64, b64, dm)
    assert y_r.dtype == DD
    dx_r, dw_r, db_r = torch.autograd.grad(y_r, (x64, w64, b64), dy.double())
    with torch.no_grad():
        z = _conv_lin_doc(x64, w64, b64, CONV_ROWS)
        torch.testing.assert_close(z * torch.sigmoid(z), y_r, rtol=1e-12,
                                   atol=1e-12)
        sg = torch.sigmoid(z)
        dsilu = sg * (1 + z * (1 - sg))
        m_z = _conv_lin_doc(x64.abs(), w64.abs(), b64.abs(), CONV_ROWS)
        m_y = m_z * dsilu.abs() + y_r.abs()
        g_abs = dy.double().abs() * sg * (1 + z.abs() * (1 - sg))
    xa = x64.detach().abs().requires_grad_()
    wa = w64.detach().abs().requires_grad_()
    ba = b64.detach().abs().requires_grad_()
    m_dx, m_dw, m_db = torch.autograd.grad(
        _conv_lin_doc(xa, wa, ba, CONV_ROWS), (xa, wa, ba), g_abs)
    # bf16 g buffer between the backward kernels, as in the unmasked test
    m_dx = rule.widen(m_dx, 2.0 ** -8 * m_dx)
    m_dw = rule.widen(m_dw, 2.0 ** -8 * m_dw)
    m_db = rule.widen(m_db, 2.0 ** -8 * m_db)
    tag = f"[W={W}]"
    rule.check("cconv_fwd_doc.y" + tag, y, y_r, m_y, A_RED)
    rule.check("cconv_bwd_doc.dx" + tag, dx, dx_r, m_dx, A_RED)
    rule.check("cconv_bwd_doc.dw" + tag, dw, dw_r, m_dw, A_RED)
    rule.check("cconv_bwd_doc.db" + tag, db, db_r, m_db, A_RED)

    # the autograd wrapper runs the same kernels
    xw = x.clone().requires_grad_()
    ww = w.clone().requires_grad_()
    bw = bias.clone().requires_grad_()
    yw = ops.causal_conv1d(xw, ww, bw, doc_mask=dm)
    assert same_bits(yw, y)
    dxw, dww, dbw = torch.autograd.grad(yw, (xw, ww, bw), dy)
    assert same_bits(dxw, dx)
    rule.check("causal_conv1d doc wrapper.dw" + tag, dww, dw_r, m_dw, A_RED)
    rule.check("causal_conv1d doc wrapper.db" + tag, dbw, db_r, m_db, A_RED)

    # against slices: every document on its own through the unmasked
    # kernels gives the same bits (masked taps add +0 in the same order)
    for r, starts in enumerate(CONV_ROWS):
        for s, e in _cuts(starts, L):
            xs = x[r:r + 1, s:e].contiguous()
            ys = C.cconv_fwd(xs, w, bias)
            dxs, _, _ = C.cconv_bwd(dy[r:r + 1, s:e].contiguous(), xs, w, bias)
            assert same_bits(y[r:r + 1, s:e], ys), (r, s, e)
            assert same_bits(dx[r:r + 1, s:e], dxs), (r, s, e)

    # one document per row: the unmasked kernels' bits (dw / db go through
    # atomics in no fixed order: held to the rule)
    one = mask_of([[0]] * b, L)
    y1 = C.cconv_fwd_doc(x, w, bias, one.start)
    dx1, dw1, db1 = C.cconv_bwd_doc(dy, x, w, bias, one.start, one.end)
    y0 = C.cconv_fwd(x, w, bias)
    dx0, _, _ = C.cconv_bwd(dy, x, w, bias)
    assert same_bits(y1, y0) and same_bits(dx1, dx0)
    z1 = _conv_lin(x64, w64, b64)
    dw1_r, db1_r = torch.autograd.grad(z1 * torch.sigmoid(z1), (w64, b64),
                                       dy.double())
    with torch.no_grad():
        sg1 = torch.sigmoid(z1)
        g1_abs = dy.double().abs() * sg1 * (1 + z1.abs() * (1 - sg1))
    _, m_dw1, m_db1 = torch.autograd.grad(_conv_lin(xa, wa, ba), (xa, wa, ba),
                                          g1_abs)
    rule.check("cconv_bwd_doc.dw one doc" + tag, dw1, dw1_r,
               rule.widen(m_dw1, 2.0 ** -8 * m_dw1), A_RED)
    rule.check("cconv_bwd_doc.db one doc" + tag, db1, db1_r,
               rule.widen(m_db1, 2.0 ** -8 * m_db1), A_RED)

    # isolation: other x / dy in the first document(s), up to a boundary
    for cut in (1, 50):
        sel = torch.zeros(b, L, 1, dtype=torch.bool, device=dev())
        sel[0, :cut] = True
        x2, dy2 = other_where(x, sel, 21), other_where(dy, sel, 22)
        y2 = C.cconv_fwd_doc(x2, w, bias, dm.start)
        dx2, _, _ = C.cconv_bwd_doc(dy2, x2, w, bias, dm.start, dm.end)
        assert not same_bits(y2[0, :cut], y[0, :cut])
        assert same_bits(y2[0, cut:], y[0, cut:]) and same_bits(y2[1], y[1])
        assert same_bits(dx2[0, cut:], dx[0, cut:]) and \
            same_bits(dx2[1], dx[1])


# ---------------------------------------------------------------------
# mixer: fused kernels against the torch path, both with the mask
# ---------------------------------------------------------------------
def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


@pytest.mark.parametrize("Q,G", [(128, 2), (64, 1)])
def test_mixer_doc_fused_matches_torch(Q, G):
    from fms_fsdp_amd.models.mamba import Mamba2Mixer, MambaConfig
    torch.manual_seed(0)
    cfg = MambaConfig(d_model=128, n_layer=1, vocab_size=512, d_state=32,
                      headdim=64, expand=2, ngroups=G, chunk_size=Q)
    mixer = Mamba2Mixer(cfg, 0)
    mixer.reset_parameters()
    mixer = mixer.to(dev()).bfloat16()
    l = NC * Q
    dm = mask_of(ssd_rows(Q), l)
    u = torch.randn(B, l, 128, device=dev(), dtype=torch.bfloat16) * 0.5

    def run(force_torch, mask):
        mixer._force_torch_scan = force_torch
        ui = u.clone().requires_grad_()
        out = mixer(ui, doc_mask=mask)
        (gu,) = torch.autograd.grad(out.float().pow(2).mean(), ui)
        return out.detach(), gu

    o_f, gu_f = run(False, dm)
    o_t, gu_t = run(True, dm)
    print(f"[mixer Q={Q}] out relerr {relerr(o_f, o_t):.3g}, "
          f"du relerr {relerr(gu_f, gu_t):.3g}")
    assert relerr(o_f, o_t) < 3e-2, relerr(o_f, o_t)
    assert relerr(gu_f, gu_t) < 6e-2, relerr(gu_f, gu_t)
    # the mask is visible at this tolerance, and absent where a row is one
    # document
    o_0, _ = run(False, None)
    assert relerr(o_0[:2], o_f[:2]) > 3e-2
    assert same_bits(o_0[2], o_f[2])
    # isolation through the whole mixer: other inputs in the first
    # documents leave the later ones' outputs untouched
    later = later_positions(ssd_rows(Q), l).view(B, l)
    u2 = other_where(u, ~later[..., None], 31)
    mixer._force_torch_scan = False
    with torch.no_grad():
        a, b_ = mixer(u, doc_mask=dm), mixer(u2, doc_mask=dm)
    assert same_bits(a[later], b_[later]) and not same_bits(a, b_)


# ---------------------------------------------------------------------
# preconditions: refused before any launch
# ---------------------------------------------------------------------
def test_doc_bindings_reject_bad_arguments():
    C = ext()
    Q, H, G, P = 64, 4, 2, 8
    l = 2 * Q
    rows, N = 2 * l, 2 * 2 * H
    f32 = torch.float32
    dtf, dacs = randn(N, Q, dtype=f32), randn(N, Q, dtype=f32)
    x, z = randn(rows, H * P), randn(rows, H * P)
    scores, g = randn(2 * 2 * G, Q, Q), randn(N, Q, Q)
    yd, yo, dout = randn(rows, H * P), randn(rows, H * P), randn(rows, H * P)
    D = randn(H, dtype=f32)
    good = mask_of([[0, 5], [0]], l)
    xc, wc, bc_ = randn(2, l, 16), randn(16, 4), randn(16, dtype=f32)
    R = pytest.raises(RuntimeError)
    bad = [good.start.long(),                       # dtype
           good.start[:, :l - 1].contiguous(),      # length
           good.start.cpu(),                        # device
           good.start.t()]                          # not contiguous
    for s in bad:
        with R:
            C.ssd_xdt_fwd_doc(x, dtf, dacs, H, P, Q, s, l)
        with R:
            C.ssd_xdt_bwd_doc(yd, yd, x, dtf, dacs, H, P, Q, s, l)
        with R:
            C.ssd_sl_fwd_doc(dacs, scores, H, G, s, l)
        with R:
            C.ssd_sl_bwd_doc(g, scores, dacs, H, G, s, l)
        with R:
            C.ssd_ygate_fwd_doc(yd, yo, dacs, x, D, z, H, G, P, Q, s, l)
        with R:
            C.ssd_ygate_bwd_doc(dout, yd, yo, dacs, x, D, z, H, G, P, Q, s, l)
        with R:
            C.cconv_fwd_doc(xc, wc, bc_, s)
        with R:
            C.cconv_bwd_doc(xc, xc, wc, bc_, s, good.end)
        with R:
            C.cconv_bwd_doc(xc, xc, wc, bc_, good.start, s)
    for bad_l in (0, l + 8, 3 * Q):                 # l % Q, rows % l
        with R:
            C.ssd_xdt_fwd_doc(x, dtf, dacs, H, P, Q, good.start, bad_l)
        with R:
            C.ssd_sl_fwd_doc(dacs, scores, H, G, good.start, bad_l)
        with R:
            C.ssd_ygate_fwd_doc(yd, yo, dacs, x, D, z, H, G, P, Q,
                                good.start, bad_l)
    with pytest.raises(ValueError):
        ops.ssd_xdt(x, dtf, dacs, H, P, Q, doc_mask=mask_of([[0]], l))
    torch.cuda.synchronize()
