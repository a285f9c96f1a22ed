"""Every `_C.ssd_*` entry point against its float64 oracle
(fms_fsdp_amd.ops.reference, tied to the recurrence on the CPU by
test_ssd_oracles_cpu.py), under the one rule of tests/oracle_rule.py.
The bindings are called directly; where a Python wrapper folds something
in (the end column of sdec, the per-group sum of dsh, dD_rows.sum(0)) the
wrapper is checked as well. All inputs are the bf16/fp32 tensors the
kernels take, upcast to float64 for the oracle."""

import math

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference

pytestmark = pytest.mark.gpu

DD = torch.float64
BF = torch.bfloat16
A_RED, A_CH = rule.A_REDUCE, rule.A_CHAIN
B_NC = 4    # b * nc = 2 * 2 chunks


def dev():
    return torch.device("cuda:0")


def ext():
    from fms_fsdp_amd import _C
    return _C


def randn(*shape, dtype=BF, scale=1.0):
    return (torch.randn(*shape, device=dev()) * scale).to(dtype)


def col_slice(rows, cols, lead=8, trail=24, scale=1.0):
    """(rows, cols) bf16 column slice of a wider buffer: row stride > cols."""
    wide = randn(rows, lead + cols + trail, scale=scale)
    return wide[:, lead:lead + cols]


def make_dacs(N, Q):
    """fp32 (N, Q) negative chunk-cumsums whose per-row rates span
    1/Q .. 60/Q per step (chunk totals of about -0.5 .. -30): the slow
    rows barely decay, the fast ones pass exp(-20) inside the chunk."""
    rate = torch.logspace(math.log10(1.0 / Q), math.log10(60.0 / Q), N,
                          device=dev())
    rate = rate[torch.randperm(N, device=dev())]
    dacs = -(torch.rand(N, Q, device=dev()) * rate[:, None]).cumsum(-1)
    assert dacs[:, -1].min() < -20 and dacs[:, -1].max() > -1
    return dacs.float().contiguous()


def revcumsum(t):
    return t.flip(-1).cumsum(-1).flip(-1)


# ---------------------------------------------------------------------
# prep
# ---------------------------------------------------------------------
@pytest.mark.parametrize("Q", [64, 128, 192, 256])
def test_ssd_prep(Q):
    torch.manual_seed(Q)
    H = 3
    rows = B_NC * Q
    dt = col_slice(rows, H, lead=5, trail=4, scale=3.0)
    assert dt.stride(0) > H
    # head 0 straddles the softplus guard at +20, head 1 lies around -20
    bias = torch.tensor([20.0, -20.0, 0.3], device=dev())
    alog = torch.tensor([-3.0, 1.0, 0.5], device=dev())
    x = dt.double() + bias.double()
    assert (x > 20).any() and (x < -20).any()

    dtf, dacs = ext().ssd_prep_fwd(dt, bias, alog, Q)
    dt64 = dt.double().requires_grad_()
    b64 = bias.double().requires_grad_()
    a64 = alog.double().requires_grad_()
    dtf_r, dacs_r = reference.ssd_prep(dt64, b64, a64, Q)
    assert dacs_r.min() < -20
    with torch.no_grad():
        # fp32 effect (measured 1.75x the plain rule at x = -25.7): the
        # sum x = dt + bias rounds by |x|*2^-24, and __expf(x) = exp2(x *
        # log2 e) rounds its argument by as much again, so e^x is off by
        # |x|*2^-23 relative; softplus passes that on times sigmoid(x).
        # Nothing to add above the guard, where dtf = x.
        xq = x.view(B_NC, Q, H).transpose(1, 2).reshape(-1, Q)
        e_exp = torch.where(xq > 20, torch.zeros_like(xq),
                            xq.abs() * 2.0 ** -23 * torch.sigmoid(xq))
        m_dtf = rule.widen(dtf_r.abs(), e_exp, A_CH)
    rule.check(f"ssd_prep_fwd.dtf[Q={Q}]", dtf, dtf_r, m_dtf, A_CH)
    # summands dtf*A all have one sign: the sum of their magnitudes is |ref|
    rule.check(f"ssd_prep_fwd.dacs[Q={Q}]", dacs, dacs_r, dacs_r.abs(), A_RED)

    ddtf = randn(*dtf.shape, dtype=torch.float32)
    ddacs = randn(*dacs.shape, dtype=torch.float32)
    ddt, dbias, dalog = ext().ssd_prep_bwd(ddtf, ddacs, dt, bias, alog, Q)
    ddt_r, dbias_r, dalog_r = torch.autograd.grad(
        (dtf_r, dacs_r), (dt64, b64, a64), (ddtf.double(), ddacs.double()))
    with torch.no_grad():
        # ddt[q] = (ddtf[q] + A * sum_{i>=q} ddacs[i]) * sigmoid(x[q])
        absA = torch.exp(a64)
        rc_abs = revcumsum(ddacs.double().abs())               # (N, Q)
        sig = torch.sigmoid(x).view(B_NC, Q, H).transpose(1, 2)
        absA_n = absA.view(1, H, 1)
        m_nq = (ddtf.double().abs().view(B_NC, H, Q)
                + absA_n * rc_abs.view(B_NC, H, Q)) * sig      # (bc, H, Q)
        m_ddt = m_nq.transpose(1, 2).reshape(rows, H)
        m_dbias = m_nq.sum((0, 2))
        m_dalog = (rc_abs.view(B_NC, H, Q) * dtf_r.view(B_NC, H, Q)
                   * absA_n).sum((0, 2))
    rule.check(f"ssd_prep_bwd.ddt[Q={Q}]", ddt, ddt_r, m_ddt, A_RED)
    rule.check(f"ssd_prep_bwd.dbias[Q={Q}]", dbias, dbias_r, m_dbias, A_RED)
    rule.check(f"ssd_prep_bwd.dalog[Q={Q}]", dalog, dalog_r, m_dalog, A_RED)


# ---------------------------------------------------------------------
# xdt
# ---------------------------------------------------------------------
@pytest.mark.parametrize("Q", [64, 128])
@pytest.mark.parametrize("P", [8, 16, 64, 128])
def test_ssd_xdt(P, Q):
    torch.manual_seed(P * 1000 + Q)
    H = 4
    rows, N = B_NC * Q, B_NC * H
    x = col_slice(rows, H * P)
    dtf = (torch.rand(N, Q, device=dev()) * 2).float()
    dacs = make_dacs(N, Q)
    tag = f"[P={P},Q={Q}]"

    xdt, xdtd = ext().ssd_xdt_fwd(x, dtf, dacs, H, P, Q)
    x64 = x.double().requires_grad_()
    f64 = dtf.double().requires_grad_()
    c64 = dacs.double().requires_grad_()
    xdt_r, xdtd_r = reference.ssd_xdt(x64, f64, c64, H, P, Q)
    rule.check("ssd_xdt_fwd.xdt" + tag, xdt, xdt_r, xdt_r.abs(), A_CH)
    rule.check("ssd_xdt_fwd.xdtd" + tag, xdtd, xdtd_r, xdtd_r.abs(), A_CH)

    g1, g2 = randn(rows, H * P), randn(rows, H * P)
    dx, ddtf, sdec = ext().ssd_xdt_bwd(g1, g2, x, dtf, dacs, H, P, Q)
    dx_r, ddtf_r, ddacs_r = torch.autograd.grad(
        (xdt_r, xdtd_r), (x64, f64, c64), (g1.double(), g2.double()))
    with torch.no_grad():
        # everything below in the h-major (bc, H, Q, P) layout of g1/g2
        a1 = g1.double().abs().view(B_NC, H, Q, P)
        a2 = g2.double().abs().view(B_NC, H, Q, P)
        xh = x.double().view(B_NC, Q, H, P).permute(0, 2, 1, 3)
        f = f64.view(B_NC, H, Q, 1)
        cs = c64.view(B_NC, H, Q)
        dec = torch.exp(cs[..., -1:] - cs).unsqueeze(-1)
        m_dx = ((a1 + a2 * dec) * f).permute(0, 2, 1, 3).reshape(rows, H * P)
        m_ddtf = ((a1 + a2 * dec) * xh.abs()).sum(-1).view(N, Q)
        s_terms = g2.double().view(B_NC, H, Q, P) * xh * f * dec
        sdec_r = s_terms.sum(-1).view(N, Q)
        m_sdec = s_terms.abs().sum(-1).view(N, Q)
        # wrapper: ddacs = -sdec, end column += sum_q sdec
        m_ddacs = m_sdec.clone()
        m_ddacs[:, -1] += m_sdec.sum(-1)
    rule.check("ssd_xdt_bwd.dx" + tag, dx, dx_r, m_dx, A_CH)
    rule.check("ssd_xdt_bwd.ddtf" + tag, ddtf, ddtf_r, m_ddtf, A_RED)
    rule.check("ssd_xdt_bwd.sdec" + tag, sdec, sdec_r, m_sdec, A_RED)

    dacs_w = dacs.clone().requires_grad_()
    o1, o2 = ops.ssd_xdt(x, dtf, dacs_w, H, P, Q)
    assert torch.equal(o1, xdt) and torch.equal(o2, xdtd)
    (ddacs,) = torch.autograd.grad((o1, o2), dacs_w, (g1, g2))
    rule.check("ssd_xdt wrapper.ddacs" + tag, ddacs, ddacs_r, m_ddacs, A_RED)


# ---------------------------------------------------------------------
# scores * decay
# ---------------------------------------------------------------------
@pytest.mark.parametrize("H,G", [(4, 4), (4, 1), (6, 2)])
@pytest.mark.parametrize("Q", [64, 128, 192, 256])
def test_ssd_sl(Q, H, G):
    torch.manual_seed(Q * 10 + H + G)
    N, M, rep = B_NC * H, B_NC * G, H // G
    dacs = make_dacs(N, Q)
    scores = randn(M, Q, Q, scale=2.0)
    tag = f"[Q={Q},H={H},G={G}]"

    sL = ext().ssd_sl_fwd(dacs, scores, H, G)
    c64 = dacs.double().requires_grad_()
    s64 = scores.double().requires_grad_()
    sL_r = reference.ssd_scores_decay(c64, s64, H, G)
    rule.check("ssd_sl_fwd.sL" + tag, sL, sL_r, sL_r.abs(), A_CH)
    upper = torch.triu(torch.ones(Q, Q, dtype=torch.bool, device=dev()), 1)
    assert (sL.view(torch.int16)[:, upper] == 0).all(), "nonzero above diag"

    g = randn(N, Q, Q)
    dsh, dcs = ext().ssd_sl_bwd(g, scores, dacs, H, G)
    dcs_r, dsc_r = torch.autograd.grad(sL_r, (c64, s64), g.double())
    with torch.no_grad():
        L = reference.ssd_scores_decay(
            c64, torch.ones(M, Q, Q, dtype=DD, device=dev()), H, G)
        dsh_r = g.double() * L
        prod = (g.double() * sL_r).abs()
        m_dcs = prod.sum(2) + prod.sum(1)
    rule.check("ssd_sl_bwd.dsh" + tag, dsh, dsh_r, dsh_r.abs(), A_CH)
    # zero above the diagonal; the fused Q = 128 kernel leaves g * 0 there,
    # which is -0.0 for negative g, so compare values, not bit patterns
    assert (dsh[:, upper] == 0).all()
    rule.check("ssd_sl_bwd.dcs" + tag, dcs, dcs_r, m_dcs, A_RED)

    # wrapper: d_scores[m] = sum over the group's heads of dsh
    dacs_w = dacs.clone().requires_grad_()
    sc_w = scores.clone().requires_grad_()
    out = ops.ssd_scores_decay(dacs_w, sc_w, H, G)
    assert torch.equal(out, sL)
    dcs_w, dsc_w = torch.autograd.grad(out, (dacs_w, sc_w), g)
    assert torch.equal(dcs_w, dcs)
    with torch.no_grad():
        m_dsc = dsh_r.abs().view(B_NC, G, rep, Q, Q).sum(2).view(M, Q, Q)
        if rep > 1:
            # the per-head summands are stored in bf16 (dsh) before the
            # fp32 group sum, so each carries a rounding of its own:
            # 2^-8 * sum_r |g_r L_r| on top of the final rounding
            m_dsc = rule.widen(m_dsc, 2.0 ** -8 * m_dsc, A_RED)
    rule.check("ssd_scores_decay wrapper.dscores" + tag, dsc_w, dsc_r, m_dsc,
               A_RED)


# ---------------------------------------------------------------------
# ygate
# ---------------------------------------------------------------------
@pytest.mark.parametrize("Q", [64, 128])
@pytest.mark.parametrize("P", [8, 64, 128])
def test_ssd_ygate(P, Q):
    torch.manual_seed(P * 1000 + Q + 1)
    H, G = 6, 2
    rep = H // G
    rows, N, HP = B_NC * Q, B_NC * H, H * P
    fused = randn(rows, 2 * HP + 40)
    z, x = fused[:, 8:8 + HP], fused[:, 16 + HP:16 + 2 * HP]
    ydiag, yoff = randn(rows, HP), randn(rows, HP)
    dacs = make_dacs(N, Q)
    # slow rows only: exp(dacs) keeps the yoff term visible in out
    dacs[::2] *= 0.01
    D = randn(H, dtype=torch.float32)
    tag = f"[P={P},Q={Q}]"

    out = ext().ssd_ygate_fwd(ydiag, yoff, dacs, x, D, z, H, G, P, Q)
    leaves = [t.double().requires_grad_()
              for t in (ydiag, yoff, dacs, x, D, z)]
    yd64, yo64, c64, x64, D64, z64 = leaves
    out_r = reference.ssd_ygate(yd64, yo64, c64, x64, D64, z64, H, G, P, Q)

    def to_rows(t_bqhp):
        return t_bqhp.reshape(rows, HP)

    with torch.no_grad():
        # all in the (bc, Q, H, P) layout of out / x / z
        ydq = yd64.view(B_NC, H, Q, P).permute(0, 2, 1, 3)
        yoq = yo64.view(B_NC, G, Q, rep, P).permute(0, 2, 1, 3, 4) \
            .reshape(B_NC, Q, H, P)
        sd = torch.exp(c64.view(B_NC, H, Q)).permute(0, 2, 1).unsqueeze(-1)
        xq = x64.view(B_NC, Q, H, P)
        zq = z64.view(B_NC, Q, H, P)
        Dq = D64.view(1, 1, H, 1)
        sg = torch.sigmoid(zq)
        m_y = ydq.abs() + yoq.abs() * sd + xq.abs() * Dq.abs()
        m_out = m_y * (zq * sg).abs()
    rule.check("ssd_ygate_fwd.out" + tag, out, out_r, to_rows(m_out), A_CH)

    dout = randn(rows, HP)
    dydiag, dyoff, ddacs, dx, dD_rows, dz = ext().ssd_ygate_bwd(
        dout, ydiag, yoff, dacs, x, D, z, H, G, P, Q)
    dyd_r, dyo_r, dc_r, dx_r, dD_r, dz_r = torch.autograd.grad(
        out_r, leaves, dout.double())
    with torch.no_grad():
        gy = dout.double().view(B_NC, Q, H, P)
        dy = gy * zq * sg
        dDrows_r = (dy * xq).sum(-1).reshape(rows, H)
        m_dDrows = (dy * xq).abs().sum(-1).reshape(rows, H)
        m_dD = m_dDrows.sum(0)
        m_ddacs = (dy * yoq * sd).abs().sum(-1).permute(0, 2, 1) \
            .reshape(N, Q)
        # dz = gy * y * sg * (1 + z*(1 - sg)): y and the bracket are sums
        m_dz = gy.abs() * m_y * sg * (1 + zq.abs() * (1 - sg))
    rule.check("ssd_ygate_bwd.dydiag" + tag, dydiag, dyd_r, dyd_r.abs(), A_CH)
    rule.check("ssd_ygate_bwd.dyoff" + tag, dyoff, dyo_r, dyo_r.abs(), A_CH)
    rule.check("ssd_ygate_bwd.dx" + tag, dx, dx_r, dx_r.abs(), A_CH)
    rule.check("ssd_ygate_bwd.dz" + tag, dz, dz_r, to_rows(m_dz), A_CH)
    rule.check("ssd_ygate_bwd.ddacs" + tag, ddacs, dc_r, m_ddacs, A_RED)
    rule.check("ssd_ygate_bwd.dD_rows" + tag, dD_rows, dDrows_r, m_dDrows,
               A_RED)

    D_w = D.clone().requires_grad_()
    o = ops.ssd_ygate(ydiag, yoff, dacs, x, D_w, z, H, G, P, Q)
    assert torch.equal(o, out)
    (dD,) = torch.autograd.grad(o, D_w, dout)
    rule.check("ssd_ygate wrapper.dD" + tag, dD, dD_r, m_dD, A_RED)


# ---------------------------------------------------------------------
# preconditions: invalid arguments only, refused before any launch
# ---------------------------------------------------------------------
def test_ssd_bindings_reject_bad_arguments():
    C = ext()
    Q, H, G, P = 64, 4, 2, 8
    rows, N = 2 * Q, 2 * H
    f32 = torch.float32
    dt = randn(rows, H)
    bias, alog = randn(H, dtype=f32), randn(H, dtype=f32)
    dtf, dacs = randn(N, Q, dtype=f32), randn(N, Q, dtype=f32)
    x, z = randn(rows, H * P), randn(rows, H * P)
    scores = randn(2 * G, Q, Q)
    g = randn(N, Q, Q)
    yd, yo, dout = randn(rows, H * P), randn(rows, H * P), randn(rows, H * P)
    D = randn(H, dtype=f32)
    R = pytest.raises(RuntimeError)

    with R:
        C.ssd_prep_fwd(dt, bias, alog, 96)            # Q not 64..256 by 64
    with R:
        C.ssd_prep_bwd(dtf, dacs, dt, bias, alog, 32)  # same check as fwd
    with R:
        C.ssd_prep_bwd(dtf, dacs, dt, bias, alog, 0)
    with R:
        C.ssd_prep_bwd(dtf[:, :32].contiguous(), dacs, dt, bias, alog, Q)
    with R:
        C.ssd_prep_bwd(dtf, dacs.double(), dt, bias, alog, Q)
    with R:
        C.ssd_prep_fwd(dt, bias[:2], alog, Q)
    with R:
        C.ssd_xdt_fwd(x, dtf, dacs, H, P, 60)          # Q % 8
    with R:
        C.ssd_xdt_fwd(randn(rows, H * 12), dtf, dacs, H, 12, Q)   # P % 8
    with R:
        C.ssd_xdt_fwd(x, dtf.t().contiguous().t(), dacs, H, P, Q)
    with R:
        C.ssd_xdt_fwd(x, dtf, dacs[:N - 1], H, P, Q)
    with R:
        C.ssd_xdt_fwd(x, dtf.bfloat16(), dacs, H, P, Q)
    with R:
        C.ssd_xdt_bwd(yd[:rows - 1], yd, x, dtf, dacs, H, P, Q)
    with R:
        C.ssd_xdt_bwd(yd.float(), yd, x, dtf, dacs, H, P, Q)
    with R:
        C.ssd_sl_fwd(dacs, scores, H, 3)               # H % G
    with R:
        C.ssd_sl_fwd(dacs, scores[:3], H, G)           # (N/H*G, Q, Q)
    with R:
        C.ssd_sl_fwd(dacs, scores[:, :, :32].contiguous(), H, G)
    with R:
        C.ssd_sl_bwd(g, scores, dacs.bfloat16(), H, G)
    with R:
        C.ssd_sl_bwd(g[:, :, :32], scores, dacs, H, G)   # not contiguous
    with R:
        C.ssd_sl_bwd(g.float(), scores, dacs, H, G)
    with R:
        C.ssd_sl_bwd(g, scores, dacs, H, 3)
    with R:
        C.ssd_ygate_fwd(yd, yo, dacs, x, D, z, H, 3, P, Q)
    with R:
        C.ssd_ygate_fwd(yd[:rows - 1], yo, dacs, x, D, z, H, G, P, Q)
    with R:
        C.ssd_ygate_fwd(yd, yo.float(), dacs, x, D, z, H, G, P, Q)
    with R:
        C.ssd_ygate_fwd(yd, yo, dacs[:N - 1], x, D, z, H, G, P, Q)
    with R:
        C.ssd_ygate_bwd(dout[:, :H * P - 8], yd, yo, dacs, x, D, z,
                        H, G, P, Q)
    with R:
        C.ssd_ygate_bwd(dout, yd, yo, dacs, x, D, z, H, G, P, 60)
    torch.cuda.synchronize()
