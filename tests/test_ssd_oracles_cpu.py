"""The SSD oracles of ops/reference.py, composed exactly as
Mamba2Mixer._scan_fused composes the HIP kernels (plain matmuls where it
calls bmm/einsum), against the sequential recurrence in float64 — so the
oracles that judge the kernels cannot be wrong in the kernels' own way.
Also the CPU test of the shared comparison rule (tests/oracle_rule.py)."""

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd.models.mamba import segsum
from fms_fsdp_amd.ops import reference
from test_mamba_cpu import naive_ssd


def scan_from_oracles(b, l, x, dt, z, B, C, dtb, Alog, D_, h, p, g, n, Q):
    nc = l // Q
    rep = h // g
    N = b * nc * h
    dt2 = dt.reshape(b * l, h)
    x2 = x.reshape(b * l, h * p)
    z2 = z.reshape(b * l, h * p)
    dtf, dacs = reference.ssd_prep(dt2, dtb, Alog, Q)
    xdt, xdtd = reference.ssd_xdt(x2, dtf, dacs, h, p, Q)
    Bm = B.reshape(b, nc, Q, g, n)
    Cm = C.reshape(b, nc, Q, g, n)
    # "bcqgn,bckgn->bcgqk"
    scores = Cm.permute(0, 1, 3, 2, 4) @ Bm.permute(0, 1, 3, 4, 2)
    sL = reference.ssd_scores_decay(
        dacs, scores.reshape(b * nc * g, Q, Q), h, g)
    y_diag = sL @ xdt.view(N, Q, p)
    # "bckgn,bcgrkp->bcgrnp"
    states = (Bm.permute(0, 1, 3, 4, 2).unsqueeze(3)
              @ xdtd.view(b, nc, g, rep, Q, p)).reshape(b, nc, h, n, p)
    G = dacs.view(b, nc, h, Q)[..., -1].permute(0, 2, 1)
    W = torch.exp(segsum(G))
    Wsh = torch.cat([torch.zeros_like(W[:, :, :1]), W[:, :, :-1]], dim=2)
    # "bhzc,bchnp->bzhnp"
    prev = (Wsh @ states.permute(0, 2, 1, 3, 4).reshape(b, h, nc, n * p)) \
        .view(b, h, nc, n, p).permute(0, 2, 1, 3, 4)
    # "bcqgn,bcgrnp->bcgqrp"
    pv = prev.reshape(b, nc, g, rep, n, p).permute(0, 1, 2, 4, 3, 5) \
        .reshape(b, nc, g, n, rep * p)
    y_off = Cm.permute(0, 1, 3, 2, 4) @ pv          # (b, nc, g, Q, rep*p)
    out = reference.ssd_ygate(
        y_diag.reshape(b * l, h * p), y_off.reshape(b * l, h * p), dacs,
        x2, D_, z2, h, g, p, Q)
    return out.view(b, l, h * p)


@pytest.mark.parametrize("Q,h,g,p", [(64, 6, 2, 8), (16, 4, 4, 8),
                                     (32, 4, 1, 16)])
def test_oracles_compose_to_recurrence(Q, h, g, p):
    torch.manual_seed(0)
    dd = torch.float64
    b, n, nc = 2, 16, 3
    l = nc * Q

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, dtype=dd) * scale).requires_grad_()

    x, z = leaf(b, l, h * p), leaf(b, l, h * p)
    dt = leaf(b, l, h, scale=2.0)
    B, C = leaf(b, l, g * n), leaf(b, l, g * n)
    dtb = leaf(h)
    # |A| from 0.02 to 4: the slow heads carry state across all three
    # chunks, the fast ones decay below e^-20 inside one
    Alog = torch.linspace(-4.0, 1.4, h, dtype=dd).requires_grad_()
    D_ = leaf(h)
    leaves = (x, dt, z, B, C, dtb, Alog, D_)
    names = ("x", "dt", "z", "B", "C", "dt_bias", "A_log", "D")

    out = scan_from_oracles(b, l, x, dt, z, B, C, dtb, Alog, D_,
                            h, p, g, n, Q)

    xh = x.view(b, l, h, p)
    dtf = torch.nn.functional.softplus(dt + dtb, threshold=1e9)
    y = naive_ssd(xh, dtf, -torch.exp(Alog), B.view(b, l, g, n),
                  C.view(b, l, g, n))
    assert y.dtype == dd
    y = y + xh * D_.view(1, 1, h, 1)
    ref = y.reshape(b, l, h * p) * torch.nn.functional.silu(z)

    with torch.no_grad():
        dacs_end = (dtf * -torch.exp(Alog)).view(b, nc, Q, h).sum(2)
        assert dacs_end.min() < -20 and dacs_end.max() > -3

    torch.testing.assert_close(out, ref, rtol=1e-9, atol=1e-12)
    cot = torch.randn_like(ref)
    got_g = torch.autograd.grad(out, leaves, cot)
    ref_g = torch.autograd.grad(ref, leaves, cot)
    for nm, a, r in zip(names, got_g, ref_g):
        torch.testing.assert_close(a, r, rtol=1e-9, atol=1e-12,
                                   msg=lambda m, nm=nm: f"d{nm}: {m}")


# ---------------------------------------------------------------------
# the comparison rule itself
# ---------------------------------------------------------------------
def _rmsnorm_case():
    torch.manual_seed(1)
    rows, H = 7, 5120
    x = torch.randn(rows, H).bfloat16()
    w = torch.randn(H).bfloat16()
    xf, wf = x.float(), w.float()
    # fp32 emulation of the kernel's chain, rounded to bf16 once
    got = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)
           * wf).bfloat16()
    xd, wd = x.double(), w.double()
    ref = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * wd
    return got, ref


def test_rule_accepts_bf16_rounding_of_fp32_emulation():
    got, ref = _rmsnorm_case()
    ratio = rule.check("selftest", got, ref, ref.abs(), rule.A_REDUCE)
    assert 0.5 < ratio <= 1.0      # the bf16 rounding itself


def test_rule_rejects_two_bf16_ulps():
    got, ref = _rmsnorm_case()
    bad = got.clone()
    bits = bad.view(torch.int16)
    assert bits[3, 1234] > 0 and bits[3, 1234] < 0x7F00
    bits[3, 1234] += 2                  # two ulps up, one element
    with pytest.raises(AssertionError, match=r"err/tol = .* \(3, 1234\)"):
        rule.check("selftest_bad", bad, ref, ref.abs(), rule.A_REDUCE)


def test_rule_rejects_nan_and_inf():
    got, ref = _rmsnorm_case()
    for v in (float("nan"), float("inf")):
        bad = got.clone()
        bad[2, 17] = v
        with pytest.raises(AssertionError, match=r"\(2, 17\)"):
            rule.check("selftest_bad", bad, ref, ref.abs(), rule.A_REDUCE)


def test_rule_zero_allowance_is_exact():
    ref = torch.zeros(4, dtype=torch.float64)
    rule.check("selftest", torch.zeros(4), ref, ref, rule.A_CHAIN)
    with pytest.raises(AssertionError):
        rule.check("selftest_bad", torch.tensor([0., 0., 1e-30, 0.]), ref,
                   ref, rule.A_CHAIN)
