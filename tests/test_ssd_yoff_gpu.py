"""The y_off kernels (ops/hip/ssd_yoff.hip) against reference.ssd_yoff in
float64 on the same bf16 inputs, under tests/oracle_rule.py, then through
ops.ssd_yoff and the training scan under ops.ssd_yoff_mode("fused").

Every output is an fp32 sum of exact products of bf16 inputs, rounded to bf16
once (dC after the sum of its head-block partials): R = 2^-8, A = A_REDUCE,
mag = the same expression at |C|, |prev|, |dyoff|, nothing widened."""

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_mamba_decode_gpu import relerr
from test_ssd_docmask_gpu import mask_of, same_bits, ssd_rows
from test_ssd_kernels_gpu import col_slice, ext, randn
from test_ssd_state_gpu import small_mixer

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
A_RED = rule.A_REDUCE

# More than one head per workgroup. ssd_yoff_plan halves the head block HB
# (cap 8; dprev 4 at (128, 64)) while base * ceil(rep / HB) stays under two
# workgroups per CU, 512 on a 256-CU MI355X, with base = bc*G*ceil(Q/128)
# for the forward and bc*G for dprev; the cases above all end at HB = 1.
# These are the smallest bc that keep HB > 1, heads per workgroup
# (fwd | dprev):
#   171 * ceil(21/8) = 513            8, 8, 5 | 8, 8, 5
#   512 * 1                           5 | 5 (odd block, odd last head)
#   256 * ceil(5/3) = 256 * ceil(5/4) 3, 2 | 4, 1 (the tile of 128 state rows)
#   256 * 2 groups * 1                3 | 3, second 64-row tile half full
# The last two hold 20 MB and 19 MB in their largest tensor, the least
# that reaches 512 workgroups at those tiles.
MULTI_HEAD = [(16, 32, 32, 21, 1, 171), (16, 32, 32, 5, 1, 512),
              (128, 64, 32, 5, 1, 256), (64, 64, 96, 6, 2, 256)]
# single-wave block, block with idle waves, two row blocks; the padded N;
# rep = 3; 21 head blocks of one head; then the blocks of several heads
FWD_CASES = [(N, P, Q, H, G, 3) for N, P in [(16, 32), (64, 64), (128, 64)]
             for Q in (32, 96, 256) for H, G in [(4, 1), (6, 2)]] \
    + [(128, 64, 32, 21, 1, 2)] + MULTI_HEAD
# ... and the partial sum over explicit head blocks
BWD_CASES = [c + (0,) for c in FWD_CASES] \
    + [(128, 64, 32, 21, 1, 2, hb) for hb in (1, 2, 21)] \
    + [(16, 32, 32, 6, 2, 3, hb) for hb in (1, 2, 3)]


def oracle(C, prev, dyoff, dims):
    """float64 (yoff, dC, dprev) and the same at the absolute values."""
    def run(f):
        Cd, pd = (f(t.double()).requires_grad_() for t in (C, prev))
        y = reference.ssd_yoff(Cd, pd, *dims)
        if dyoff is None:
            return (y.detach(),)
        return (y.detach(),) + torch.autograd.grad(
            y, (Cd, pd), f(dyoff.double()).view_as(y))
    return run(lambda t: t), run(torch.abs)


def check_grads(tag, dC, dprev, C, prev, dyoff, dims):
    ref, mag = oracle(C, prev, dyoff, dims)
    assert dC.dtype == BF and dprev.dtype == BF
    rule.check("ssd_yoff_bwd.dC" + tag, dC, ref[1], mag[1], A_RED)
    rule.check("ssd_yoff_bwd.dprev" + tag, dprev, ref[2], mag[2], A_RED)


@pytest.mark.parametrize("N,P,Q,H,G,bc", FWD_CASES)
def test_yoff_fwd(N, P, Q, H, G, bc):
    torch.manual_seed(N + P + Q + H)
    C, prev = col_slice(bc * Q, G * N), randn(bc * H, N, P)
    assert C.stride(0) > G * N
    n0 = ext().ssd_yoff_calls()
    y = ext().ssd_yoff_fwd(C, prev, H, G, P, N, Q)
    assert ext().ssd_yoff_calls() == n0 + 1
    assert y.dtype == BF and y.numel() == bc * Q * H * P
    ref, mag = oracle(C, prev, None, (H, G, P, N, Q))
    rule.check(f"ssd_yoff_fwd[N={N},P={P},Q={Q},H={H},G={G},bc={bc}]",
               y.view(ref[0].shape), ref[0], mag[0], A_RED)
    assert same_bits(ext().ssd_yoff_fwd(C, prev, H, G, P, N, Q), y)


@pytest.mark.parametrize("N,P,Q,H,G,bc,hb", BWD_CASES)
def test_yoff_bwd(N, P, Q, H, G, bc, hb):
    torch.manual_seed(N + P + Q + H + hb)
    C, prev = col_slice(bc * Q, G * N), randn(bc * H, N, P)
    dyoff = randn(bc, G, Q, H // G, P)
    n0 = ext().ssd_yoff_calls()
    dCp, dprev = ext().ssd_yoff_bwd(dyoff, C, prev, H, G, P, N, Q, hb)
    assert ext().ssd_yoff_calls() == n0 + 1
    assert dCp.dtype == torch.float32 and dCp.shape[1:] == (bc * Q, G * N)
    assert dCp.shape[0] == hb or hb == 0
    assert dprev.shape == prev.shape
    check_grads(f"[N={N},P={P},Q={Q},H={H},G={G},bc={bc},hb={hb}]",
                dCp.sum(0).to(BF), dprev, C, prev, dyoff, (H, G, P, N, Q))
    again = ext().ssd_yoff_bwd(dyoff, C, prev, H, G, P, N, Q, hb)
    assert same_bits(again[0], dCp) and same_bits(again[1], dprev)


def test_through_the_op():
    N, P, Q, H, G, bc = 64, 64, 96, 6, 2, 3
    dims = (H, G, P, N, Q)
    torch.manual_seed(5)
    C, prev = col_slice(bc * Q, G * N), randn(bc * H, N, P)
    dyoff = randn(bc, G, Q, H // G, P)

    def run(mode):
        old = ops.ssd_yoff_mode(mode)
        try:
            assert ops.ssd_yoff_mode() == mode
            Ci, pi = C.detach().requires_grad_(), prev.clone().requires_grad_()
            n0 = ext().ssd_yoff_calls()
            y = ops.ssd_yoff(Ci, pi, *dims)
            gr = torch.autograd.grad(y, (Ci, pi), dyoff.view_as(y))
            return y.detach(), gr, ext().ssd_yoff_calls() - n0
        finally:
            assert ops.ssd_yoff_mode(old) == mode
    y, (dC, dprev), calls = run("fused")
    assert calls == 2
    assert dC.shape == C.shape and dprev.shape == prev.shape
    ref, mag = oracle(C, prev, None, dims)
    rule.check("ssd_yoff[op]", y, ref[0], mag[0], A_RED)
    check_grads("[op]", dC, dprev, C, prev, dyoff, dims)
    y_g, _, calls = run("gemm")
    assert calls == 0
    inline = torch.einsum("bcqgn,bcgrnp->bcgqrp", C.reshape(1, bc, Q, G, N),
                          prev.view(1, bc, G, H // G, N, P))
    assert y_g.shape == y.shape and same_bits(y_g, inline[0])
    # a gradient that nobody asks for is not computed: an empty tensor
    part, none = ext().ssd_yoff_bwd(dyoff, C, prev, *dims, need_dprev=False)
    assert none.numel() == 0 and same_bits(part.sum(0).to(BF), dC)
    with pytest.raises(ValueError):
        ops.ssd_yoff_mode("einsum")


@pytest.mark.parametrize("masked", [False, True])
def test_training_scan_fused_yoff_matches_gemm(masked):
    mixer = small_mixer()
    b, Q = 3, 64
    l = 5 * Q
    h, p, g, n = mixer.nheads, mixer.headdim, mixer.ngroups, mixer.d_state
    torch.manual_seed(1)
    x, z = randn(b, l, h * p, scale=0.5), randn(b, l, h * p)
    dt, B, C = randn(b, l, h), randn(b, l, g * n), randn(b, l, g * n)
    doc = ()
    if masked:
        dm = mask_of(ssd_rows(Q), l)
        doc = (dm.start, dm.end)

    def run(mode):
        old = ops.ssd_state_chain("fused"), ops.ssd_yoff_mode(mode)
        try:
            leaves = [t.clone().requires_grad_() for t in (x, dt, B, C)]
            xi, dti, Bi, Ci = leaves
            n0 = ext().ssd_yoff_calls()
            out = mixer._scan_fused(b, l, xi, dti, z, Bi, Ci, mixer.dt_bias,
                                    mixer.A_log, mixer.D, *doc)
            gr = torch.autograd.grad(out.float().pow(2).mean(),
                                     leaves + [mixer.A_log])
            return out.detach(), gr, ext().ssd_yoff_calls() - n0
        finally:
            ops.ssd_state_chain(old[0])
            ops.ssd_yoff_mode(old[1])
    o_g, g_g, calls_g = run("gemm")
    o_f, g_f, calls_f = run("fused")
    assert calls_g == 0 and calls_f == 2
    assert relerr(o_f, o_g) < 3e-2, relerr(o_f, o_g)
    for nm, a, r in zip(("x", "dt", "B", "C"), g_f, g_g):
        assert relerr(a, r) < 6e-2, (nm, relerr(a, r))
    assert relerr(g_f[4], g_g[4]) < 8e-2, relerr(g_f[4], g_g[4])


def test_binding_rejects_bad_arguments():
    N, P, Q, H, G, bc = 16, 32, 32, 4, 2, 2
    dims = (H, G, P, N, Q)
    C, prev = randn(bc * Q, G * N), randn(bc * H, N, P)
    dyoff = randn(bc, G, Q, H // G, P)
    wide = randn(bc * Q, G * N + 8)
    bad_fwd = [
        (C.float(), prev.float()) + dims,
        (C, randn(bc * H, N, 2 * P)[..., :P]) + dims,
        (C, prev[1:]) + dims,
        (randn(bc * Q, G * 48), randn(bc * H, 48, P), H, G, P, 48, Q),
        (randn(bc * 48, G * N), prev, H, G, P, N, 48),
        (wide[:, 4:4 + G * N], prev) + dims,
        (C.cpu(), prev.cpu()) + dims,
    ]
    bad_bwd = [(dyoff,) + a for a in bad_fwd] + [
        (dyoff.float(), C, prev) + dims,
        (dyoff[1:], C, prev) + dims,
        (dyoff, C, prev) + dims + (H // G + 1,),
    ]
    n0 = ext().ssd_yoff_calls()
    for fn, bad in ((ext().ssd_yoff_fwd, bad_fwd),
                    (ext().ssd_yoff_bwd, bad_bwd)):
        for args in bad:
            with pytest.raises(RuntimeError):
                fn(*args)
    assert ext().ssd_yoff_fwd(C[:0], prev[:0], *dims).numel() == 0
    dCp, dprev = ext().ssd_yoff_bwd(dyoff[:0], C[:0], prev[:0], *dims)
    assert dCp.shape[1:] == (0, G * N) and dprev.numel() == 0
    assert ext().ssd_yoff_calls() == n0
