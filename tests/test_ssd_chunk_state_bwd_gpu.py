"""The chunk-state backward kernel (ops/hip/ssd_state_bwd.hip) against the
float64 gradients of reference.ssd_chunk_state on the same bf16 inputs,
under tests/oracle_rule.py, then through ops.ssd_chunk_state and the training
scan under ops.ssd_chunk_state_backward("fused").

Both outputs are fp32 sums of exact products of bf16 inputs, rounded to bf16
once (dB after the sum of its head-block partials): R = 2^-8, A = A_REDUCE,
mag = the same gradient at |B|, |xdtd|, |dS|, nothing widened."""

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_mamba_decode_gpu import relerr
from test_ssd_docmask_gpu import mask_of, same_bits, ssd_rows
from test_ssd_kernels_gpu import col_slice, dev, ext, randn
from test_ssd_state_gpu import small_mixer

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
A_RED = rule.A_REDUCE

# single-wave block, block with idle waves, two row blocks; the padded N;
# rep = 3; then the uneven head-block tail and the partial sum
CASES = [(N, P, Q, H, G, 3, 0) for N, P in [(16, 32), (64, 64), (128, 64)]
         for Q in (32, 96, 256) for H, G in [(4, 1), (6, 2)]] \
    + [(128, 64, 32, 21, 1, 2, hb) for hb in (1, 2, 21)] \
    + [(16, 32, 32, 6, 2, 3, hb) for hb in (1, 2, 3)]


def oracle(B, xdtd, dS, dims):
    """float64 (dB, dxdtd) and their sums of |terms|."""
    def grads(f):
        Bd, xd = (f(t.double()).requires_grad_() for t in (B, xdtd))
        S = reference.ssd_chunk_state(Bd, xd, *dims)
        return torch.autograd.grad(S, (Bd, xd), f(dS.double()))
    return grads(lambda t: t), grads(torch.abs)


def check_grads(tag, dB, dxdtd, B, xdtd, dS, dims):
    ref, mag = oracle(B, xdtd, dS, dims)
    assert dB.dtype == BF and dxdtd.dtype == BF
    rule.check("ssd_chunk_state_bwd.dB" + tag, dB, ref[0], mag[0], A_RED)
    rule.check("ssd_chunk_state_bwd.dxdtd" + tag, dxdtd, ref[1], mag[1], A_RED)


@pytest.mark.parametrize("N,P,Q,H,G,bc,hb", CASES)
def test_chunk_state_bwd(N, P, Q, H, G, bc, hb):
    torch.manual_seed(N + P + Q + H + hb)
    B = col_slice(bc * Q, G * N)
    assert B.stride(0) > G * N
    xdtd, dS = randn(bc * H, Q, P), randn(bc * H, N, P)
    n0 = ext().ssd_chunk_state_bwd_calls()
    dBp, dxdtd = ext().ssd_chunk_state_bwd(dS, B, xdtd, H, G, P, N, Q, hb)
    assert ext().ssd_chunk_state_bwd_calls() == n0 + 1
    assert dBp.dtype == torch.float32 and dBp.shape[1:] == (bc * Q, G * N)
    assert dBp.shape[0] == hb or hb == 0
    assert dxdtd.shape == xdtd.shape
    check_grads(f"[N={N},P={P},Q={Q},H={H},G={G},bc={bc},hb={hb}]",
                dBp.sum(0).to(BF), dxdtd, B, xdtd, dS, (H, G, P, N, Q))
    again = ext().ssd_chunk_state_bwd(dS, B, xdtd, H, G, P, N, Q, hb)
    assert same_bits(again[0], dBp) and same_bits(again[1], dxdtd)


def test_through_the_op():
    N, P, Q, H, G, bc = 64, 64, 96, 6, 2, 3
    torch.manual_seed(5)
    B, xdtd = col_slice(bc * Q, G * N), randn(bc * H, Q, P)
    dS = randn(bc * H, N, P)

    def run(mode):
        prev = ops.ssd_chunk_state_backward(mode)
        try:
            assert ops.ssd_chunk_state_backward() == mode
            Bi, xi = B.detach().requires_grad_(), xdtd.clone().requires_grad_()
            n0 = ext().ssd_chunk_state_bwd_calls(), ext().ssd_state_calls()
            S = ops.ssd_chunk_state(Bi, xi, H, G, P, N, Q)
            gr = torch.autograd.grad(S, (Bi, xi), dS)
            return gr, (ext().ssd_chunk_state_bwd_calls() - n0[0],
                        ext().ssd_state_calls() - n0[1])
        finally:
            assert ops.ssd_chunk_state_backward(prev) == mode
    (dB, dxdtd), calls = run("fused")
    assert calls == (1, 1)
    assert dB.shape == B.shape and dxdtd.shape == xdtd.shape
    check_grads("[op]", dB, dxdtd, B, xdtd, dS, (H, G, P, N, Q))
    assert run("gemm")[1] == (0, 1)
    with pytest.raises(ValueError):
        ops.ssd_chunk_state_backward("einsum")


@pytest.mark.parametrize("masked", [False, True])
def test_training_scan_fused_bwd_matches_gemm(masked):
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
        prev = ops.ssd_state_chain("fused"), ops.ssd_chunk_state_backward(mode)
        try:
            leaves = [t.clone().requires_grad_() for t in (x, dt, B, C)]
            xi, dti, Bi, Ci = leaves
            n0 = ext().ssd_chunk_state_bwd_calls()
            out = mixer._scan_fused(b, l, xi, dti, z, Bi, Ci, mixer.dt_bias,
                                    mixer.A_log, mixer.D, *doc)
            gr = torch.autograd.grad(out.float().pow(2).mean(),
                                     leaves + [mixer.A_log])
            return out.detach(), gr, ext().ssd_chunk_state_bwd_calls() - n0
        finally:
            ops.ssd_state_chain(prev[0])
            ops.ssd_chunk_state_backward(prev[1])
    o_g, g_g, calls_g = run("gemm")
    o_f, g_f, calls_f = run("fused")
    assert calls_g == 0 and calls_f == 1
    assert relerr(o_f, o_g) < 3e-2, relerr(o_f, o_g)
    for nm, a, r in zip(("x", "dt", "B", "C"), g_f, g_g):
        assert relerr(a, r) < 6e-2, (nm, relerr(a, r))
    assert relerr(g_f[4], g_g[4]) < 8e-2, relerr(g_f[4], g_g[4])


def test_binding_rejects_bad_arguments():
    N, P, Q, H, G, bc = 16, 32, 32, 4, 2, 2
    B, xdtd, dS = randn(bc * Q, G * N), randn(bc * H, Q, P), randn(bc * H, N, P)
    wide = randn(bc * Q, G * N + 8)
    bad = [
        (dS.float(), B, xdtd, H, G, P, N, Q),
        (dS, B, randn(bc * H, Q, 2 * P)[..., :P], H, G, P, N, Q),
        (dS[1:], B, xdtd, H, G, P, N, Q),
        (dS, B, xdtd, H, G, P, N, Q, H // G + 1),
        (randn(bc * H, 48, P), randn(bc * Q, G * 48), xdtd, H, G, P, 48, Q),
        (dS, randn(bc * 48, G * N), randn(bc * H, 48, P), H, G, P, N, 48),
        (dS, wide[:, 4:4 + G * N], xdtd, H, G, P, N, Q),
        (dS.cpu(), B.cpu(), xdtd.cpu(), H, G, P, N, Q),
    ]
    n0 = ext().ssd_chunk_state_bwd_calls()
    for args in bad:
        with pytest.raises(RuntimeError):
            ext().ssd_chunk_state_bwd(*args)
    assert ext().ssd_chunk_state_bwd_calls() == n0
    dBp, dxdtd = ext().ssd_chunk_state_bwd(dS[:0], B[:0], xdtd[:0], H, G, P,
                                           N, Q)
    assert dBp.shape[1:] == (0, G * N) and dxdtd.numel() == 0
    assert ext().ssd_chunk_state_bwd_calls() == n0
