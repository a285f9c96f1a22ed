"""The fused intra-chunk SSD kernel (ops/hip/ssd_diag.hip) against
reference.ssd_diag in float64 on the same bf16 inputs, under the rule of
tests/oracle_rule.py: |got - ref| <= R|ref| + A*mag for every element with
R = 2^-8 (the output rounding), A = 2^-9 + A_REDUCE (the allowance for one
bf16 rounding of each sL term before the second MFMA, plus the fp32
reductions; the kernel carries the rounding's remainder as well) and
mag[i,p] = sum_j (sum_n |C_in B_jn|) L_ij |xdt_jp|. A masked term leaves mag
too, so where the oracle is 0 the rule demands exact 0."""

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_ssd_docmask_gpu import (later_positions, mask_of, pos_hmajor,
                                  relerr, same_bits, sel_hmajor, ssd_rows)
from test_ssd_kernels_gpu import col_slice, dev, ext, make_dacs, randn

pytestmark = pytest.mark.gpu

A_DIAG = 2.0 ** -9 + rule.A_REDUCE


def make_case(Q, N, P, H, G, bc=3):
    """C/B strided slices (16-byte aligned, row stride > G*N), decays
    spanning e^-0.5 .. e^-30 inside a chunk, xdt h-major."""
    C, B = col_slice(bc * Q, G * N), col_slice(bc * Q, G * N)
    assert C.stride(0) > G * N and C.data_ptr() % 16 == 0
    return C, B, make_dacs(bc * H, Q), randn(bc * H, Q, P)


def check(name, got, C, B, dacs, xdt, dims, dm=None):
    d64 = [t.double() for t in (C, B, dacs, xdt)]
    ref = reference.ssd_diag(*d64, *dims, doc_mask=dm)
    mag = reference.ssd_diag(d64[0].abs(), d64[1].abs(), d64[2], d64[3].abs(),
                             *dims, doc_mask=dm)
    return rule.check(name, got, ref, mag, A_DIAG)


@pytest.mark.parametrize("H,G", [(4, 1), (6, 2)])
@pytest.mark.parametrize("N,P", [(16, 32), (16, 64), (128, 32), (128, 64)])
@pytest.mark.parametrize("Q", [64, 128, 256])
def test_ssd_diag_oracle(Q, N, P, H, G):
    """Worst err/tol on an MI355X: 0.24 .. 0.59 (docs/kernels.md)."""
    torch.manual_seed(Q + N + P + H)
    C, B, dacs, xdt = make_case(Q, N, P, H, G)
    dims = (H, G, P, N, Q)
    got = ext().ssd_diag_fwd(C, B, dacs, xdt, *dims)
    assert got.shape == (3 * H, Q, P)
    check(f"ssd_diag[Q={Q},N={N},P={P},H={H},G={G}]", got, C, B, dacs, xdt,
          dims)


def test_ssd_diag_overflow_above_diagonal():
    """dacs falls by more than 100 across the chunk: exp(cs_i - cs_j) is inf
    for many j > i; the select must leave a finite result inside the rule."""
    torch.manual_seed(7)
    dims = (4, 1, 64, 128, 128)
    C, B, dacs, xdt = make_case(128, 128, 64, 4, 1)
    dacs = (dacs * 40).contiguous()
    assert (dacs[:, 0] - dacs[:, -1]).max() > 100
    assert torch.isinf(torch.exp(dacs[:, :1] - dacs[:, -1:])).any()
    got = ext().ssd_diag_fwd(C, B, dacs, xdt, *dims)
    assert torch.isfinite(got).all()
    check("ssd_diag[overflow]", got, C, B, dacs, xdt, dims)


@pytest.mark.parametrize("Q,N,P", [(64, 16, 32), (128, 128, 64)])
def test_ssd_diag_doc(Q, N, P):
    torch.manual_seed(Q)
    H, G, b, nc = 6, 2, 3, 5
    l, dims = nc * Q, (H, G, P, N, Q)
    dm = mask_of(ssd_rows(Q), l)
    C, B, dacs, xdt = make_case(Q, N, P, H, G, bc=b * nc)
    got = ext().ssd_diag_fwd_doc(C, B, dacs, xdt, *dims, dm.start, l)
    check(f"ssd_diag_doc[Q={Q}]", got, C, B, dacs, xdt, dims, dm)
    assert same_bits(ops.ssd_diag(C, B, dacs, xdt, *dims, doc_mask=dm), got)
    # one document per row: the unmasked kernel's bits
    one = mask_of([[0]] * b, l)
    assert same_bits(
        ext().ssd_diag_fwd_doc(C, B, dacs, xdt, *dims, one.start, l),
        ext().ssd_diag_fwd(C, B, dacs, xdt, *dims))
    # large finite values all over the first documents move no bit of a
    # later document
    later = later_positions(ssd_rows(Q), l)
    big = torch.full((), 1e30, device=dev(), dtype=torch.bfloat16)
    C2 = torch.where(later[:, None], C, big)
    B2 = torch.where(later[:, None], B, -big)
    x2 = torch.where(sel_hmajor(later, H, Q, P).view_as(xdt), xdt, big)
    got2 = ext().ssd_diag_fwd_doc(C2, B2, dacs, x2, *dims, dm.start, l)

    def by_pos(t):
        return pos_hmajor(t.view(b * l, H * P), H, Q, P)[later]
    assert same_bits(by_pos(got2), by_pos(got))
    assert not same_bits(got2, got)


def test_ssd_diag_views_and_determinism():
    torch.manual_seed(3)
    dims = (6, 2, 64, 128, 256)
    C, B, dacs, xdt = make_case(256, 128, 64, 6, 2)
    a = ext().ssd_diag_fwd(C, B, dacs, xdt, *dims)
    assert same_bits(ext().ssd_diag_fwd(C, B, dacs, xdt, *dims), a)
    assert same_bits(ext().ssd_diag_fwd(C.contiguous(), B.contiguous(), dacs,
                                        xdt, *dims), a)


@pytest.mark.parametrize("Q,N,P,H", [(64, 16, 32, 4), (128, 128, 64, 80)])
def test_ssd_diag_backward_is_the_gemm_route(Q, N, P, H, monkeypatch):
    """The fused op's backward runs the three-launch route's own library
    calls on the same values: every gradient has that route's bits."""
    torch.manual_seed(Q)
    G, bc = 1, 2
    dims = (H, G, P, N, Q)
    C, B, dacs, xdt = make_case(Q, N, P, H, G, bc=bc)
    dy = randn(bc * H, Q, P)

    def grads(route):
        monkeypatch.setenv("FMS_AMD_SSD_DIAG", route)
        leaves = [t.clone().requires_grad_() for t in (C, B, dacs, xdt)]
        n0 = ext().ssd_diag_calls()
        y = ops.ssd_diag(*leaves, *dims)
        assert ext().ssd_diag_calls() - n0 == (route == "fused")
        return torch.autograd.grad(y, leaves, dy)
    for nm, a, r in zip(("dC", "dB", "ddacs", "dxdt"), grads("fused"),
                        grads("gemm")):
        assert same_bits(a, r), nm


def test_ssd_diag_bindings_reject_bad_arguments():
    fwd, Q = ext().ssd_diag_fwd, 64
    C, B, dacs, xdt = make_case(Q, 16, 32, 4, 1)
    dims = (4, 1, 32, 16, Q)
    wide = randn(3 * Q, 64)
    dm = mask_of([[0]] * 3, Q)
    bad = [
        (C, B, dacs, xdt, 4, 1, 32, 48, Q),               # N unsupported
        (C, B, dacs, xdt, 4, 1, 16, 16, Q),               # P unsupported
        (C, B, dacs, xdt, 4, 1, 32, 16, 48),              # Q % 32
        (C, B, dacs, xdt, 4, 3, 32, 16, Q),               # H % G
        (wide[:, 4:20], B, dacs, xdt, *dims),             # misaligned slice
        (wide[:, ::2][:, :16], B, dacs, xdt, *dims),      # last stride 2
        (C.float(), B, dacs, xdt, *dims),
        (C, B, dacs.double(), xdt, *dims),
        (C, B, dacs.t().contiguous().t(), xdt, *dims),
        (C, B, dacs, xdt.transpose(1, 2), *dims),
        (C, B[:Q], dacs, xdt, *dims),
        (C, B, dacs, xdt[:, :, :16].contiguous(), *dims),
        (C, B, dacs, xdt.cpu(), *dims),
    ]
    n0 = ext().ssd_diag_calls()
    for args in bad:
        with pytest.raises(RuntimeError):
            fwd(*args)
    with pytest.raises(RuntimeError):                     # short doc_start
        ext().ssd_diag_fwd_doc(C, B, dacs, xdt, *dims,
                               dm.start.reshape(-1)[:-1], Q)
    with pytest.raises(RuntimeError):                     # l not a row length
        ext().ssd_diag_fwd_doc(C, B, dacs, xdt, *dims, dm.start, Q + 32)
    assert ext().ssd_diag_calls() == n0
    torch.cuda.synchronize()


def test_mixer_runs_the_fused_diag(monkeypatch):
    """Mamba2Mixer (headdim 32, d_state 16, chunk 64), forward and backward
    under both routes: each within the tolerance of
    test_ops_gpu.test_ssd_fused_scan_matches_torch against the torch scan,
    and only the fused route launches the kernel."""
    from fms_fsdp_amd.models.mamba import Mamba2Mixer, MambaConfig
    torch.manual_seed(0)
    cfg = MambaConfig(d_model=128, n_layer=1, vocab_size=512, d_state=16,
                      headdim=32, expand=2, ngroups=2, chunk_size=64)
    mixer = Mamba2Mixer(cfg, 0)
    mixer.reset_parameters()
    mixer = mixer.to(dev()).bfloat16()
    u = torch.randn(2, 192, 128, device=dev(), dtype=torch.bfloat16) * 0.5

    def run(route, force_torch=False):
        monkeypatch.setenv("FMS_AMD_SSD_DIAG", route)
        mixer._force_torch_scan = force_torch
        ui = u.clone().requires_grad_()
        n0 = ext().ssd_diag_calls()
        out = mixer(ui)
        (gu,) = torch.autograd.grad(out.float().pow(2).mean(), ui)
        return out.detach(), gu, ext().ssd_diag_calls() - n0
    o_t, gu_t, _ = run("fused", force_torch=True)
    for route in ("fused", "gemm"):
        o, gu, calls = run(route)
        assert (calls > 0) == (route == "fused"), (route, calls)
        assert relerr(o, o_t) < 3e-2, (route, relerr(o, o_t))
        assert relerr(gu, gu_t) < 6e-2, (route, relerr(gu, gu_t))
