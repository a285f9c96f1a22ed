"""The fused backward of the intra-chunk SSD term (ops/hip/ssd_diag_bwd.hip)
against reference.ssd_diag in float64 on the same bf16 inputs, differentiated
by autograd with a random bf16 dy, under the rule of tests/oracle_rule.py.

dxdt, dC, dB (bf16): R = 2^-8, A = 2^-8 + A_REDUCE: every term passes one
bf16 rounding of an MFMA operand (M, or one head's dS; half a bf16 ulp is at
most 2^-8 relative), the rest is fp32 reduction. mag is the same gradient at
|C|, |B|, dacs, |xdt| with |dy|: all its terms are non-negative, so it is the
sum of the absolute terms. ddacs (fp32): R = 0, A = A_REDUCE, mag[n,i] =
sum_j |Gm|[i,j] + sum_i' |Gm|[i',i]. Where the mask makes the oracle 0 the
rule demands exact 0. Worst err/tol on an MI355X: docs/kernels.md."""

import functools

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_ssd_diag_gpu import make_case
from test_ssd_docmask_gpu import mask_of, same_bits, ssd_rows
from test_ssd_kernels_gpu import ext, randn

pytestmark = pytest.mark.gpu

A_BF16 = 2.0 ** -8 + rule.A_REDUCE
NAMES = ("dC", "dB", "ddacs", "dxdt")


def grads64(C, B, dacs, xdt, dy, dims, dm):
    leaves = [t.detach().clone().requires_grad_() for t in (C, B, dacs, xdt)]
    y = reference.ssd_diag(*leaves, *dims, doc_mask=dm)
    return torch.autograd.grad(y, leaves, dy.reshape(y.shape))


@functools.lru_cache(maxsize=None)
def case(Q, N, P, H, G, bc=3, scale=1.0, nc=0):
    """Inputs, dy and the float64 oracle of one shape: (ref, mag) per output.
    nc > 0: bc = 3 rows of nc chunks under the mask of ssd_rows(Q)."""
    torch.manual_seed(Q + N + P + H + bc)
    dims = (H, G, P, N, Q)
    dm = mask_of(ssd_rows(Q), nc * Q) if nc else None
    C, B, dacs, xdt = make_case(Q, N, P, H, G, bc=bc)
    dacs = (dacs * scale).contiguous()
    dy = randn(bc * H, Q, P)
    c64, b64, cs64, x64, dy64 = (t.double() for t in (C, B, dacs, xdt, dy))
    ref = grads64(c64, b64, cs64, x64, dy64, dims, dm)
    mag = list(grads64(c64.abs(), b64.abs(), cs64, x64.abs(), dy64.abs(),
                       dims, dm))
    ones = torch.ones(bc * G, Q, Q, dtype=torch.float64, device=C.device)
    L = reference.ssd_scores_decay(cs64, ones, H, G, dm).view(bc, H, Q, Q)
    s = torch.einsum("cign,cjgn->cgij", c64.abs().view(bc, Q, G, N),
                     b64.abs().view(bc, Q, G, N))
    a = torch.einsum("chip,chjp->chij", dy64.abs().view(bc, H, Q, P),
                     x64.abs().view(bc, H, Q, P))
    gm = a * s.repeat_interleave(H // G, dim=1) * L
    mag[2] = (gm.sum(3) + gm.sum(2)).view(bc * H, Q)
    return (C, B, dacs, xdt), dy, dims, dm, ref, mag


def run(k, head_blocks=0):
    inp, dy, dims, dm, _, _ = k
    if dm is None:
        return ext().ssd_diag_bwd(dy, *inp, *dims, head_blocks)
    return ext().ssd_diag_bwd_doc(dy, *inp, *dims, dm.start,
                                  dm.start.shape[-1], head_blocks)


def judge(name, got, k):
    """got = (dC, dB, ddacs, dxdt), dC / dB already summed and cast."""
    ref, mag = k[4], k[5]
    for nm, t, r, m in zip(NAMES, got, ref, mag):
        rule.check(f"{name}.{nm}", t, r.reshape(t.shape), m.reshape(t.shape),
                   rule.A_REDUCE if nm == "ddacs" else A_BF16)


def reduced(out):
    dCp, dBp, ddacs, dxdt = out
    return (dCp.sum(0).to(torch.bfloat16), dBp.sum(0).to(torch.bfloat16),
            ddacs, dxdt)


@pytest.mark.parametrize("H,G,head_blocks", [(3, 1, 2), (6, 2, 1), (6, 2, 3)])
@pytest.mark.parametrize("N,P", [(16, 32), (128, 64)])
@pytest.mark.parametrize("Q", [32, 96, 256])
def test_ssd_diag_bwd_oracle(Q, N, P, H, G, head_blocks):
    k = case(Q, N, P, H, G)
    out = run(k, head_blocks)
    assert out[0].shape == (head_blocks, 3 * Q, G * N)
    assert out[0].dtype == torch.float32 and out[2].dtype == torch.float32
    judge(f"ssd_diag_bwd[Q={Q},N={N},P={P},H={H},G={G},nhb={head_blocks}]",
          reduced(out), k)


def test_ssd_diag_bwd_overflow_on_the_masked_side():
    """dacs falls by more than 100 across the chunk: exp(cs_i - cs_j) is inf
    for many j > i, in the registers of both passes."""
    k = case(128, 128, 64, 4, 1, scale=40.0)
    dacs = k[0][2]
    assert torch.isinf(torch.exp(dacs[:, :1] - dacs[:, -1:])).any()
    got = reduced(run(k))
    assert all(torch.isfinite(t).all() for t in got)
    judge("ssd_diag_bwd[overflow]", got, k)


@pytest.mark.parametrize("Q,N,P", [(64, 16, 32), (128, 128, 64)])
def test_ssd_diag_bwd_doc(Q, N, P):
    k = case(Q, N, P, 6, 2, bc=15, nc=5)
    inp, dy, dims, dm = k[:4]
    judge(f"ssd_diag_bwd_doc[Q={Q}]", reduced(run(k)), k)
    # one document per row: the unmasked kernel's bits
    one = mask_of([[0]] * 3, 5 * Q)
    for a, b in zip(ext().ssd_diag_bwd_doc(dy, *inp, *dims, one.start, 5 * Q),
                    ext().ssd_diag_bwd(dy, *inp, *dims)):
        assert same_bits(a, b)


def test_ssd_diag_bwd_views_and_determinism():
    k = case(256, 128, 64, 6, 2)
    (C, B, dacs, xdt), dy, dims = k[:3]
    assert not C.is_contiguous()
    a = run(k)
    for b in (run(k), ext().ssd_diag_bwd(dy, C.contiguous(), B.contiguous(),
                                         dacs, xdt, *dims)):
        assert all(same_bits(x, y) for x, y in zip(a, b))


def test_ssd_diag_bwd_through_the_op():
    k = case(96, 128, 64, 6, 2)
    inp, dy, dims = k[:3]

    def grads():
        leaves = [t.clone().requires_grad_() for t in inp]
        n0 = ext().ssd_diag_bwd_calls()
        got = torch.autograd.grad(ops.ssd_diag(*leaves, *dims), leaves, dy)
        return got, ext().ssd_diag_bwd_calls() - n0
    prev = ops.ssd_diag_backward("fused")
    try:
        assert ops.ssd_diag_backward() == "fused"
        got, calls = grads()
    finally:
        assert ops.ssd_diag_backward(prev) == "fused"
    assert calls == 1
    assert [t.dtype for t in got] == [t.dtype for t in inp]
    judge("ssd_diag_bwd[op]", got, k)
    assert grads()[1] == (prev == "fused")


def test_ssd_diag_bwd_bindings_reject_bad_arguments():
    Q = 64
    (C, B, dacs, xdt), dy, dims = case(Q, 16, 32, 4, 1)[:3]
    bad = [
        (dy, C, B, dacs, xdt, 4, 1, 32, 48, Q),               # N unsupported
        (dy, C, B, dacs, xdt, 4, 1, 32, 16, 48),              # Q % 32
        (dy, C, B, dacs, xdt, *dims, 5),                      # nhb > H/G
        (dy, C, B, dacs, xdt, *dims, -1),
        (dy[:, :, :16].contiguous(), C, B, dacs, xdt, *dims),
        (dy.view(-1, Q * 32), C, B, dacs, xdt, *dims),
        (dy.transpose(1, 2), C, B, dacs, xdt, *dims),
        (dy.float(), C, B, dacs, xdt, *dims),
        (dy.cpu(), C, B, dacs, xdt, *dims),
        (dy, C, B[:Q], dacs, xdt, *dims),
    ]
    n0 = ext().ssd_diag_bwd_calls()
    for args in bad:
        with pytest.raises(RuntimeError):
            ext().ssd_diag_bwd(*args)
    assert ext().ssd_diag_bwd_calls() == n0
    torch.cuda.synchronize()
