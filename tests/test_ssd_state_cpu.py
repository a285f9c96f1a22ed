"""The oracles of ops/hip/ssd_state.hip on the CPU, in float64.

reference.ssd_chunk_state and reference.ssd_state_pass, composed with the
other oracles exactly as Mamba2Mixer._scan_fused composes the kernels under
ops.ssd_state_chain("fused"), against the W-matrix formulation (the
composition test_ssd_docmask_cpu.py ties to the recurrence), masked and
unmasked: this pins the scan form keep_c of the select doc_chunk_keep
applies to W. Then, from a random initial state, against the token-by-token
recurrence reference.ssd_state_update."""

import pytest
import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_ssd_docmask_cpu import scan_from_oracles_doc, starts_to_doc_start

DD = torch.float64


def scan_state_pass(b, l, x, dt, z, B, C, dtb, Alog, D_, h, p, g, n, Q,
                    doc_mask=None, initial_state=None):
    """_scan_fused's fused state chain over the oracles -> (out, final)."""
    nc, rep = l // Q, h // g
    dt2, x2, z2 = (t.reshape(b * l, -1) for t in (dt, x, z))
    dtf, dacs = reference.ssd_prep(dt2, dtb, Alog, Q)
    xdt, xdtd = reference.ssd_xdt(x2, dtf, dacs, h, p, Q, doc_mask)
    B2, C2 = B.reshape(b * l, g * n), C.reshape(b * l, g * n)
    y_diag = reference.ssd_diag(C2, B2, dacs, xdt, h, g, p, n, Q, doc_mask)
    states = reference.ssd_chunk_state(B2, xdtd, h, g, p, n, Q)
    prev, final = reference.ssd_state_pass(
        states, dacs, b, h, p, n, Q, doc_mask, initial_state, True)
    y_off = torch.einsum("bcqgn,bcgrnp->bcgqrp", C.reshape(b, nc, Q, g, n),
                         prev.view(b, nc, g, rep, n, p))
    out = reference.ssd_ygate(
        y_diag.reshape(b * l, h * p), y_off.reshape(b * l, h * p), dacs, x2,
        D_, z2, h, g, p, Q, doc_mask)
    return out.view(b, l, h * p), final


def inputs(b, l, h, p, g, n):
    torch.manual_seed(0)
    r = lambda *s, scale=1.0: torch.randn(*s, dtype=DD) * scale
    # |A| from 0.02 to 4: the slow heads carry state across all the chunks
    return (r(b, l, h * p), r(b, l, h, scale=2.0), r(b, l, h * p),
            r(b, l, g * n), r(b, l, g * n), r(h),
            torch.linspace(-4.0, 1.4, h, dtype=DD), r(h))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Q,h,g,p", [(64, 6, 2, 8), (16, 4, 4, 8),
                                     (32, 4, 1, 16)])
def test_state_pass_equals_the_w_matrix(Q, h, g, p, masked):
    b, n, nc = 3, 16, 5
    l = nc * Q
    # a boundary on a chunk start, one mid-chunk, a document over two whole
    # chunks that ends on a chunk's last token, two one-token documents,
    # one document
    rows = [[0, 1, 2, Q], [0, Q + 5, 4 * Q - 1], [0]] if masked else [[0]] * 3
    dm = ops.doc_mask_from_starts(starts_to_doc_start(rows, l))
    args = inputs(b, l, h, p, g, n)
    got, _ = scan_state_pass(b, l, *args, h, p, g, n, Q,
                             dm if masked else None)
    ref = scan_from_oracles_doc(b, l, *args, h, p, g, n, Q, dm)
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("Q,h,g,p", [(16, 4, 2, 8), (32, 4, 1, 16)])
def test_state_pass_from_an_initial_state_equals_the_recurrence(Q, h, g, p):
    b, n, nc = 2, 16, 3
    l = nc * Q
    x, dt, z, B, C, dtb, Alog, D_ = inputs(b, l, h, p, g, n)
    init = torch.randn(b, h, p, n, dtype=DD)
    got, final = scan_state_pass(b, l, x, dt, z, B, C, dtb, Alog, D_, h, p,
                                 g, n, Q, initial_state=init)
    state = init.clone()
    ref = reference.ssd_state_update(state, x, dt, B, C, z, dtb, Alog, D_, h,
                                     g, p, n)
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(final, state, rtol=1e-9, atol=1e-12)
    # the initial state matters at this tolerance
    zero, _ = scan_state_pass(b, l, x, dt, z, B, C, dtb, Alog, D_, h, p, g,
                              n, Q)
    assert (zero - ref).abs().max() > 1e-3
    with pytest.raises(ValueError):
        reference.ssd_state_pass(
            torch.zeros(b * nc * h, n, p, dtype=DD),
            torch.zeros(b * nc * h, Q, dtype=DD), b, h, p, n, Q,
            ops.doc_mask_from_starts(torch.zeros(b, l, dtype=torch.int64)),
            init)


@pytest.mark.parametrize("chunk,h,g", [(16, 4, 2), (32, 4, 1)])
def test_ssd_chunked_from_an_initial_state_equals_the_recurrence(chunk, h, g):
    """The torch scan (fp32 math) from a carried state against the float64
    token-by-token recurrence, output and final state."""
    from fms_fsdp_amd.models.mamba import ssd_chunked
    torch.manual_seed(0)
    b, p, n, l = 2, 8, 16, 3 * chunk
    x, B, C = (torch.randn(b, l, d) for d in (h * p, g * n, g * n))
    dt = torch.rand(b, l, h) * 0.5
    A = -torch.rand(h) * 2
    init = torch.randn(b, h, p, n)
    y, final = ssd_chunked(x.view(b, l, h, p), dt, A, B.view(b, l, g, n),
                           C.view(b, l, g, n), chunk, return_final_state=True,
                           initial_state=init)
    S = init.double().transpose(-1, -2)                        # (b, h, n, p)
    rep, ys = h // g, []
    Bh = B.view(b, l, g, n).repeat_interleave(rep, 2).double()
    Ch = C.view(b, l, g, n).repeat_interleave(rep, 2).double()
    for t in range(l):
        a = torch.exp(dt[:, t].double() * A.double())[:, :, None, None]
        S = a * S + torch.einsum("bhn,bhp->bhnp",
                                 Bh[:, t] * dt[:, t, :, None].double(),
                                 x.view(b, l, h, p)[:, t].double())
        ys.append(torch.einsum("bhn,bhnp->bhp", Ch[:, t], S))
    ref = torch.stack(ys, 1)
    assert (y - ref).abs().max() / ref.abs().max() < 1e-4
    assert (final - S.transpose(-1, -2)).abs().max() / S.abs().max() < 1e-4


def test_cached_mixer_continues_a_used_cache_through_the_chunked_scan():
    """16 + 3 tokens on a fresh cache, then 16 + 2 on the used one."""
    from fms_fsdp_amd.models.mamba import Mamba2Mixer, MambaConfig
    torch.manual_seed(0)
    cfg = MambaConfig(d_model=32, n_layer=1, vocab_size=64, d_state=16,
                      headdim=8, chunk_size=16)
    mixer = Mamba2Mixer(cfg, 0)
    mixer.reset_parameters()
    mixer = mixer.double().eval()
    u = torch.randn(2, 37, 32, dtype=DD)

    def cache():
        return ops.MambaCache(2, mixer.conv_dim, mixer.d_conv, mixer.nheads,
                              mixer.headdim, mixer.d_state, DD, "cpu")
    with torch.no_grad():
        whole_c, split_c = cache(), cache()
        whole = mixer(u, cache=whole_c)
        split = torch.cat([mixer(u[:, :19], cache=split_c),
                           mixer(u[:, 19:], cache=split_c)], dim=1)
    # ssd_chunked computes in fp32
    torch.testing.assert_close(split, whole, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(split_c.ssm, whole_c.ssm, rtol=1e-4, atol=1e-5)
