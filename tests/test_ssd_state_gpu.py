"""The inter-chunk state kernels (ops/hip/ssd_state.hip) against their
float64 oracles on the same bf16 inputs, under tests/oracle_rule.py; then
the two routes they open: a prompt prefilled in pieces over a used cache,
and the training scan under ops.ssd_state_chain("fused").

state pass forward: `mag` follows the recurrence m_c = a_c m_{c-1} + |S_c|,
m_{-1} = |initial_state|. The one second effect is the compounded error of
a_c = __expf(G_c), ssd_step's term (docs/kernels.md, "Error rule" of
ssd_step.hip) with what exists here: G_c is an exact input, so the relative
error of a_c is d_c = (|G_c| + 2) 2^-23 (1: __expf's scaling of its
argument by log2 e; 2: v_exp_f32's result and the fma), S_c is exact, and
E_c = a_c (E_{c-1} + d_c m_{c-1}) widens mag. R and A are never raised."""

import os
import subprocess
import sys

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_mamba_decode_gpu import FWD_TOL, relerr
from test_ssd_docmask_gpu import mask_of, same_bits, ssd_rows
from test_ssd_kernels_gpu import col_slice, dev, ext, make_dacs, randn

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
A_RED = rule.A_REDUCE
U = 2.0 ** -23


# bc = 3 plans one head per workgroup; the last two rows plan two, with a
# one-head tail block: the head loop over the held B^T fragments.
CS_CASES = [(N, P, Q, H, G, 3) for N, P in [(16, 32), (64, 64), (128, 64)]
            for Q in (32, 96, 256) for H, G in [(4, 1), (6, 2)]] \
    + [(16, 32, 32, 6, 2, 128), (128, 64, 32, 21, 1, 64)]


@pytest.mark.parametrize("N,P,Q,H,G,bc", CS_CASES)
def test_chunk_state(N, P, Q, H, G, bc):
    torch.manual_seed(N + P + Q + H)
    B = col_slice(bc * Q, G * N)
    assert B.stride(0) > G * N
    xdtd = randn(bc * H, Q, P)
    n = bc * H * N * P
    buf = torch.full((n + 512,), 7.0, device=dev(), dtype=BF)
    got = ext().ssd_chunk_state(B, xdtd, H, G, P, N, Q, buf[256:256 + n])
    assert got.shape == (bc * H, N, P) and got.data_ptr() == buf[256:].data_ptr()
    assert (buf[:256] == 7).all() and (buf[256 + n:] == 7).all()
    ref = reference.ssd_chunk_state(B.double(), xdtd.double(), H, G, P, N, Q)
    mag = reference.ssd_chunk_state(B.double().abs(), xdtd.double().abs(),
                                    H, G, P, N, Q)
    rule.check(f"ssd_chunk_state[N={N},P={P},Q={Q},H={H},G={G},bc={bc}]",
               got, ref, mag, A_RED)
    assert same_bits(got, ext().ssd_chunk_state(B, xdtd, H, G, P, N, Q))


# H, P, N, Q: one 64-thread block per (b, h); four 256-thread blocks
SMALL, WIDE = (3, 32, 16, 32), (2, 64, 128, 64)


def pass_case(dims, nc, with_init, seed, b=2):
    torch.manual_seed(seed)
    H, P, N, Q = dims
    S = randn(b * nc * H, N, P)
    dacs = make_dacs(b * nc * H, Q)      # chunk totals about -0.5 .. -30
    init = torch.randn(b, H, P, N, device=dev()) * 2 if with_init else None
    return S, dacs, init


def pass_oracle(dims, S, dacs, init, dm=None, b=2):
    """float64 (prev, final) and their widened rule magnitudes."""
    H, P, N, Q = dims
    i64 = None if init is None else init.double()
    ref = reference.ssd_state_pass(S.double(), dacs.double(), b, H, P, N, Q,
                                   dm, i64, True)
    m, m_fin = reference.ssd_state_pass(
        S.double().abs(), dacs.double(), b, H, P, N, Q, dm,
        None if init is None else i64.abs(), True)
    nc = S.shape[0] // (b * H)
    Gc = dacs.double().view(b, nc, H, Q)[..., -1]
    a, d = torch.exp(Gc), (Gc.abs() + 2) * U
    if dm is not None:
        keep = reference.doc_rel_start(dm, Q, dev()).view(b, nc, Q)[..., -1] < 0
        a = a * keep[..., None]
    m5 = m.view(b, nc, H, N, P)
    E, Es = torch.zeros_like(m5[:, 0]), []
    for c in range(nc):
        Es.append(E)
        E = a[:, c, :, None, None] * (E + d[:, c, :, None, None] * m5[:, c])
    mag = rule.widen(m, torch.stack(Es, 1).reshape(m.shape))
    return ref, (mag, rule.widen(m_fin, E.transpose(-1, -2)))


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("nc", [1, 2, 5, 33])
@pytest.mark.parametrize("dims", [SMALL, WIDE])
def test_state_pass_fwd(dims, nc, with_init):
    (H, P, N, Q), b = dims, 2
    S, dacs, init = pass_case(dims, nc, with_init, nc)
    prev, final = ext().ssd_state_pass_fwd(S, dacs, b, nc, H, P, N, Q, init,
                                           True)
    assert prev.dtype == BF and final.dtype == torch.float32
    (p_ref, f_ref), (p_mag, f_mag) = pass_oracle(dims, S, dacs, init)
    tag = f"[N={N},nc={nc},init={with_init}]"
    rule.check("ssd_state_pass.prev" + tag, prev, p_ref, p_mag, A_RED)
    rule.check("ssd_state_pass.final" + tag, final, f_ref, f_mag, A_RED)
    only = ext().ssd_state_pass_fwd(S, dacs, b, nc, H, P, N, Q, init, False)
    assert len(only) == 1 and same_bits(only[0], prev)


@pytest.mark.parametrize("dims", [SMALL, WIDE])
def test_state_pass_fwd_doc(dims):
    (H, P, N, Q), b, nc = dims, 3, 5
    S, dacs, _ = pass_case(dims, nc, False, 7, b=b)
    dm = mask_of(ssd_rows(Q), nc * Q)

    def run(S_):
        return ext().ssd_state_pass_fwd_doc(S_, dacs, b, nc, H, P, N, Q, None,
                                            True, dm.start, nc * Q)
    prev, final = run(S)
    (p_ref, f_ref), (p_mag, f_mag) = pass_oracle(dims, S, dacs, None, dm, b=b)
    assert (p_ref == 0).any() and (p_ref.view(b, nc, -1)[:, 1:] != 0).any()
    rule.check("ssd_state_pass_doc.prev", prev, p_ref, p_mag, A_RED)
    rule.check("ssd_state_pass_doc.final", final, f_ref, f_mag, A_RED)
    # chunks that end in the row's first document get large finite states:
    # prev behind a chunk that ends in a later document keeps its bits
    first = dm.start[:, Q - 1::Q] == 0                            # (b, nc)
    assert first[1, 0] and not first[1, 1:].any() and first[2].all()
    big = torch.where(first[:, :, None, None, None],
                      torch.full_like(S.view(b, nc, H, N, P), 1e30),
                      S.view(b, nc, H, N, P)).view_as(S)
    later = torch.ones_like(first)
    later[:, 1:] = ~first[:, :-1]
    prev2 = run(big)[0]
    assert same_bits(prev.view(b, nc, -1)[later], prev2.view(b, nc, -1)[later])
    assert not same_bits(prev, prev2)
    with pytest.raises(RuntimeError):     # initial state under a mask
        ext().ssd_state_pass_fwd_doc(
            S, dacs, b, nc, H, P, N, Q,
            torch.zeros(b, H, P, N, device=dev()), True, dm.start, nc * Q)


@pytest.mark.parametrize("dims,nc,with_init,masked", [
    (SMALL, 1, True, False), (SMALL, 5, True, False),
    (SMALL, 5, False, False), (SMALL, 5, False, True),
    (WIDE, 5, True, False), (WIDE, 5, False, True)])
def test_state_pass_bwd(dims, nc, with_init, masked):
    H, P, N, Q = dims
    b = 3 if masked else 2
    S, dacs, init = pass_case(dims, nc, with_init, 11 + nc, b=b)
    dm = mask_of(ssd_rows(Q), nc * Q) if masked else None
    dprev = randn(b * nc * H, N, P)
    dfinal = torch.randn(b, H, P, N, device=dev())

    def grads(S_, dacs_, init_, cot, fn):
        leaves = [t.detach().requires_grad_() for t in (S_, dacs_, init_)
                  if t is not None]
        prev, final = fn(leaves[0], leaves[1], b, H, P, N, Q, dm,
                         leaves[2] if with_init else None, True)
        return torch.autograd.grad((prev, final), leaves, cot)

    n0 = ext().ssd_state_calls()
    got = grads(S, dacs, init, (dprev, dfinal), ops.ssd_state_pass)
    assert ext().ssd_state_calls() == n0 + 2
    again = grads(S, dacs, init, (dprev, dfinal), ops.ssd_state_pass)
    assert all(same_bits(x, y) for x, y in zip(got, again))
    up = lambda t: None if t is None else t.double()
    ab = lambda t: None if t is None else t.double().abs()
    ref = grads(up(S), up(dacs), up(init), (up(dprev), up(dfinal)),
                reference.ssd_state_pass)
    # every term of every gradient is a product of factors that the abs
    # run makes non-negative: its gradients are the sums of |terms|
    mag = grads(ab(S), up(dacs), ab(init), (ab(dprev), ab(dfinal)),
                reference.ssd_state_pass)
    tag = f"[N={N},nc={nc},init={with_init},masked={masked}]"
    rule.check("ssd_state_pass_bwd.dS" + tag, got[0], ref[0], mag[0], A_RED)
    # dG_c reads the saved bf16 prev: up to 2^-8 of every |gH_c prev_c|
    rule.check("ssd_state_pass_bwd.ddacs" + tag, got[1], ref[1],
               rule.widen(mag[1], 2.0 ** -8 * mag[1]), A_RED)
    if with_init:
        rule.check("ssd_state_pass_bwd.dinitial" + tag, got[2], ref[2],
                   mag[2], A_RED)


def small_mixer(headdim=32):
    from fms_fsdp_amd.models.mamba import Mamba2Mixer, MambaConfig
    torch.manual_seed(0)
    cfg = MambaConfig(d_model=128, n_layer=1, vocab_size=512, d_state=16,
                      headdim=headdim, expand=2, ngroups=2, chunk_size=64)
    mixer = Mamba2Mixer(cfg, 0)
    mixer.reset_parameters()
    return mixer.to(dev()).bfloat16()


def split_prefill(expect_kernels, headdim=32):
    """2*64 + 5 tokens fed as 64 + 3 on a fresh cache and 64 + 2 on the
    used one, against the prompt fed whole."""
    mixer = small_mixer(headdim).eval()
    u = torch.randn(2, 133, 128, device=dev(), dtype=BF) * 0.5

    def cache():
        return ops.MambaCache(2, mixer.conv_dim, mixer.d_conv, mixer.nheads,
                              mixer.headdim, mixer.d_state, BF, dev())
    with torch.no_grad():
        whole_c, split_c = cache(), cache()
        whole = mixer(u, cache=whole_c)
        first = mixer(u[:, :67], cache=split_c)
        n0 = ext().ssd_state_calls()
        split = torch.cat([first, mixer(u[:, 67:], cache=split_c)], dim=1)
    assert (ext().ssd_state_calls() > n0) == expect_kernels
    assert split_c.len == 133
    errs = relerr(split, whole), relerr(split_c.ssm, whole_c.ssm)
    print(f"[split prefill kernels={expect_kernels}] relerr out {errs[0]:.3g}, "
          f"ssm {errs[1]:.3g}")
    assert max(errs) < FWD_TOL, errs


def test_split_prefill_takes_the_kernels(monkeypatch):
    monkeypatch.delenv("FMS_AMD_MAMBA_PREFILL", raising=False)
    monkeypatch.delenv("FMS_AMD_FORCE_TORCH_SCAN", raising=False)
    split_prefill(True)


def test_split_prefill_without_a_state_pass_kernel_keeps_the_step_route(
        monkeypatch):
    """headdim 16 with d_state 16: N*P is no multiple of 512."""
    monkeypatch.delenv("FMS_AMD_MAMBA_PREFILL", raising=False)
    assert not ops.ssd_state_pass_has_kernel(16, 16)
    assert ops.ssd_state_pass_has_kernel(16, 32)
    split_prefill(False, headdim=16)


def test_split_prefill_step_route_in_a_child_process():
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]\n"
            "import test_ssd_state_gpu as t; t.split_prefill(False)")
    env = dict(os.environ, FMS_AMD_MAMBA_PREFILL="step")
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("masked", [False, True])
def test_training_scan_fused_chain_matches_gemm(masked):
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
        prev = ops.ssd_state_chain(mode)
        try:
            leaves = [t.clone().requires_grad_() for t in (x, dt, B, C)]
            xi, dti, Bi, Ci = leaves
            n0 = ext().ssd_state_calls()
            out = mixer._scan_fused(b, l, xi, dti, z, Bi, Ci, mixer.dt_bias,
                                    mixer.A_log, mixer.D, *doc)
            gr = torch.autograd.grad(out.float().pow(2).mean(),
                                     leaves + [mixer.A_log])
            return out.detach(), gr, ext().ssd_state_calls() - n0
        finally:
            ops.ssd_state_chain(prev)
    o_g, g_g, calls_g = run("gemm")
    o_f, g_f, calls_f = run("fused")
    assert calls_g == 0 and calls_f == 3
    # the criterion of test_ops_gpu.test_ssd_fused_scan_matches_torch
    assert relerr(o_f, o_g) < 3e-2, relerr(o_f, o_g)
    for nm, a, r in zip(("x", "dt", "B", "C"), g_f, g_g):
        assert relerr(a, r) < 6e-2, (nm, relerr(a, r))
    assert relerr(g_f[4], g_g[4]) < 8e-2, relerr(g_f[4], g_g[4])
