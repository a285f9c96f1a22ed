"""_C.ssd_step (ops/hip/ssd_step.hip) against its float64 oracle,
reference.ssd_state_update, under the one rule of tests/oracle_rule.py,
plus the bitwise properties of the kernel (split calls, strided inputs,
batch rows, memory outside the state) and the binding's rejections.

All inputs are the bf16/fp32 tensors the kernel takes, upcast to float64
for the oracle. x/B/C/z/dt are column slices of wider buffers, as the
model hands them over."""

import math

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference

pytestmark = pytest.mark.gpu

DD = torch.float64
BF = torch.bfloat16
A_RED = rule.A_REDUCE
U = 2.0 ** -23          # one fp32 ulp, relative

# Compounded error of the per-step decay a_t = __expf(dtf_t * A_h), as a
# relative error (C1 * |dtf_t A_h| + C2A) * U of a_t. C1 counts the
# relative errors of the exponent's argument, in units of U:
#   8  dtf: the allowance of its own chain (A_CHAIN = 2^-20 = 8 U, the
#      plain rule of the ssd_prep_fwd.dtf row; its |x|-proportional
#      softplus term comes on top, see e_sp below)
#   3  A_h = -__expf(A_log): the argument A_log * log2(e) rounds by
#      |A_log| / 2 <= 1.4 U (A in [-16, -1]), v_exp_f32 adds 1 U
#   1  the product dtf * A and its scaling by log2(e) in __expf round by
#      U / 2 each
# C2A: 1 U for v_exp_f32's result and 1 U for the roundings of the fma
# a * s + in and of the product in = (dtf x) * B.
C1, C2A = 12.0, 2.0
# Relative error of the input term (dtf x) B through dtf: its chain
# allowance again (the softplus term comes on top).
C2IN = 8.0


def dev():
    return torch.device("cuda:0")


def ext():
    from fms_fsdp_amd import _C
    return _C


def col_slice3(b, T, cols, lead=8, trail=24, scale=1.0, shift=0.0):
    """(b, T, cols) bf16 column slice of a wider buffer: unit last stride,
    one uniform row stride > cols, 16-byte aligned."""
    wide = (torch.randn(b, T, lead + cols + trail, device=dev()) * scale
            + shift).to(BF)
    return wide[..., lead:lead + cols]


def make_inputs(b, T, H, G, P, N, seed):
    torch.manual_seed(seed)
    inp = dict(
        x=col_slice3(b, T, H * P), z=col_slice3(b, T, H * P, scale=2.0),
        B=col_slice3(b, T, G * N), C=col_slice3(b, T, G * N),
        # raw dt spans about -8 .. 4
        dt=(torch.rand(b, T, 5 + H + 4, device=dev()) * 12 - 8)
        .to(BF)[..., 5:5 + H],
        dt_bias=(torch.rand(H, device=dev()) - 0.5),
        # A = -exp(A_log) covers [-16, -1], both ends included
        A_log=torch.linspace(0.0, math.log(16.0), H, device=dev()),
        D=torch.randn(H, device=dev()))
    assert inp["x"].stride(1) > H * P and inp["dt"].stride(1) > H
    state = torch.randn(b, H, P, N, device=dev())
    return inp, state


def call(state, inp, H, G, P, N, lo=None, hi=None, fn=None):
    sl = slice(lo, hi)
    fn = fn or ext().ssd_step
    return fn(state, inp["x"][:, sl], inp["dt"][:, sl], inp["B"][:, sl],
              inp["C"][:, sl], inp["z"][:, sl], inp["dt_bias"], inp["A_log"],
              inp["D"], H, G, P, N)


def oracle(state0, inp, H, G, P, N):
    """float64 state and out, their rule magnitudes and the derived
    absolute bounds of the compounded decay error (widening terms)."""
    i64 = {k: v.double() for k, v in inp.items()}
    s_ref = state0.double().clone()
    out_ref = call(s_ref, i64, H, G, P, N, fn=reference.ssd_state_update)
    b, T, _ = inp["x"].shape
    rep = H // G
    xs = i64["dt"] + i64["dt_bias"]
    dtf = torch.logaddexp(xs, torch.zeros_like(xs))            # (b, T, H)
    A = -torch.exp(i64["A_log"])
    a = torch.exp(dtf * A)
    # softplus below the guard (the ssd_prep_fwd.dtf row): x = dt + bias
    # and __expf's argument round by |x| U / 2 each, passed on times
    # sigmoid(x): an absolute error of dtf
    e_sp = torch.where(xs > 20, torch.zeros_like(xs),
                       xs.abs() * U * torch.sigmoid(xs))
    d_a = (C1 * (dtf * A).abs() + C2A) * U + A.abs() * e_sp
    d_in = C2IN * U + e_sp / dtf
    xh = i64["x"].reshape(b, T, H, P).abs()
    Bh = i64["B"].reshape(b, T, G, N).repeat_interleave(rep, 2).abs()
    Ch = i64["C"].reshape(b, T, G, N).repeat_interleave(rep, 2).abs()
    # m_t = a_t m_{t-1} + |dtf x B|, m_0 = |state0|; E_t, the error the
    # decays and dtf carry into the state, follows the same recurrence:
    #   E_t = a_t (E_{t-1} + d_a_t m_{t-1}) + d_in_t |dtf x B|
    # (never above sum_{tau<=t} max(d_a, d_in)_tau * m_t)
    m = state0.double().abs()
    E = torch.zeros_like(m)
    mag_y, err_y = [], []
    for t in range(T):
        inn = (dtf[:, t, :, None] * xh[:, t])[..., None] \
            * Bh[:, t, :, None, :]
        at = a[:, t, :, None, None]
        E = at * (E + d_a[:, t, :, None, None] * m) \
            + d_in[:, t, :, None, None] * inn
        m = at * m + inn
        mag_y.append((m * Ch[:, t, :, None, :]).sum(-1)
                     + i64["D"].abs().view(1, H, 1) * xh[:, t])
        err_y.append((E * Ch[:, t, :, None, :]).sum(-1))
    zh = i64["z"].reshape(b, T, H, P)
    gate = (zh * torch.sigmoid(zh)).abs()
    mag_out = (torch.stack(mag_y, 1) * gate).reshape(b, T, H * P)
    err_out = (torch.stack(err_y, 1) * gate).reshape(b, T, H * P)
    return s_ref, out_ref, m, E, mag_out, err_out


@pytest.mark.parametrize("T", [1, 3, 63])
@pytest.mark.parametrize("N", [16, 128])
@pytest.mark.parametrize("P", [8, 16, 64])
@pytest.mark.parametrize("H,G", [(3, 1), (4, 2), (6, 2)])
def test_ssd_step(H, G, P, N, T):
    b = 2
    inp, state = make_inputs(b, T, H, G, P, N, seed=H * 1000 + P * 10 + T + N)
    state0 = state.clone()
    out = call(state, inp, H, G, P, N)
    assert out.shape == (b, T, H * P) and out.dtype == BF
    assert out.is_contiguous()
    s_ref, out_ref, m, E, mag_out, err_out = oracle(state0, inp, H, G, P, N)
    tag = f"[H={H},G={G},P={P},N={N},T={T}]"
    rule.check("ssd_step.state" + tag, state, s_ref,
               rule.widen(m, E, A_RED), A_RED)
    rule.check("ssd_step.out" + tag, out, out_ref,
               rule.widen(mag_out, err_out, A_RED), A_RED)


def test_split_calls_are_bit_identical():
    H, G, P, N = 4, 2, 16, 128
    inp, state = make_inputs(2, 5, H, G, P, N, seed=1)
    s_one, s_two = state.clone(), state.clone()
    one = call(s_one, inp, H, G, P, N)
    # pieces of a (b, T) buffer have no uniform row stride at b = 2
    p1 = {k: (v[:, :2].contiguous() if v.dim() == 3 else v)
          for k, v in inp.items()}
    p2 = {k: (v[:, 2:].contiguous() if v.dim() == 3 else v)
          for k, v in inp.items()}
    two = torch.cat([call(s_two, p1, H, G, P, N),
                     call(s_two, p2, H, G, P, N)], dim=1)
    assert torch.equal(one, two)
    assert torch.equal(s_one, s_two)
    # and a second call gives the same bits as the first
    s_again = state.clone()
    assert torch.equal(call(s_again, inp, H, G, P, N), one)
    assert torch.equal(s_again, s_one)


@pytest.mark.parametrize("T", [1, 4])
def test_strided_inputs_equal_their_contiguous_copies(T):
    H, G, P, N = 6, 2, 8, 16
    inp, state = make_inputs(2, T, H, G, P, N, seed=2 + T)
    cont = {k: v.contiguous() for k, v in inp.items()}
    assert not inp["x"].is_contiguous()
    s_a, s_b = state.clone(), state.clone()
    assert torch.equal(call(s_a, inp, H, G, P, N),
                       call(s_b, cont, H, G, P, N))
    assert torch.equal(s_a, s_b)
    # the wrapper: same bits, and it copies what the kernel cannot read
    s_c = state.clone()
    assert torch.equal(call(s_c, inp, H, G, P, N, fn=ops.ssd_state_update),
                       call(state.clone(), cont, H, G, P, N))
    assert torch.equal(s_c, s_a)
    odd = dict(inp)
    wide = torch.randn(2, T, H * P + 3, device=dev()).to(BF)
    wide[..., 3:] = inp["x"]
    odd["x"] = wide[..., 3:]                  # 6-byte offset, stride % 8 != 0
    s_d = state.clone()
    assert torch.equal(call(s_d, odd, H, G, P, N, fn=ops.ssd_state_update),
                       call(state.clone(), cont, H, G, P, N))
    assert torch.equal(s_d, s_a)


def test_batch_rows_are_independent():
    H, G, P, N = 3, 1, 64, 128
    inp, state = make_inputs(2, 3, H, G, P, N, seed=4)
    s_a = state.clone()
    out_a = call(s_a, inp, H, G, P, N)
    other = {k: (v.contiguous().clone() if v.dim() == 3 else v)
             for k, v in inp.items()}
    for k, v in other.items():
        if v.dim() == 3:
            v[0] = torch.randn_like(v[0].float()).to(BF)
    s_b = state.clone()
    s_b[0] = torch.randn_like(s_b[0])
    out_b = call(s_b, other, H, G, P, N)
    assert torch.equal(out_a[1], out_b[1])
    assert torch.equal(s_a[1], s_b[1])
    assert not torch.equal(out_a[0], out_b[0])


@pytest.mark.parametrize("P,N", [(8, 16), (24, 128)])
def test_memory_around_the_state_is_untouched(P, N):
    # P = 8 and P = 24: the last block of 16 rows is half masked
    H, G, b, T = 3, 1, 2, 2
    inp, _ = make_inputs(b, T, H, G, P, N, seed=5)
    guard, n = 4096, b * H * P * N
    buf = torch.full((guard + n + guard,), -77.0, device=dev())
    state = buf[guard:guard + n].view(b, H, P, N)
    state.normal_()
    before = state.clone()
    call(state, inp, H, G, P, N)
    assert (buf[:guard] == -77.0).all() and (buf[guard + n:] == -77.0).all()
    assert not torch.equal(state, before)
    assert torch.isfinite(state).all()


def test_binding_rejects_what_the_kernel_cannot_run():
    H, G, P, N, b, T = 4, 2, 16, 16, 2, 2
    inp, state = make_inputs(b, T, H, G, P, N, seed=6)
    keep = state.clone()

    def bad(state_=None, H_=H, G_=G, P_=P, N_=N, **over):
        i = dict(inp, **over)
        with pytest.raises(RuntimeError):
            call(state if state_ is None else state_, i, H_, G_, P_, N_)

    bad(x=inp["x"].half())                                   # dtype
    bad(state_=state.to(BF))
    bad(dt_bias=inp["dt_bias"].double())
    bad(state_=torch.randn(b, H, P, 24, device=dev()), N_=24,  # N = 24
        B=col_slice3(b, T, G * 24), C=col_slice3(b, T, G * 24))
    bad(state_=torch.randn(b, H, 12, N, device=dev()), P_=12,  # P = 12
        x=col_slice3(b, T, H * 12), z=col_slice3(b, T, H * 12))
    bad(G_=3, B=col_slice3(b, T, 3 * N), C=col_slice3(b, T, 3 * N))
    bad(state_=torch.randn(b, H, N, P, device=dev()).transpose(2, 3))
    empty = {k: v[:, :0] for k, v in inp.items() if v.dim() == 3}
    bad(**empty)                                             # T = 0
    wide = torch.randn(b, T, H * P + 8, device=dev()).to(BF)
    bad(x=wide[..., 4:4 + H * P])                            # 8-byte offset
    wide = torch.randn(b, T, H * P + 4, device=dev()).to(BF)
    bad(z=wide[..., :H * P])                                 # stride % 8 != 0
    bad(B=inp["B"][:1])                                      # batch mismatch
    bad(x=inp["x"].cpu())
    torch.cuda.synchronize()
    assert torch.equal(state, keep)
    with pytest.raises(RuntimeError):                        # under grad
        call(state, dict(inp, dt_bias=inp["dt_bias"].requires_grad_()),
             H, G, P, N, fn=ops.ssd_state_update)
