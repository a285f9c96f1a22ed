"""_C.cconv_update (causal_conv1d.hip cconv_update_kernel): a sequence
stepped in pieces from a zero conv state equals _C.cconv_fwd on the whole
sequence bit for bit, and the state ends as the last W-1 raw input rows."""

import pytest
import torch

from fms_fsdp_amd import ops

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B_, L = 2, 23
PIECES = (1, 1, 2, 3, 5, 11)


def dev():
    return torch.device("cuda:0")


def ext():
    from fms_fsdp_amd import _C
    return _C


def strided(t, lead=8, trail=16):
    """The same values as a column slice of a wider buffer of its own:
    unit last stride, uniform row stride > C, 16-byte aligned."""
    b, T, C = t.shape
    wide = torch.full((b, T, lead + C + trail), float("nan"), dtype=BF,
                      device=dev())
    wide[..., lead:lead + C] = t
    v = wide[..., lead:lead + C]
    assert v.stride(1) > C and not v.is_contiguous()
    return v


def make(W, C, seed):
    torch.manual_seed(seed)
    x = torch.randn(B_, L, C, device=dev()).to(BF)
    w = (torch.randn(C, W, device=dev()) * 0.5).to(BF)
    bias = torch.randn(C, device=dev())
    return x, w, bias


@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("W", [2, 3, 4])
def test_pieces_equal_the_whole_sequence(W, C):
    x, w, bias = make(W, C, seed=W * 1000 + C)
    ref = ext().cconv_fwd(x, w, bias)
    state = torch.zeros(B_, W - 1, C, dtype=BF, device=dev())
    ys, lo = [], 0
    assert sum(PIECES) == L
    for n in PIECES:
        ys.append(ext().cconv_update(state, strided(x[:, lo:lo + n]), w,
                                     bias))
        lo += n
        seen = torch.cat([torch.zeros_like(state), x[:, :lo]], dim=1)
        assert torch.equal(state, seen[:, seen.shape[1] - (W - 1):]), lo
    got = torch.cat(ys, dim=1)
    assert got.is_contiguous() and torch.equal(got, ref)
    assert torch.equal(state, x[:, L - (W - 1):])

    # the op: the same bits, whatever the view (a piece of a (b, L) buffer
    # has no uniform row stride at b = 2 and is copied), fp32 parameters
    state2 = torch.zeros_like(state)
    y2 = torch.cat([ops.causal_conv1d_update(state2, piece, w.float(), bias)
                    for piece in x.split(list(PIECES), dim=1)], dim=1)
    assert torch.equal(y2, ref) and torch.equal(state2, state)


def test_short_pieces_keep_the_older_rows_in_order():
    W, C = 4, 264
    x, w, bias = make(W, C, seed=7)
    state = torch.zeros(B_, W - 1, C, dtype=BF, device=dev())
    ext().cconv_update(state, strided(x[:, 0:1]), w, bias)
    assert not state[:, :2].any() and torch.equal(state[:, 2], x[:, 0])
    ext().cconv_update(state, strided(x[:, 1:2]), w, bias)
    assert not state[:, 0].any()
    assert torch.equal(state[:, 1:], x[:, 0:2])
    ext().cconv_update(state, strided(x[:, 2:4]), w, bias)
    assert torch.equal(state, x[:, 1:4])


def test_binding_rejects_what_the_kernel_cannot_run():
    W, C = 4, 16
    x, w, bias = make(W, C, seed=8)
    state = torch.zeros(B_, W - 1, C, dtype=BF, device=dev())
    xs = x[:, :2].contiguous()
    for args in [
        (state.float(), xs, w, bias),                       # dtype
        (state, xs.half(), w, bias),
        (state, xs, w, bias.to(BF)),
        (state[:, :2], xs, w, bias),                        # W-1 rows
        (state.transpose(0, 1).contiguous().transpose(0, 1), xs, w, bias),
        (state, xs[:, :0], w, bias),                        # T = 0
        (state, xs[..., :8], w, bias),                      # channels
        (state, torch.randn(B_, 2, C + 4, device=dev()).to(BF)[..., 4:],
         w, bias),                                          # misaligned
        (state, xs, torch.randn(C, 5, device=dev()).to(BF), bias),
    ]:
        with pytest.raises(RuntimeError):
            ext().cconv_update(*args)
    torch.cuda.synchronize()
    assert not state.any()
