"""The attention backward's preprocess kernel on its own: delta (b, h, s) =
rowsum(dO * O), read with 16-byte loads by D/8 lanes per row, against
float64 by the rule of tests/oracle_rule.py."""

import pytest
import torch

import oracle_rule as rule

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def dev():
    return torch.device("cuda:0")


def ext():
    from fms_fsdp_amd import _C
    return _C


# (b, s, h, d): one tile; several heads and batches at d=64; row counts
# (b*s*h) that fill neither the last wave (4 rows at d=128, 8 at d=64)
# nor the last block
@pytest.mark.parametrize("b,s,h,d", [(1, 128, 1, 128), (2, 384, 3, 64),
                                     (1, 3, 1, 128), (1, 67, 3, 64),
                                     (3, 43, 5, 128)])
def test_attn_bwd_delta(b, s, h, d):
    torch.manual_seed(b * 1000 + s)
    do = torch.randn(b, s, h, d, device=dev()).to(BF)
    o = torch.randn(b, s, h, d, device=dev()).to(BF)
    delta = ext().attn_bwd_delta(do, o)
    assert delta.dtype == torch.float32 and delta.shape == (b, h, s)
    prod = do.double() * o.double()
    ref = prod.sum(-1).permute(0, 2, 1)
    mag = prod.abs().sum(-1).permute(0, 2, 1)
    rule.check(f"attn_bwd_delta[{b},{s},{h},{d}]", delta, ref, mag,
               rule.A_REDUCE, R=0.0)


def test_attn_bwd_delta_repeats_and_rejects():
    """Two calls agree bit for bit (no atomics), and the binding rejects
    what the kernel cannot read."""
    C = ext()
    do = torch.randn(1, 128, 2, 64, device=dev()).to(BF)
    o = torch.randn(1, 128, 2, 64, device=dev()).to(BF)
    a, b_ = C.attn_bwd_delta(do, o), C.attn_bwd_delta(do, o)
    assert torch.equal(a.view(torch.int32), b_.view(torch.int32))
    R = pytest.raises(RuntimeError)
    with R:
        C.attn_bwd_delta(do, o.float())
    with R:
        C.attn_bwd_delta(do, o[:, :64])
    with R:
        C.attn_bwd_delta(do.transpose(1, 2), o.transpose(1, 2))
    with R:
        C.attn_bwd_delta(do[..., :32].contiguous(), o[..., :32].contiguous())
    torch.cuda.synchronize()
