"""Causal attention under both workgroup orders (attn_sched.h): each order
against the fp32 references, and balanced bit-identical to legacy.

Outputs are torch.empty inside the bindings, so a recycled allocator block
could still hold an earlier correct result; every call is therefore
preceded by allocating and freeing NaN-filled tensors of the output sizes
and dtypes, and the outputs are checked for NaN."""

import functools

import pytest
import torch

from fms_fsdp_amd.ops import reference

pytestmark = pytest.mark.gpu

# one tile; odd tile/head counts; nbh % 8 != 0; the pinned nbh % 8 == 0
# path; GQA at both head dims
SHAPES = [
    (1, 128, 2, 2, 128),
    (1, 384, 3, 3, 128),
    (3, 640, 4, 4, 64),
    (2, 1024, 4, 4, 128),
    (1, 1152, 16, 4, 128),
    (2, 512, 12, 4, 64),
]
MODES = ["balanced", "legacy"]
FUSED_SHAPE = (2, 1024, 4, 4, 128)


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def poison(*specs):
    """Fill blocks of the given (shape, dtype) with NaN and hand them back
    to the caching allocator."""
    junk = [torch.full(shape, float("nan"), device=dev(), dtype=dtype)
            for shape, dtype in specs]
    torch.cuda.synchronize()
    del junk


class sched_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from fms_fsdp_amd import _C
        self.prev = _C.attn_sched_mode(self.mode)
        assert _C.attn_sched_mode() == self.mode

    def __exit__(self, *exc):
        from fms_fsdp_amd import _C
        _C.attn_sched_mode(self.prev)


@functools.lru_cache(maxsize=None)
def inputs(shape):
    b, s, h, kvh, d = shape
    g = torch.Generator(device=dev()).manual_seed(1234)
    mk = lambda nh: torch.randn(b, s, nh, d, device=dev(), generator=g,
                                dtype=torch.bfloat16)
    return mk(h), mk(kvh), mk(kvh), mk(h)   # q, k, v, do


@functools.lru_cache(maxsize=None)
def references(shape):
    """Computed once per shape, shared and never modified."""
    b, s, h, kvh, d = shape
    q, k, v, do = inputs(shape)
    o_ref = reference.attention_causal(q, k, v)
    qt = q.transpose(1, 2).float()
    kt = k.transpose(1, 2).float()
    if kvh != h:
        kt = kt.repeat_interleave(h // kvh, dim=1)
    scores = qt @ kt.transpose(-1, -2) / (d ** 0.5)
    mask = torch.full((s, s), float("-inf"), device=dev()).triu(1)
    lse_ref = (scores + mask).logsumexp(-1)
    qf = q.float().requires_grad_()
    kf = k.float().requires_grad_()
    vf = v.float().requires_grad_()
    of = torch.nn.functional.scaled_dot_product_attention(
        qf.transpose(1, 2), kf.transpose(1, 2), vf.transpose(1, 2),
        is_causal=True, enable_gqa=(kvh != h)).transpose(1, 2)
    of.backward(do.float())
    return dict(o=o_ref, lse=lse_ref, dq=qf.grad, dk=kf.grad, dv=vf.grad)


@functools.lru_cache(maxsize=None)
def kernel_outputs(shape, mode):
    from fms_fsdp_amd import _C
    b, s, h, kvh, d = shape
    q, k, v, do = inputs(shape)
    bf, f32 = torch.bfloat16, torch.float32
    kv_dtype = bf if kvh == h else f32
    with sched_mode(mode):
        poison(((b, s, h, d), bf), ((b, h, s), f32))
        o, lse = _C.attn_fwd(q, k, v)
        poison(((b, s, h, d), bf), ((b, s, kvh, d), kv_dtype),
               ((b, s, kvh, d), kv_dtype), ((b, h, s), f32),
               ((b * h, s, s), bf))
        dq, dk, dv = _C.attn_bwd(do, q, k, v, o, lse, None)
        torch.cuda.synchronize()
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mode_matches_reference(shape, mode):
    got, ref = kernel_outputs(shape, mode), references(shape)
    for name in ("o", "lse", "dq", "dk", "dv"):
        assert not torch.isnan(got[name]).any(), name
    errs = {n: relerr(got[n], ref[n]) for n in got}
    print(shape, mode, errs)
    assert errs["o"] < 3e-2, errs
    assert errs["lse"] < 3e-2, errs
    assert errs["dq"] < 6e-2, errs
    assert errs["dk"] < 6e-2, errs
    assert errs["dv"] < 6e-2, errs


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_balanced_bit_identical_to_legacy(shape):
    """The same workgroup code writes each element exactly once in the
    same order, whichever workgroup id runs it. GQA dk/dv accumulate
    through fp32 atomics (order-dependent): reference check only."""
    b, s, h, kvh, d = shape
    bal, leg = kernel_outputs(shape, "balanced"), kernel_outputs(shape, "legacy")
    names = ["o", "lse", "dq"] + (["dk", "dv"] if kvh == h else [])
    for name in names:
        assert not torch.isnan(bal[name]).any(), name
        assert torch.equal(bal[name], leg[name]), name


def test_fused_qkv_rope_attention_bit_identical():
    """Strided-v forward and dv written into the fused dqkv buffer."""
    from fms_fsdp_amd import ops
    b, s, h, kvh, d = FUSED_SHAPE
    E = (h + 2 * kvh) * d
    g = torch.Generator(device=dev()).manual_seed(4321)
    qkv = torch.randn(b, s, E, device=dev(), generator=g,
                      dtype=torch.bfloat16)
    do = torch.randn(b, s, h, d, device=dev(), generator=g,
                     dtype=torch.bfloat16)
    pos = torch.arange(s, dtype=torch.float32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    ang = torch.outer(pos, inv)
    cos, sin = ang.cos().to(dev()), ang.sin().to(dev())
    bf, f32 = torch.bfloat16, torch.float32

    def run(mode):
        a = qkv.clone().requires_grad_()
        with sched_mode(mode):
            poison(((b, s, h, d), bf), ((b, s, kvh, d), bf),
                   ((b, s, h, d), bf), ((b, h, s), f32))
            o = ops.qkv_rope_attention(a, cos, sin, h, kvh, d)
            poison(((b, s, E), bf), ((b, s, h, d), bf), ((b, s, kvh, d), bf),
                   ((b, h, s), f32), ((b * h, s, s), bf))
            o.backward(do)
            torch.cuda.synchronize()
        return o.detach(), a.grad

    o_b, g_b = run("balanced")
    o_l, g_l = run("legacy")
    for t in (o_b, g_b, o_l, g_l):
        assert not torch.isnan(t).any()
    assert torch.equal(o_b, o_l)
    assert torch.equal(g_b, g_l)
