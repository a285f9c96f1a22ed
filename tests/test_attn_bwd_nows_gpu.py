"""Workspace-free causal attention backward (attn_ws.h gate at limit 0):
attn_bwd_dq_recompute_kernel + the non-publishing dkv instantiations.

Against fp32 SDPA autograd under both workgroup orders; dk/dv bit-identical
to the workspace path (same arithmetic, only the dS store removed); no
(b*h, s, s) allocation; the public autograd paths; the knob itself.

Outputs are torch.empty inside the bindings, so every call is preceded by
allocating and freeing NaN-filled tensors of the output sizes and dtypes
(never the workspace's), and the outputs are checked for NaN."""

import functools

import pytest
import torch

from fms_fsdp_amd.ops import reference

pytestmark = pytest.mark.gpu

# one tile (diagonal only); odd tile count with nbh % 8 != 0; d64 MHA;
# GQA at both head dims; several tiles with nbh % 8 == 0
SHAPES = [
    (1, 128, 2, 2, 128),
    (1, 384, 3, 3, 128),
    (3, 640, 4, 4, 64),
    (2, 512, 12, 4, 64),
    (1, 1152, 16, 4, 128),
    (2, 1024, 4, 4, 128),
]
MHA_SHAPES = [s for s in SHAPES if s[2] == s[3]]
MODES = ["balanced", "legacy"]
MEM_SHAPE = (1, 2048, 4, 4, 64)     # workspace 32 MiB, outputs ~3 MiB
FUSED_SHAPE = (2, 1024, 4, 4, 128)
MIB = 1 << 20
DEFAULT_LIMIT = 4096 * MIB
BWD_TOL = 6e-2
FWD_TOL = 3e-2


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


class ws_limit:
    """Set the workspace limit (bytes) and restore the previous one."""

    def __init__(self, nbytes):
        self.nbytes = nbytes

    def __enter__(self):
        from fms_fsdp_amd import _C
        self.prev = _C.attn_bwd_ws_limit(self.nbytes)
        assert _C.attn_bwd_ws_limit() == self.nbytes

    def __exit__(self, *exc):
        from fms_fsdp_amd import _C
        _C.attn_bwd_ws_limit(self.prev)


class sched_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from fms_fsdp_amd import _C
        self.prev = _C.attn_sched_mode(self.mode)

    def __exit__(self, *exc):
        from fms_fsdp_amd import _C
        _C.attn_sched_mode(self.prev)


@functools.lru_cache(maxsize=None)
def inputs(shape):
    b, s, h, kvh, d = shape
    g = torch.Generator(device=dev()).manual_seed(2468)
    mk = lambda nh: torch.randn(b, s, nh, d, device=dev(), generator=g,
                                dtype=torch.bfloat16)
    return mk(h), mk(kvh), mk(kvh), mk(h)   # q, k, v, do


@functools.lru_cache(maxsize=None)
def forward(shape):
    from fms_fsdp_amd import _C
    q, k, v, _ = inputs(shape)
    o, lse = _C.attn_fwd(q, k, v)
    torch.cuda.synchronize()
    return o, lse


@functools.lru_cache(maxsize=None)
def references(shape):
    """fp32 SDPA autograd; computed once per shape, never modified."""
    b, s, h, kvh, d = shape
    q, k, v, do = inputs(shape)
    qf = q.float().requires_grad_()
    kf = k.float().requires_grad_()
    vf = v.float().requires_grad_()
    of = torch.nn.functional.scaled_dot_product_attention(
        qf.transpose(1, 2), kf.transpose(1, 2), vf.transpose(1, 2),
        is_causal=True, enable_gqa=(kvh != h)).transpose(1, 2)
    of.backward(do.float())
    return dict(dq=qf.grad, dk=kf.grad, dv=vf.grad)


@functools.lru_cache(maxsize=None)
def backward(shape, mode, limit):
    from fms_fsdp_amd import _C
    b, s, h, kvh, d = shape
    q, k, v, do = inputs(shape)
    o, lse = forward(shape)
    bf, f32 = torch.bfloat16, torch.float32
    kv_dtype = bf if kvh == h else f32
    with sched_mode(mode), ws_limit(limit):
        poison(((b, s, h, d), bf), ((b, s, kvh, d), kv_dtype),
               ((b, s, kvh, d), kv_dtype), ((b, h, s), f32))
        dq, dk, dv = _C.attn_bwd(do, q, k, v, o, lse, None)
        torch.cuda.synchronize()
    return dict(dq=dq, dk=dk, dv=dv)


def check_against_reference(shape, got):
    ref = references(shape)
    for name in ("dq", "dk", "dv"):
        assert not torch.isnan(got[name]).any(), name
    errs = {n: relerr(got[n], ref[n]) for n in ("dq", "dk", "dv")}
    print(shape, errs)
    for name, err in errs.items():
        assert err < BWD_TOL, errs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_nows_matches_reference(shape, mode):
    check_against_reference(shape, backward(shape, mode, 0))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_nows_balanced_bit_identical_to_legacy(shape):
    """Each dq element is written once by the same workgroup code whichever
    workgroup id runs it; MHA dk/dv too. GQA dk/dv accumulate through fp32
    atomics (order-dependent): reference check only."""
    b, s, h, kvh, d = shape
    bal, leg = backward(shape, "balanced", 0), backward(shape, "legacy", 0)
    for name in ["dq"] + (["dk", "dv"] if kvh == h else []):
        assert not torch.isnan(bal[name]).any(), name
        assert torch.equal(bal[name], leg[name]), name


@pytest.mark.parametrize("shape", MHA_SHAPES, ids=str)
def test_dkv_unchanged_by_dropping_the_publish(shape):
    nows = backward(shape, "balanced", 0)
    ws = backward(shape, "balanced", DEFAULT_LIMIT)
    for name in ("dk", "dv"):
        assert not torch.isnan(nows[name]).any(), name
        assert torch.equal(nows[name], ws[name]), name


def test_no_workspace_is_allocated():
    from fms_fsdp_amd import _C
    b, s, h, kvh, d = MEM_SHAPE
    q, k, v, do = inputs(MEM_SHAPE)
    o, lse = forward(MEM_SHAPE)
    ws_bytes = b * h * s * s * 2
    assert ws_bytes == 32 * MIB

    def rise(limit):
        with ws_limit(limit):
            _C.attn_bwd(do, q, k, v, o, lse, None)   # warm-up
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.max_memory_allocated()
            out = _C.attn_bwd(do, q, k, v, o, lse, None)
            torch.cuda.synchronize()
            after = torch.cuda.max_memory_allocated()
        return after - before, out

    rise_nows, out = rise(0)
    rise_ws, _ = rise(DEFAULT_LIMIT)
    print("peak rise MiB: workspace-free", rise_nows / MIB, "workspace",
          rise_ws / MIB)
    assert rise_nows < ws_bytes // 4, rise_nows
    assert rise_ws >= ws_bytes, rise_ws
    check_against_reference(MEM_SHAPE, dict(zip(("dq", "dk", "dv"), out)))


def test_attention_causal_padded_at_limit_0():
    from fms_fsdp_amd import ops
    b, s, h, kvh, d = 2, 200, 2, 2, 128
    g = torch.Generator(device=dev()).manual_seed(1357)
    mk = lambda nh: torch.randn(b, s, nh, d, device=dev(), generator=g,
                                dtype=torch.bfloat16)
    q, k, v, do = mk(h), mk(kvh), mk(kvh), mk(h)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    reference.attention_causal(qf, kf, vf).backward(do.float())
    o_ref = reference.attention_causal(q, k, v)

    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    with ws_limit(0):
        o = ops.attention_causal(qg, kg, vg)
        o.backward(do)
        torch.cuda.synchronize()
    errs = dict(o=relerr(o, o_ref), dq=relerr(qg.grad, qf.grad),
                dk=relerr(kg.grad, kf.grad), dv=relerr(vg.grad, vf.grad))
    print(errs)
    for t in (o, qg.grad, kg.grad, vg.grad):
        assert not torch.isnan(t).any()
    assert errs["o"] < FWD_TOL, errs
    assert max(errs["dq"], errs["dk"], errs["dv"]) < BWD_TOL, errs


def test_qkv_rope_attention_at_limit_0():
    """Strided v and dv written into the fused dqkv buffer. dk/dv slices
    bit-identical between the two paths; dq slice against the modular
    fp32 split -> rope -> SDPA composition."""
    from fms_fsdp_amd import ops
    b, s, h, kvh, d = FUSED_SHAPE
    hq, hk = h * d, kvh * d
    E = hq + 2 * hk
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

    def run(limit):
        a = qkv.clone().requires_grad_()
        with ws_limit(limit):
            o = ops.qkv_rope_attention(a, cos, sin, h, kvh, d)
            poison(((b, s, E), bf), ((b, s, h, d), bf), ((b, s, kvh, d), bf),
                   ((b, h, s), f32))
            o.backward(do)
            torch.cuda.synchronize()
        return a.grad

    g_nows, g_ws = run(0), run(DEFAULT_LIMIT)
    assert not torch.isnan(g_nows).any() and not torch.isnan(g_ws).any()
    assert torch.equal(g_nows[..., hq:], g_ws[..., hq:])

    af = qkv.float().requires_grad_()
    qf, kf, vf = af.split([hq, hk, hk], dim=-1)
    qr, kr = reference.rope_apply(qf.view(b, s, h, d), kf.view(b, s, kvh, d),
                                  cos, sin)
    reference.attention_causal(qr, kr, vf.view(b, s, kvh, d)).backward(
        do.float())
    err = relerr(g_nows[..., :hq], af.grad[..., :hq])
    print("fused dq relerr", err)
    assert err < BWD_TOL, err


def test_knob_round_trips():
    from fms_fsdp_amd import _C, ops
    entry = _C.attn_bwd_ws_limit()
    try:
        assert _C.attn_bwd_ws_limit(123 * MIB) == entry
        assert _C.attn_bwd_ws_limit() == 123 * MIB
        assert _C.attn_bwd_ws_limit(None) == 123 * MIB
        assert ops.attn_bwd_workspace_limit() == 123
        assert ops.attn_bwd_workspace_limit(77) == 123
        assert _C.attn_bwd_ws_limit() == 77 * MIB
        assert ops.attn_bwd_workspace_limit(0) == 77
        assert _C.attn_bwd_ws_limit(entry) == 0
    finally:
        _C.attn_bwd_ws_limit(entry)
    assert _C.attn_bwd_ws_limit() == entry
