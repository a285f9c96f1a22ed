"""Key-on-the-lane dk/dv kernel (attn_bwd_dkv_keylane_kernel, the default
body) against the legacy body it replaces (_C.attn_dkv_mode).

Every shape under both dkv bodies, both workgroup orders and both
workspace paths against fp32 SDPA autograd; within the new body dk/dv
bit-identical across publishing / non-publishing instantiations, orders
and calls; dq on the workspace path bit-identical between the two bodies
(same dS bits, tiled against row-major workspace); a one-hot dO row check of
the q-row-to-register map and the mask; the fused qkv path (strided dv);
the mode binding.

Outputs are torch.empty inside the bindings, so every call is preceded by
allocating and freeing NaN-filled tensors of the output sizes and dtypes
and the outputs are checked for NaN."""

import functools

import pytest
import torch

from fms_fsdp_amd.ops import reference

pytestmark = pytest.mark.gpu

# one tile (diagonal only); first off-diagonal step at d64; odd tile
# count; d64 MHA with several tiles; GQA atomics epilogue at both head dims
SHAPES = [
    (1, 128, 2, 2, 128),
    (1, 256, 1, 1, 64),
    (1, 384, 3, 3, 128),
    (3, 640, 4, 4, 64),
    (2, 512, 12, 4, 64),
    (1, 1152, 16, 4, 128),
]
MHA_SHAPES = [s for s in SHAPES if s[2] == s[3]]
DKV_MODES = ["keylane", "legacy"]
SCHEDS = ["balanced", "legacy"]
MIB = 1 << 20
DEFAULT_LIMIT = 4096 * MIB
LIMITS = [0, DEFAULT_LIMIT]
ROW_SHAPE = (1, 256, 1, 1, 128)
ROW_QS = [0, 5, 37, 127, 137]
FUSED_SHAPES = [(2, 1024, 4, 4, 128), (2, 512, 8, 2, 128)]
BWD_TOL = 6e-2


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


class knobs:
    """Set dkv body, workgroup order and workspace limit; restore all."""

    def __init__(self, dkv, sched, limit):
        self.want = (dkv, sched, limit)

    def __enter__(self):
        from fms_fsdp_amd import _C
        dkv, sched, limit = self.want
        self.prev = (_C.attn_dkv_mode(dkv), _C.attn_sched_mode(sched),
                     _C.attn_bwd_ws_limit(limit))
        assert _C.attn_dkv_mode() == dkv

    def __exit__(self, *exc):
        from fms_fsdp_amd import _C
        _C.attn_dkv_mode(self.prev[0])
        _C.attn_sched_mode(self.prev[1])
        _C.attn_bwd_ws_limit(self.prev[2])


@functools.lru_cache(maxsize=None)
def inputs(shape):
    b, s, h, kvh, d = shape
    g = torch.Generator(device=dev()).manual_seed(97531)
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


def sdpa_grads(shape, q, k, v, do):
    b, s, h, kvh, d = shape
    qf = q.float().requires_grad_()
    kf = k.float().requires_grad_()
    vf = v.float().requires_grad_()
    of = torch.nn.functional.scaled_dot_product_attention(
        qf.transpose(1, 2), kf.transpose(1, 2), vf.transpose(1, 2),
        is_causal=True, enable_gqa=(kvh != h)).transpose(1, 2)
    of.backward(do.float())
    return dict(dq=qf.grad, dk=kf.grad, dv=vf.grad)


@functools.lru_cache(maxsize=None)
def references(shape):
    """fp32 SDPA autograd; computed once per shape, never modified."""
    return sdpa_grads(shape, *inputs(shape))


def run_bwd(shape, do, dkv, sched, limit):
    from fms_fsdp_amd import _C
    b, s, h, kvh, d = shape
    q, k, v, _ = inputs(shape)
    o, lse = forward(shape)
    bf, f32 = torch.bfloat16, torch.float32
    kv_dtype = bf if kvh == h else f32
    with knobs(dkv, sched, limit):
        poison(((b, s, h, d), bf), ((b, s, kvh, d), kv_dtype),
               ((b, s, kvh, d), kv_dtype), ((b, h, s), f32))
        dq, dk, dv = _C.attn_bwd(do, q, k, v, o, lse, None)
        torch.cuda.synchronize()
    return dict(dq=dq, dk=dk, dv=dv)


@functools.lru_cache(maxsize=None)
def backward(shape, dkv, sched, limit):
    return run_bwd(shape, inputs(shape)[3], dkv, sched, limit)


def assert_no_nan(got):
    for name in ("dq", "dk", "dv"):
        assert not torch.isnan(got[name]).any(), name


@pytest.mark.parametrize("limit", LIMITS, ids=["nows", "ws"])
@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("dkv", DKV_MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_matches_reference(shape, dkv, sched, limit):
    got = backward(shape, dkv, sched, limit)
    ref = references(shape)
    assert_no_nan(got)
    errs = {n: relerr(got[n], ref[n]) for n in ("dq", "dk", "dv")}
    print(shape, dkv, sched, limit, errs)
    for name, err in errs.items():
        assert err < BWD_TOL, errs


@pytest.mark.parametrize("shape", MHA_SHAPES, ids=str)
def test_keylane_dkv_same_with_and_without_publish(shape):
    ws = backward(shape, "keylane", "balanced", DEFAULT_LIMIT)
    nows = backward(shape, "keylane", "balanced", 0)
    for name in ("dk", "dv"):
        assert not torch.isnan(ws[name]).any(), name
        assert torch.equal(ws[name], nows[name]), name


@pytest.mark.parametrize("limit", LIMITS, ids=["nows", "ws"])
@pytest.mark.parametrize("shape", MHA_SHAPES, ids=str)
def test_keylane_dkv_same_under_both_orders(shape, limit):
    bal = backward(shape, "keylane", "balanced", limit)
    leg = backward(shape, "keylane", "legacy", limit)
    for name in ("dk", "dv"):
        assert not torch.isnan(bal[name]).any(), name
        assert torch.equal(bal[name], leg[name]), name


@pytest.mark.parametrize("limit", LIMITS, ids=["nows", "ws"])
@pytest.mark.parametrize("shape", MHA_SHAPES, ids=str)
def test_keylane_dkv_same_on_second_call(shape, limit):
    first = backward(shape, "keylane", "balanced", limit)
    again = run_bwd(shape, inputs(shape)[3], "keylane", "balanced", limit)
    for name in ("dk", "dv"):
        assert not torch.isnan(again[name]).any(), name
        assert torch.equal(first[name], again[name]), name


@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_workspace_dq_same_as_with_legacy_dkv(shape, sched):
    """Both bodies publish the same dS bits (the key-lane body into 2 KB
    tiles, the legacy body row-major) and the dq kernel stages either
    layout into the same LDS image, so dq does not change by a bit."""
    new = backward(shape, "keylane", sched, DEFAULT_LIMIT)
    old = backward(shape, "legacy", sched, DEFAULT_LIMIT)
    assert not torch.isnan(new["dq"]).any()
    assert torch.equal(new["dq"], old["dq"])


@pytest.mark.parametrize("dkv", DKV_MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_workspace_dq_same_under_both_orders(shape, dkv):
    bal = backward(shape, dkv, "balanced", DEFAULT_LIMIT)
    leg = backward(shape, dkv, "legacy", DEFAULT_LIMIT)
    assert not torch.isnan(bal["dq"]).any()
    assert torch.equal(bal["dq"], leg["dq"])


@pytest.mark.parametrize("limit", LIMITS, ids=["nows", "ws"])
@pytest.mark.parametrize("qstar", ROW_QS)
def test_one_hot_do_row(qstar, limit):
    """dO is zero except q row q*: dv[key] = P[q*][key] dO[q*], so rows
    with key > q* are exactly zero. A wrong q-row-to-register map or mask
    would put weight there, or miss the rows below."""
    b, s, h, kvh, d = ROW_SHAPE
    q, k, v, do_full = inputs(ROW_SHAPE)
    do = torch.zeros_like(do_full)
    do[:, qstar] = do_full[:, qstar]
    got = run_bwd(ROW_SHAPE, do, "keylane", "balanced", limit)
    ref = sdpa_grads(ROW_SHAPE, q, k, v, do)
    assert_no_nan(got)
    dv = got["dv"]
    assert (dv[:, qstar + 1:] == 0).all()
    err = relerr(dv[:, :qstar + 1], ref["dv"][:, :qstar + 1])
    print("q*", qstar, "dv relerr", err)
    assert err < BWD_TOL, err


@pytest.mark.parametrize("limit", LIMITS, ids=["nows", "ws"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=str)
def test_qkv_rope_attention_grad(shape, limit):
    """dv (and for MHA dk) land in strided slices of the fused dqkv
    buffer; against the modular fp32 split -> rope -> SDPA composition."""
    from fms_fsdp_amd import ops
    b, s, h, kvh, d = shape
    hq, hk = h * d, kvh * d
    E = hq + 2 * hk
    g = torch.Generator(device=dev()).manual_seed(8642)
    qkv = torch.randn(b, s, E, device=dev(), generator=g,
                      dtype=torch.bfloat16)
    do = torch.randn(b, s, h, d, device=dev(), generator=g,
                     dtype=torch.bfloat16)
    pos = torch.arange(s, dtype=torch.float32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    ang = torch.outer(pos, inv)
    cos, sin = ang.cos().to(dev()), ang.sin().to(dev())
    bf, f32 = torch.bfloat16, torch.float32

    a = qkv.clone().requires_grad_()
    with knobs("keylane", "balanced", limit):
        o = ops.qkv_rope_attention(a, cos, sin, h, kvh, d)
        poison(((b, s, E), bf), ((b, s, h, d), bf), ((b, s, kvh, d), bf),
               ((b, s, kvh, d), f32), ((b, h, s), f32))
        o.backward(do)
        torch.cuda.synchronize()
    assert not torch.isnan(a.grad).any()

    af = qkv.float().requires_grad_()
    qf, kf, vf = af.split([hq, hk, hk], dim=-1)
    qr, kr = reference.rope_apply(qf.view(b, s, h, d), kf.view(b, s, kvh, d),
                                  cos, sin)
    reference.attention_causal(qr, kr, vf.view(b, s, kvh, d)).backward(
        do.float())
    parts = dict(dq=relerr(a.grad[..., :hq], af.grad[..., :hq]),
                 dk=relerr(a.grad[..., hq:hq + hk], af.grad[..., hq:hq + hk]),
                 dv=relerr(a.grad[..., hq + hk:], af.grad[..., hq + hk:]))
    err = relerr(a.grad, af.grad)
    print("fused dqkv relerr", err, parts)
    assert err < BWD_TOL, (err, parts)


def test_mode_round_trips():
    from fms_fsdp_amd import _C
    entry = _C.attn_dkv_mode()
    assert entry in ("keylane", "legacy")
    try:
        assert _C.attn_dkv_mode("legacy") == entry
        assert _C.attn_dkv_mode() == "legacy"
        assert _C.attn_dkv_mode(None) == "legacy"
        assert _C.attn_dkv_mode("keylane") == "legacy"
        assert _C.attn_dkv_mode() == "keylane"
        with pytest.raises(RuntimeError):
            _C.attn_dkv_mode("fastest")
        assert _C.attn_dkv_mode() == "keylane"
        assert _C.attn_dkv_mode(entry) == "keylane"
    finally:
        _C.attn_dkv_mode(entry)
    assert _C.attn_dkv_mode() == entry
