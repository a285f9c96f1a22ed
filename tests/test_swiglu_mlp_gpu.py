"""The fused MLP backward: `_C.swiglu_bwd_t` (dgu, dgu^T and h^T in one
pass), `_C.wgrad_tn_pre` and `ops.swiglu_mlp`.

The kernel is held bit for bit to what it replaces (`swiglu_bwd`,
`swiglu_fwd`, `transpose_bf16`), and dgu and hT elementwise to float64 by
the rule tests/test_ops_edges_gpu.py applies to swiglu. The function is
held bit for bit to the composition it replaces (FMS_AMD_MLP_BWD=split):
both issue the same GEMM calls on operands with the same bits.

Kernel shapes (rows, H): less than one 64x64 tile, exactly one, partial
tiles both ways, several tiles with a ragged edge, the 7B ratio scaled
down. Function: emb 64, hidden 176, 128 tokens, the routing thresholds
patched to 0."""

import pytest
import torch

import oracle_rule as rule
from test_ops_edges_gpu import A_CH, randn

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [(8, 8), (64, 64), (72, 88), (136, 200), (256, 1376)]


def ext():
    from fms_fsdp_amd import _C
    return _C


def bits(t):
    return t.contiguous().view(torch.int16)


_CASES = {}


def case(rows, H):
    """Inputs of one shape with saturating gates (+-30) and zeros strewn
    in, and what the separate kernels give: computed once, shared, never
    modified."""
    if (rows, H) not in _CASES:
        torch.manual_seed(100 + rows)
        gu = randn(rows, 2 * H, scale=2.0)
        dh = randn(rows, H)
        pick = torch.rand(rows, 2 * H, device=gu.device)
        gu[pick < 0.05] = 30.0
        gu[(pick >= 0.05) & (pick < 0.10)] = -30.0
        gu[(pick >= 0.10) & (pick < 0.15)] = 0.0
        dh[torch.rand(rows, H, device=gu.device) < 0.05] = 0.0
        dgu = ext().swiglu_bwd(dh, gu)
        h = ext().swiglu_fwd(gu)
        _CASES[(rows, H)] = dict(gu=gu, dh=dh, dgu=dgu, h=h,
                                 dguT=ext().transpose_bf16(dgu),
                                 hT=ext().transpose_bf16(h))
    return _CASES[(rows, H)]


@pytest.mark.parametrize("rows,H", SHAPES)
def test_swiglu_bwd_t_bit_exact(rows, H):
    c = case(rows, H)
    dgu, dguT, hT = ext().swiglu_bwd_t(c["dh"], c["gu"])
    assert dgu.shape == (rows, 2 * H) and dgu.is_contiguous()
    assert dguT.shape == (2 * H, rows) and dguT.is_contiguous()
    assert hT.shape == (H, rows) and hT.is_contiguous()
    assert torch.equal(bits(dgu), bits(c["dgu"]))
    assert torch.equal(bits(dguT), bits(c["dguT"]))
    assert torch.equal(bits(hT), bits(c["hT"]))


@pytest.mark.parametrize("rows,H", SHAPES)
def test_swiglu_bwd_t_oracle(rows, H):
    c = case(rows, H)
    dgu, _, hT = ext().swiglu_bwd_t(c["dh"], c["gu"])
    g, u = c["gu"].double().chunk(2, -1)
    s = torch.sigmoid(g)
    d = c["dh"].double()
    tag = f"[{rows}x{H}]"
    h_r = g * s * u
    rule.check("swiglu_bwd_t.hT" + tag, hT, h_r.t(), h_r.abs().t(), A_CH)
    dg_r = d * u * s * (1 + g * (1 - s))
    m_dg = (d * u).abs() * s * (1 + g.abs() * (1 - s))
    du_r = d * g * s
    rule.check("swiglu_bwd_t.dg" + tag, dgu[:, :H], dg_r, m_dg, A_CH)
    rule.check("swiglu_bwd_t.du" + tag, dgu[:, H:], du_r, du_r.abs(), A_CH)


def test_swiglu_bwd_t_rejects():
    c = case(72, 88)
    with pytest.raises(RuntimeError):       # rows % 8
        ext().swiglu_bwd_t(c["dh"][:-4], c["gu"][:-4])
    with pytest.raises(RuntimeError):       # gu is not (rows, 2H)
        ext().swiglu_bwd_t(c["dh"], c["gu"][:, :-8].contiguous())
    with pytest.raises(RuntimeError):       # not contiguous
        ext().swiglu_bwd_t(c["dh"][:, :80], c["gu"][:, :160])


@pytest.mark.parametrize("dy_pre,x_pre", [(True, False), (False, True),
                                          (True, True), (False, False)])
def test_wgrad_tn_pre_matches_wgrad_tn(dy_pre, x_pre):
    """The same GEMM on the same bits whichever side transposes."""
    torch.manual_seed(5)
    dy, x = randn(200, 192), randn(200, 128)
    want = torch.full((192, 128), float("nan"), device=dy.device, dtype=BF)
    ext().wgrad_tn(dy, x, want, False, 3)
    a = ext().transpose_bf16(dy) if dy_pre else dy
    b = ext().transpose_bf16(x) if x_pre else x
    got = torch.full_like(want, float("nan"))
    before = ext().wgrad_tn_calls()
    ext().wgrad_tn_pre(a, b, got, False, dy_pre, x_pre)
    assert ext().wgrad_tn_calls() == before + 1
    assert torch.equal(bits(got), bits(want))
    ext().wgrad_tn(dy, x, want, True, 3)
    ext().wgrad_tn_pre(a, b, got, True, dy_pre, x_pre)
    assert torch.equal(bits(got), bits(want))
    with pytest.raises(RuntimeError):       # tokens do not match
        ext().wgrad_tn_pre(a, b[:, :-8].contiguous() if x_pre else b[:-8],
                           got, False, dy_pre, x_pre)


# --------------------------------------------------------------------------
# ops.swiglu_mlp through the Llama MLP, with fake flat grad views
# --------------------------------------------------------------------------
EMB, HID, TOKENS = 64, 176, 128


def zero_thresholds(monkeypatch):
    from fms_fsdp_amd import ops
    for name in ("_WGRAD_TN_MIN_TOKENS", "_WGRAD_TN_MIN_WEIGHT",
                 "_DGRAD_TN_MIN_TOKENS", "_DGRAD_TN_MIN_WEIGHT"):
        monkeypatch.setattr(ops, name, 0)


def run_mlp(with_residual, passes=1, checkpoint=False):
    """`passes` forward+backward passes of one MLP, the first onto a NaN
    grad view marked fresh, the later ones accumulating."""
    from fms_fsdp_amd.models.llama import LlamaConfig, SwiGLU
    cfg = LlamaConfig(src_vocab_size=32, emb_dim=EMB, nheads=2, kvheads=2,
                      nlayers=1, multiple_of=16, max_expected_seq_len=64)
    assert cfg.hidden_dim == HID
    dev = "cuda:0"
    torch.manual_seed(11)
    mlp = SwiGLU(cfg)
    mlp.reset_parameters()
    mlp = mlp.to(dev).to(BF)
    fired = {}
    for n, lin in (("wg1", mlp.wg1), ("w2", mlp.w2)):
        w = lin.weight
        w._flat_grad_view = torch.full(tuple(w.shape), float("nan"),
                                       device=dev, dtype=BF)
        w._wgrad_fresh = True
        fired[n] = []
        w._wgrad_done = lambda n=n: fired[n].append(1)
    x = randn(2, TOKENS // 2, EMB).requires_grad_()
    res = randn(2, TOKENS // 2, EMB).requires_grad_() if with_residual \
        else None
    dy = randn(2, TOKENS // 2, EMB)
    w0, d0 = ext().wgrad_tn_calls(), ext().dgrad_tn_calls()
    for _ in range(passes):
        if checkpoint:
            y = torch.utils.checkpoint.checkpoint(mlp, x, res,
                                                  use_reentrant=False)
        else:
            y = mlp(x, res)
        y.backward(dy)
    return dict(y=y.detach(), dx=x.grad,
                dres=None if res is None else res.grad,
                g1=mlp.wg1.weight._flat_grad_view,
                g2=mlp.w2.weight._flat_grad_view,
                fired=(len(fired["wg1"]), len(fired["w2"])),
                fresh=(mlp.wg1.weight._wgrad_fresh,
                       mlp.w2.weight._wgrad_fresh),
                autograd=(mlp.wg1.weight.grad, mlp.w2.weight.grad),
                wgrad_calls=ext().wgrad_tn_calls() - w0,
                dgrad_calls=ext().dgrad_tn_calls() - d0)


def same(a, b):
    for k in ("y", "dx", "dres", "g1", "g2"):
        if a[k] is None:
            assert b[k] is None, k
            continue
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(bits(a[k]), bits(b[k])), k


def fused_fn_runs(monkeypatch):
    """Counts applications of the fused function."""
    from fms_fsdp_amd import ops
    calls = []
    orig = ops._SwiGLUMLPFn.apply
    monkeypatch.setattr(ops._SwiGLUMLPFn, "apply",
                        lambda *a: (calls.append(1), orig(*a))[1])
    return calls


@pytest.mark.parametrize("passes", [1, 2])          # fresh; then accumulate
@pytest.mark.parametrize("with_residual", [True, False])
def test_fused_matches_split(monkeypatch, with_residual, passes):
    zero_thresholds(monkeypatch)
    calls = fused_fn_runs(monkeypatch)
    monkeypatch.delenv("FMS_AMD_MLP_BWD", raising=False)
    new = run_mlp(with_residual, passes)
    assert len(calls) == passes
    monkeypatch.setenv("FMS_AMD_MLP_BWD", "split")
    old = run_mlp(with_residual, passes)
    assert len(calls) == passes                     # split: not applied
    same(new, old)
    for r in (new, old):
        assert r["wgrad_calls"] == 2 * passes
        assert r["dgrad_calls"] == 2 * passes
        assert r["fired"] == (passes, passes)       # once per weight and pass
        assert r["fresh"] == (False, False)
        assert r["autograd"] == (None, None)


def test_fused_under_checkpoint(monkeypatch):
    """The forward re-run by non-reentrant activation checkpointing."""
    zero_thresholds(monkeypatch)
    calls = fused_fn_runs(monkeypatch)
    monkeypatch.delenv("FMS_AMD_MLP_BWD", raising=False)
    plain = run_mlp(True, 2)
    ckpt = run_mlp(True, 2, checkpoint=True)
    assert len(calls) == 2 + 4                      # forward + its re-run
    same(ckpt, plain)
    assert ckpt["wgrad_calls"] == 4 and ckpt["dgrad_calls"] == 4
    assert ckpt["fired"] == (2, 2)


def test_fallback_below_thresholds(monkeypatch):
    """At this size the measured thresholds send every GEMM down the old
    route, and the MLP is the composition."""
    calls = fused_fn_runs(monkeypatch)
    monkeypatch.delenv("FMS_AMD_MLP_BWD", raising=False)
    r = run_mlp(True)
    assert not calls
    assert r["wgrad_calls"] == 0 and r["dgrad_calls"] == 0
    assert r["fired"] == (1, 1) and r["fresh"] == (False, False)
    for k in ("y", "dx", "dres", "g1", "g2"):
        assert torch.isfinite(r[k]).all(), k


def test_fallback_rule(monkeypatch):
    from fms_fsdp_amd import ops
    monkeypatch.delenv("FMS_AMD_MLP_BWD", raising=False)
    monkeypatch.delenv("FMS_AMD_WGRAD", raising=False)
    monkeypatch.delenv("FMS_AMD_DGRAD", raising=False)
    dev = "cuda:0"

    def weights(attach=True):
        ws = [torch.empty(2 * 11008, 4096, device=dev, dtype=BF,
                          requires_grad=True),
              torch.empty(4096, 11008, device=dev, dtype=BF,
                          requires_grad=True)]
        if attach:
            for w in ws:
                w._flat_grad_view = torch.empty(0, device=dev, dtype=BF)
        return ws

    x = torch.empty(8192, 4096, device=dev, dtype=BF)
    assert ops._mlp_bwd_fused(x, *weights())            # the 7B shape
    assert not ops._mlp_bwd_fused(x[:4096], *weights())  # too few tokens
    assert not ops._mlp_bwd_fused(x, *weights(attach=False))
    frozen = weights()
    frozen[1].requires_grad_(False)
    assert not ops._mlp_bwd_fused(x, *frozen)
    assert not ops._mlp_bwd_fused(x.float(), *weights())
    assert not ops._mlp_bwd_fused(x.cpu(), *weights())
    with torch.no_grad():
        assert not ops._mlp_bwd_fused(x, *weights())
    for var, val in (("FMS_AMD_MLP_BWD", "split"), ("FMS_AMD_WGRAD", "nt"),
                     ("FMS_AMD_DGRAD", "nn")):
        monkeypatch.setenv(var, val)
        assert not ops._mlp_bwd_fused(x, *weights())
        monkeypatch.delenv(var)
