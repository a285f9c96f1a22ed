"""ops.swiglu_mlp where the fused backward does not apply (CPU, no
extension needed): it is the composition linear_flat -> swiglu ->
linear_flat, forward and grads, and agrees with ops/reference.py."""

import pytest
import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference


def inputs(with_residual):
    torch.manual_seed(0)
    x = torch.randn(2, 5, 16)
    wg1 = torch.randn(2 * 24, 16) * 0.3
    w2 = torch.randn(16, 24) * 0.3
    res = torch.randn(2, 5, 16) if with_residual else None
    return x, wg1, w2, res, torch.randn(2, 5, 16)


def grads(fn, with_residual, attach=False):
    x, wg1, w2, res, dy = inputs(with_residual)
    leaves = [t.requires_grad_() for t in (x, wg1, w2, res) if t is not None]
    views = []
    if attach:      # the direct-wgrad protocol of the sharded runtime
        for w in (wg1, w2):
            w._flat_grad_view = torch.full_like(w, float("nan")).detach()
            w._wgrad_fresh = True
            views.append(w._flat_grad_view)
    y = fn(x, wg1, w2, res)
    y.backward(dy)
    return [y.detach()] + [t.grad for t in leaves] + views


def composition(x, wg1, w2, res):
    return ops.linear_flat(ops.swiglu(ops.linear_flat(x, wg1)), w2, res)


def by_reference(x, wg1, w2, res):
    y = reference.swiglu(x @ wg1.t()) @ w2.t()
    return y if res is None else y + res


@pytest.mark.parametrize("with_residual", [False, True])
def test_swiglu_mlp_is_the_composition(with_residual):
    assert not ops._mlp_bwd_fused(torch.randn(10, 16), torch.randn(48, 16),
                                  torch.randn(16, 24))
    got = grads(ops.swiglu_mlp, with_residual)
    for g, w in zip(got, grads(composition, with_residual)):
        assert torch.equal(g, w)
    for g, w in zip(got, grads(by_reference, with_residual)):
        torch.testing.assert_close(g, w, rtol=1e-5, atol=1e-5)


def test_swiglu_mlp_flat_grad_views_on_cpu():
    """Attached weights on the CPU: still the composition, grads in the
    views and none for autograd."""
    got = grads(ops.swiglu_mlp, True, attach=True)
    want = grads(by_reference, True)
    y, dx, dwg1, dw2, dres, g1, g2 = got
    assert dwg1 is None and dw2 is None
    for g, w in zip((y, dx, g1, g2, dres), want):
        torch.testing.assert_close(g, w, rtol=1e-5, atol=1e-5)


def test_llama_mlp_uses_swiglu_mlp(monkeypatch):
    from fms_fsdp_amd.models.llama import LlamaConfig, SwiGLU
    seen = []
    orig = ops.swiglu_mlp
    monkeypatch.setattr(ops, "swiglu_mlp",
                        lambda *a: (seen.append(1), orig(*a))[1])
    torch.manual_seed(1)
    mlp = SwiGLU(LlamaConfig(src_vocab_size=32, emb_dim=16, nheads=2,
                             kvheads=1, nlayers=1, multiple_of=8))
    x, res = torch.randn(2, 3, 16), torch.randn(2, 3, 16)
    y = mlp(x, res)
    assert seen == [1]
    want = reference.swiglu(x @ mlp.wg1.weight.t()) @ mlp.w2.weight.t() + res
    torch.testing.assert_close(y, want, rtol=1e-5, atol=1e-5)
