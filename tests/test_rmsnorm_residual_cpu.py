"""ops.rmsnorm_residual and the direct-wgrad protocol of Llama's norm
weights on the paths that never reach the kernels (CPU reference)."""

import copy

import torch

from fms_fsdp_amd import ops


def test_rmsnorm_residual_grad_matches_two_uses_of_x():
    """The op is the norm plus a pass-through of x: its gradient is what
    plain autograd gives when x feeds the norm and the residual add."""
    torch.manual_seed(0)
    x = torch.randn(3, 5, 16)
    w = torch.randn(16)
    gy, gr = torch.randn(3, 5, 16), torch.randn(3, 5, 16)

    x1, w1 = x.clone().requires_grad_(), w.clone().requires_grad_()
    y1, r1 = ops.rmsnorm_residual(x1, w1, 1e-6)
    assert torch.equal(r1, x1)
    (y1 * gy + r1 * gr).sum().backward()

    x2, w2 = x.clone().requires_grad_(), w.clone().requires_grad_()
    y2 = ops.rmsnorm(x2, w2, 1e-6)
    (y2 * gy + x2 * gr).sum().backward()

    assert torch.equal(y1, y2)
    torch.testing.assert_close(x1.grad, x2.grad, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(w1.grad, w2.grad, rtol=1e-6, atol=1e-6)


def _tiny():
    from fms_fsdp_amd.models import Llama, LlamaConfig
    cfg = LlamaConfig(src_vocab_size=64, emb_dim=32, nheads=4, kvheads=2,
                      nlayers=2, max_expected_seq_len=32)
    m = Llama(cfg)
    torch.manual_seed(3)
    m.reset_parameters()
    with torch.no_grad():      # norm weights off their all-ones init
        for n, p in m.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    return m


def _norm_slices(sm):
    """{param name: its slice of the flat grad buffer} of the norm weights"""
    out = {}
    for u in sm.all_units:
        for n, p, off in zip(u.param_names, u.params, u.offsets):
            if "norm" in n:
                out[n] = u.flat_grad[off:off + p.numel()]
    return out


def test_wrapped_llama_norm_grads_land_in_flat_buffer():
    from fms_fsdp_amd.models import LlamaBlock
    from fms_fsdp_amd.parallel import ShardedModel

    plain = _tiny()
    wrapped = copy.deepcopy(plain)
    for p_, w_ in zip(plain.parameters(), wrapped.parameters()):
        if getattr(p_, "_direct_wgrad", False):   # deepcopy drops attributes
            w_._direct_wgrad = True
    sm = ShardedModel(wrapped, LlamaBlock, sharding_strategy="fsdp",
                      param_dtype=torch.float32)
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, 64, (2, 16), generator=g)
    y = torch.randint(0, 64, (2, 16), generator=g)

    norm_names = [n for n, _ in plain.named_parameters() if "norm" in n]
    assert len(norm_names) == 5      # 2 per block, 1 final
    for n, p in wrapped.named_parameters():
        if "norm" in n:
            assert getattr(p, "_direct_wgrad", False), n
            assert p._flat_grad_view is not None and p.grad is None

    sm.zero_grad()
    sm(x, labels=y).backward()
    plain(x, labels=y).backward()
    ref = dict(plain.named_parameters())
    slices = _norm_slices(sm)
    assert sorted(slices) == sorted(norm_names)
    for n, sl in slices.items():
        assert ref[n].grad.abs().max() > 0
        torch.testing.assert_close(sl, ref[n].grad, rtol=1e-5, atol=1e-6,
                                   msg=lambda m, n=n: f"{n}: {m}")
    # autograd never saw these weights' grads
    for n, p in wrapped.named_parameters():
        if "norm" in n:
            assert p.grad is None, n
    # every unit's countdown completed: the norm callbacks fired
    assert all(u._grad_countdown == 0 for u in sm.all_units)

    # a second backward without zero_grad accumulates
    sm(x, labels=y).backward()
    for n, sl in _norm_slices(sm).items():
        torch.testing.assert_close(sl, 2 * ref[n].grad, rtol=1e-5, atol=1e-6,
                                   msg=lambda m, n=n: f"{n}: {m}")

    # zero_grad marks the slices fresh: the next backward overwrites
    sm.zero_grad()
    sm(x, labels=y).backward()
    for n, sl in _norm_slices(sm).items():
        torch.testing.assert_close(sl, ref[n].grad, rtol=1e-5, atol=1e-6,
                                   msg=lambda m, n=n: f"{n}: {m}")
