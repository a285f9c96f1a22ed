"""The attention modules over an ops.KVCache on the GPU: a 37-token prefill
and five decode steps against the matching rows of the uncached
full-sequence forward, and the FMS_AMD_DECODE=sdpa switch (the former
torch.cat + SDPA route) against the kernels on the same inputs.

Tokens are never compared between the routes: a bf16 near-tie in the
logits can legitimately flip an argmax."""

import pytest
import torch

from fms_fsdp_amd import ops

pytestmark = pytest.mark.gpu

FWD_TOL = 3e-2
BF = torch.bfloat16
B, S0, STEPS = 2, 37, 5


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def llama_attention():
    from fms_fsdp_amd.models.llama import (Attention, LlamaConfig,
                                           RotaryEmbedding)
    cfg = LlamaConfig(src_vocab_size=64, emb_dim=1024, nheads=8, kvheads=2,
                      nlayers=1, max_expected_seq_len=64)
    torch.manual_seed(0)
    attn = Attention(cfg)
    attn.reset_parameters()
    rot = RotaryEmbedding(cfg.head_dim, 64, cfg.rope_theta)
    cos, sin = rot.get(S0 + STEPS, torch.device("cpu"))
    return attn.to(dev(), BF).eval(), cfg, cos.to(dev()), sin.to(dev())


def bigcode_attention():
    from fms_fsdp_amd.models.gpt_bigcode import (BigCodeAttention,
                                                 GPTBigCodeConfig)
    cfg = GPTBigCodeConfig(src_vocab_size=64, emb_dim=384, nheads=6,
                           nlayers=1, max_expected_seq_len=64)
    torch.manual_seed(1)
    attn = BigCodeAttention(cfg)
    attn.reset_parameters()
    return attn.to(dev(), BF).eval(), cfg


def hidden(emb_dim, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(B, S0 + STEPS, emb_dim, generator=g).to(dev(), BF)


def run_cached(step_fn, cache_of, x):
    """Prefill of S0 tokens, then STEPS single tokens; outputs joined."""
    cache = cache_of()
    outs = [step_fn(x[:, :S0], 0, S0, cache)]
    for i in range(S0, S0 + STEPS):
        outs.append(step_fn(x[:, i:i + 1], i, i + 1, cache))
    return torch.cat(outs, dim=1), cache


def llama_runner():
    attn, cfg, cos, sin = llama_attention()
    x = hidden(cfg.emb_dim, 10)

    def step(xs, lo, hi, cache):
        return attn(xs, cos[lo:hi], sin[lo:hi], cache)

    def cache_of():
        return ops.KVCache(B, S0 + STEPS, cfg.kvheads, cfg.head_dim, BF,
                           dev())

    def full():
        return attn(x, cos, sin)
    return x, step, cache_of, full


def bigcode_runner():
    attn, cfg = bigcode_attention()
    x = hidden(cfg.emb_dim, 11)

    def step(xs, lo, hi, cache):
        return attn(xs, cache)

    def cache_of():
        return ops.KVCache(B, S0 + STEPS, 1, cfg.head_dim, BF, dev())

    def full():
        return attn(x)
    return x, step, cache_of, full


RUNNERS = {"llama_h8_kvh2_d128": llama_runner,
           "bigcode_h6_d64": bigcode_runner}


@pytest.mark.parametrize("name", list(RUNNERS))
def test_cached_steps_match_the_full_forward(name, monkeypatch):
    monkeypatch.delenv("FMS_AMD_DECODE", raising=False)
    monkeypatch.delenv("FMS_AMD_ALLOW_TORCH_SDPA", raising=False)
    x, step, cache_of, full = RUNNERS[name]()
    with torch.no_grad():
        ref = full()
        got, cache = run_cached(step, cache_of, x)
    assert cache.len == S0 + STEPS and not cache._cat
    assert got.shape == ref.shape
    err = relerr(got[:, :S0], ref[:, :S0])
    print(f"[{name}] prefill relerr {err:.3g}")
    assert err < FWD_TOL
    for i in range(S0, S0 + STEPS):
        err = relerr(got[:, i], ref[:, i])
        print(f"[{name}] step {i} relerr {err:.3g}")
        assert err < FWD_TOL, i


@pytest.mark.parametrize("name", list(RUNNERS))
def test_sdpa_switch_gives_the_former_route(name, monkeypatch):
    monkeypatch.delenv("FMS_AMD_ALLOW_TORCH_SDPA", raising=False)
    x, step, cache_of, _ = RUNNERS[name]()
    with torch.no_grad():
        monkeypatch.delenv("FMS_AMD_DECODE", raising=False)
        new, c_new = run_cached(step, cache_of, x)
        monkeypatch.setenv("FMS_AMD_DECODE", "sdpa")
        old, c_old = run_cached(step, cache_of, x)
    assert not c_new._cat and c_old._cat["k"].shape[1] == S0 + STEPS
    # the kernels wrote the same keys the cat route grew
    assert torch.equal(c_new.k[:, :c_new.len], c_old._cat["k"])
    assert torch.equal(c_new.v[:, :c_new.len], c_old._cat["v"])
    for i in range(S0 + STEPS):
        err = relerr(new[:, i], old[:, i])
        assert err < FWD_TOL, (i, err)
    print(f"[{name}] kernels vs sdpa route: {relerr(new, old):.3g}")
