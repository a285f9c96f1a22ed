"""The Mamba2 / hybrid model over its state caches on the GPU, in bf16: a
prefill of S0 tokens and five teacher-forced single-token steps against
the matching rows of the uncached full-sequence forward, for prompts that
end before, at and behind a chunk boundary.

Tokens are never compared: a bf16 near-tie in the logits can legitimately
flip an argmax."""

import pytest
import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.config import get_model_config
from fms_fsdp_amd.models.mamba import MambaConfig, MambaLMHeadModel

pytestmark = pytest.mark.gpu

FWD_TOL = 3e-2
BF = torch.bfloat16
B, STEPS, SPARE = 2, 5, 16


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def wide_state_cfg():
    """The step kernel at the registry models' head geometry (d_state 128,
    headdim 64), one chunk of 128; no MLP between the mixers."""
    return MambaConfig(
        d_model=256, n_layer=2, vocab_size=512, attn_layer_idx=[1],
        attn_cfg={"causal": True, "head_dim": 64, "num_heads": 4,
                  "num_heads_kv": 2, "rotary_emb_dim": 32},
        d_state=128, headdim=64, ngroups=1, chunk_size=128)


CONFIGS = {
    "mamba_test": (lambda: MambaConfig.from_dict(
        get_model_config("mamba_test")), 128, (37, 64, 91, 123)),
    "d_state128_headdim64": (wide_state_cfg, 256, (37, 128, 219, 251)),
}
_built = {}


def setup(name):
    """(model, tokens, full-forward logits), built once per config."""
    if name not in _built:
        cfg_of, ntok, _ = CONFIGS[name]
        torch.manual_seed(0)
        model = MambaLMHeadModel(cfg_of())
        model.reset_parameters()
        model = model.to(dev(), BF).eval()
        g = torch.Generator(device="cpu").manual_seed(1)
        tokens = torch.randint(0, model.config.vocab_size, (B, ntok),
                               generator=g).to(dev())
        with torch.no_grad():
            ref = model(tokens)
        _built[name] = (model, tokens, ref)
    return _built[name]


@pytest.mark.parametrize("name,S0", [(n, s) for n, c in CONFIGS.items()
                                     for s in c[2]])
def test_cached_steps_match_the_full_forward(name, S0, monkeypatch):
    monkeypatch.delenv("FMS_AMD_DECODE", raising=False)
    monkeypatch.delenv("FMS_AMD_ALLOW_TORCH_SDPA", raising=False)
    monkeypatch.delenv("FMS_AMD_FORCE_TORCH_SCAN", raising=False)
    model, tokens, ref = setup(name)
    with torch.no_grad():
        caches = model.allocate_cache(B, S0 + STEPS + SPARE, BF, dev())
        for c in caches:
            if isinstance(c, ops.KVCache):
                # a KV row past `len` that reached a result would show
                c.k.fill_(float("nan"))
                c.v.fill_(float("nan"))
        got = [model(tokens[:, :S0], caches=caches)]
        for i in range(S0, S0 + STEPS):
            got.append(model(tokens[:, i:i + 1], caches=caches))
    got = torch.cat(got, dim=1)
    n = S0 + STEPS
    assert got.shape == ref[:, :n].shape
    assert torch.isfinite(got).all()
    kinds = set()
    for c in caches:
        assert c.len == n
        kinds.add(type(c))
        if isinstance(c, ops.KVCache):
            assert not c._cat
            assert torch.isfinite(c.k[:, :n]).all()
            assert torch.isnan(c.k[:, n:]).all()
            assert torch.isnan(c.v[:, n:]).all()
        else:
            assert c.ssm.dtype == torch.float32 and c.conv.dtype == BF
            assert torch.isfinite(c.ssm).all() and c.ssm.any()
    assert kinds == {ops.KVCache, ops.MambaCache}
    err = relerr(got[:, :S0], ref[:, :S0])
    print(f"[{name} S0={S0}] prefill relerr {err:.3g}")
    assert err < FWD_TOL
    for i in range(S0, n):
        err = relerr(got[:, i], ref[:, i])
        print(f"[{name} S0={S0}] step {i} relerr {err:.3g}")
        assert err < FWD_TOL, i


def test_batch_of_one_with_a_prompt_of_whole_attention_tiles():
    """b = 1 and a 128-token prompt: the prefill hands the attention
    kernel unpadded views of a cache that is longer than the prompt."""
    model, tokens, ref = setup("d_state128_headdim64")
    S0 = 128
    with torch.no_grad():
        caches = model.allocate_cache(1, S0 + 1 + SPARE, BF, dev())
        got = torch.cat([model(tokens[:1, :S0], caches=caches),
                         model(tokens[:1, S0:S0 + 1], caches=caches)], dim=1)
    assert all(c.len == S0 + 1 for c in caches)
    err = relerr(got[:, :S0], ref[:1, :S0])
    err1 = relerr(got[:, S0], ref[:1, S0])
    print(f"[b=1 S0={S0}] prefill relerr {err:.3g}, step relerr {err1:.3g}")
    assert err < FWD_TOL and err1 < FWD_TOL


@pytest.mark.parametrize("name", list(CONFIGS))
def test_generate_runs_end_to_end(name):
    model, tokens, _ = setup(name)
    prompt = tokens[:, :37]
    out, emb = model.generate(prompt, 4, do_sample=False,
                              include_embeds=True)
    assert out.shape == (B, 41) and torch.equal(out[:, :37], prompt)
    assert emb.shape == (B, 4, model.config.d_model)
    assert torch.isfinite(emb).all()
    assert int(out.min()) >= 0 and int(out.max()) < model.config.vocab_size
    assert model.generate(prompt, 4).shape == (B, 41)
