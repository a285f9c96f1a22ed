"""Mamba2 recurrent decode without a GPU: the float64 oracles of the step
ops against the chunked scan and the whole-row conv, and the model's
cached forward (prefill + single-token steps) against its uncached
forward, in fp32."""

import pytest
import torch
import torch.nn.functional as F

from fms_fsdp_amd import ops
from fms_fsdp_amd.config import get_model_config
from fms_fsdp_amd.models.mamba import (MambaConfig, MambaLMHeadModel,
                                       ssd_chunked)
from fms_fsdp_amd.ops import reference

DD = torch.float64


def relmax(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def step_inputs(b, T, H, G, P, N, seed):
    g = torch.Generator().manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=g, dtype=DD)
    return dict(
        x=rn(b, T, H * P), dt=rn(b, T, H) * 0.5, B=rn(b, T, G * N),
        C=rn(b, T, G * N), z=rn(b, T, H * P), dt_bias=rn(H) * 0.3 - 1.0,
        A_log=torch.log(torch.rand(H, generator=g, dtype=DD) * 2 + 0.05),
        D=rn(H))


def run_steps(inp, state, H, G, P, N, lo=None, hi=None):
    sl = slice(lo, hi)
    return reference.ssd_state_update(
        state, inp["x"][:, sl], inp["dt"][:, sl], inp["B"][:, sl],
        inp["C"][:, sl], inp["z"][:, sl], inp["dt_bias"], inp["A_log"],
        inp["D"], H, G, P, N)


@pytest.mark.parametrize("H,G", [(4, 1), (4, 2)])
def test_state_update_matches_the_chunked_scan(H, G):
    b, T, P, N, Q = 2, 96, 8, 16, 32
    inp = step_inputs(b, T, H, G, P, N, seed=H * 10 + G)
    state = torch.zeros(b, H, P, N, dtype=DD)
    out = run_steps(inp, state, H, G, P, N)

    # the chunked scan computes in fp32 (as the model calls it)
    dtf = F.softplus(inp["dt"] + inp["dt_bias"]).float()
    A = -torch.exp(inp["A_log"]).float()
    xh = inp["x"].view(b, T, H, P).float()
    Bh = inp["B"].view(b, T, G, N).float()
    Ch = inp["C"].view(b, T, G, N).float()
    y, final = ssd_chunked(xh, dtf, A, Bh, Ch, Q, return_final_state=True)
    y = (y + xh * inp["D"].float().view(1, 1, H, 1)).reshape(b, T, H * P)
    ref = y.double() * F.silu(inp["z"])
    assert final.shape == (b, H, P, N) and final.dtype == torch.float32
    e_y, e_s = relmax(out, ref), relmax(state, final.double())
    print(f"[H={H},G={G}] y {e_y:.3g} state {e_s:.3g}")
    assert e_y < 1e-4
    assert e_s < 1e-4
    # default calls return y alone
    assert torch.is_tensor(ssd_chunked(xh, dtf, A, Bh, Ch, Q))


def test_state_update_split_calls_are_bit_identical():
    b, H, G, P, N = 2, 4, 2, 8, 16
    inp = step_inputs(b, 5, H, G, P, N, seed=3)
    s0 = torch.randn(b, H, P, N, dtype=DD)
    s_one, s_two = s0.clone(), s0.clone()
    one = run_steps(inp, s_one, H, G, P, N)
    two = torch.cat([run_steps(inp, s_two, H, G, P, N, 0, 2),
                     run_steps(inp, s_two, H, G, P, N, 2, 5)], dim=1)
    assert torch.equal(one, two)
    assert torch.equal(s_one, s_two)
    assert not torch.equal(s_one, s0)


@pytest.mark.parametrize("W", [2, 3, 4])
def test_conv_update_in_pieces_matches_the_whole_row(W):
    torch.manual_seed(W)
    b, L, C = 2, 9, 24
    x = torch.randn(b, L, C, dtype=DD)
    w = torch.randn(C, W, dtype=DD)
    bias = torch.randn(C, dtype=DD)
    ref = reference.causal_conv1d(x, w, bias)
    state = torch.zeros(b, W - 1, C, dtype=DD)
    ys, lo = [], 0
    for n in (1, 2, 5, 1):
        ys.append(reference.causal_conv1d_update(state, x[:, lo:lo + n], w,
                                                 bias))
        lo += n
        # the last W-1 rows of [zeros | x[:lo]]
        seen = torch.cat([torch.zeros(b, W - 1, C, dtype=DD), x[:, :lo]], 1)
        assert torch.equal(state, seen[:, seen.shape[1] - (W - 1):])
    got = torch.cat(ys, dim=1)
    assert got.shape == ref.shape
    assert relmax(got, ref) < 1e-12
    assert torch.equal(state, x[:, L - (W - 1):])


def test_ops_dispatch_to_the_reference_on_the_cpu():
    b, H, G, P, N = 1, 2, 1, 8, 16
    inp = {k: v.float() for k, v in
           step_inputs(b, 3, H, G, P, N, seed=5).items()}
    s_a = torch.zeros(b, H, P, N)
    s_b = torch.zeros(b, H, P, N)
    args = (inp["x"], inp["dt"], inp["B"], inp["C"], inp["z"],
            inp["dt_bias"], inp["A_log"], inp["D"], H, G, P, N)
    assert torch.equal(ops.ssd_state_update(s_a, *args),
                       reference.ssd_state_update(s_b, *args))
    assert torch.equal(s_a, s_b)
    cache = ops.MambaCache(3, 40, 4, H, P, N, torch.float32, "cpu")
    assert cache.conv.shape == (3, 3, 40) and cache.ssm.shape == (3, H, P, N)
    assert cache.ssm.dtype == torch.float32 and cache.len == 0
    assert not cache.conv.any() and not cache.ssm.any()
    with pytest.raises(RuntimeError):
        ops.ssd_state_update(s_a, inp["x"].requires_grad_(), *args[1:])
    with pytest.raises(RuntimeError):
        ops.causal_conv1d_update(
            torch.zeros(1, 3, 8), torch.randn(1, 2, 8),
            torch.randn(8, 4, requires_grad=True), torch.zeros(8))


# ---------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------
L_TOK, STEPS = 128, 5


@pytest.fixture(scope="module")
def hybrid():
    torch.manual_seed(0)
    model = MambaLMHeadModel(
        MambaConfig.from_dict(get_model_config("mamba_test")))
    model.reset_parameters()
    model.eval()
    tokens = torch.randint(0, model.config.vocab_size, (2, L_TOK),
                           generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = model(tokens)
    return model, tokens, ref


@pytest.mark.parametrize("S0", [37, 64, 91, 123])
def test_cached_forward_matches_the_full_forward(hybrid, S0):
    model, tokens, ref = hybrid
    with torch.no_grad():
        caches = model.allocate_cache(2, S0 + STEPS, torch.float32, "cpu")
        assert isinstance(caches[0], ops.MambaCache)
        assert isinstance(caches[1], ops.KVCache)
        got = [model(tokens[:, :S0], caches=caches)]
        for i in range(S0, S0 + STEPS):
            got.append(model(tokens[:, i:i + 1], caches=caches))
    got = torch.cat(got, dim=1)
    assert all(c.len == S0 + STEPS for c in caches)
    err = relmax(got[:, :S0], ref[:, :S0])
    print(f"[S0={S0}] prefill {err:.3g}")
    assert err < 1e-4
    for i in range(S0, S0 + STEPS):
        err = relmax(got[:, i], ref[:, i])
        print(f"[S0={S0}] step {i} {err:.3g}")
        assert err < 1e-4, i


def test_generate_shapes(hybrid):
    model, tokens, _ = hybrid
    prompt = tokens[:, :11]
    out = model.generate(prompt, 4, do_sample=False)
    assert out.shape == (2, 15) and torch.equal(out[:, :11], prompt)
    out2, emb = model.generate(prompt, 4, do_sample=False,
                               include_embeds=True)
    assert torch.equal(out, out2)
    assert emb.shape == (2, 4, model.config.d_model)
    assert model.generate(prompt, 3).shape == (2, 14)


def test_cache_with_doc_mask_raises(hybrid):
    model, tokens, _ = hybrid
    caches = model.allocate_cache(2, 16, torch.float32, "cpu")
    start = torch.zeros(2, 8, dtype=torch.int32)
    mask = ops.doc_mask_from_starts(start)
    with torch.no_grad():
        with pytest.raises(ValueError):
            model(tokens[:, :8], doc_mask=mask, caches=caches)
        x = torch.randn(2, 8, model.config.d_model)
        for layer, cache in zip(model.layers, caches):
            with pytest.raises(ValueError):
                layer.mixer(x, doc_mask=mask, cache=cache)
    assert all(c.len == 0 for c in caches)


def test_cached_forward_under_grad_raises(hybrid):
    model, tokens, _ = hybrid
    caches = model.allocate_cache(2, 80, torch.float32, "cpu")
    with pytest.raises(RuntimeError):
        model(tokens[:, :64], caches=caches)      # a whole chunk, no tail
    caches = model.allocate_cache(2, 80, torch.float32, "cpu")
    with pytest.raises(RuntimeError):
        model(tokens[:, :1], caches=caches)
