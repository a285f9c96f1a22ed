"""CPU checks of the preallocated KV cache (ops.KVCache and the ops around
it), of generation on top of it, and of the split plan (attn_decode_plan.h,
through a stand-alone C++ program as tests/test_attn_ws_cpu.py does for
attn_ws.h)."""

import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference

HIP_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                       "fms_fsdp_amd", "ops", "hip")

B, H, KVH, D = 2, 4, 2, 8


def tables(n, d=D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.outer(torch.arange(n, dtype=torch.float32), inv)
    return fr.cos(), fr.sin()


def qkv_steps(chunks, seed=0):
    """Per step a fused (b, s, (h+2kvh)*d) projection and its q/k/v slices,
    as the models pass them."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in chunks:
        fused = torch.randn(B, s, (H + 2 * KVH) * D, generator=g)
        q, k, v = fused.split([H * D, KVH * D, KVH * D], dim=-1)
        out.append((q.view(B, s, H, D), k.view(B, s, KVH, D),
                    v.view(B, s, KVH, D)))
    return out


def dict_route(q, k, v, cache, cos, sin):
    """The cat-grown dict cache of Attention.forward before KVCache."""
    if cos is not None:
        q, k = ops.rope_apply(q, k, cos, sin)
    if cache.get("k") is not None:
        k = torch.cat([cache["k"], k], dim=1)
        v = torch.cat([cache["v"], v], dim=1)
    cache["k"], cache["v"] = k, v
    return F.scaled_dot_product_attention(
        q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
        is_causal=(q.shape[1] == k.shape[1]),
        enable_gqa=(KVH != H)).transpose(1, 2)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
def test_same_as_the_cat_route(rope):
    chunks = [5, 1, 1, 1]
    cos, sin = tables(sum(chunks))
    cache = ops.KVCache(B, sum(chunks), KVH, D, torch.float32, "cpu")
    old = {}
    pos = 0
    with torch.no_grad():
        for q, k, v in qkv_steps(chunks):
            s = q.shape[1]
            cs = (cos[pos:pos + s], sin[pos:pos + s]) if rope else (None, None)
            o_new = ops.attention_cached(q, k, v, cache, *cs)
            o_old = dict_route(q, k, v, old, *cs)
            pos += s
            assert cache.len == pos
            assert torch.equal(cache.k[:, :pos], old["k"])
            assert torch.equal(cache.v[:, :pos], old["v"])
            # same fp32 SDPA call on the same values; the operands differ
            # in their strides only
            torch.testing.assert_close(o_new, o_old, rtol=0, atol=1e-6)


def test_append_returns_rotated_q_and_plain_q():
    (q, k, v), = qkv_steps([3])
    cos, sin = tables(3)
    with torch.no_grad():
        c = ops.KVCache(B, 4, KVH, D, torch.float32, "cpu")
        qr = ops.kv_cache_append(c, q, k, v, cos, sin)
        q_ref, k_ref = reference.rope_apply(q, k, cos, sin)
        assert torch.equal(qr, q_ref) and torch.equal(c.k[:, :3], k_ref)
        assert torch.equal(c.v[:, :3], v)
        c2 = ops.KVCache(B, 4, KVH, D, torch.float32, "cpu")
        q2 = ops.kv_cache_append(c2, q, k, v)
        assert torch.equal(q2, q) and torch.equal(c2.k[:, :3], k)


def test_chunked_prefill_equals_the_full_causal_forward():
    chunks = [5, 4, 1, 1]
    n = sum(chunks)
    cos, sin = tables(n)
    steps = qkv_steps(chunks, seed=1)
    qf, kf, vf = (torch.cat([st[i] for st in steps], dim=1) for i in range(3))
    with torch.no_grad():
        qr, kr = ops.rope_apply(qf, kf, cos, sin)
        full = ops.attention_causal(qr, kr, vf)
        cache = ops.KVCache(B, n, KVH, D, torch.float32, "cpu")
        pos = 0
        for q, k, v in steps:
            s = q.shape[1]
            o = ops.attention_cached(q, k, v, cache, cos[pos:pos + s],
                                     sin[pos:pos + s])
            torch.testing.assert_close(o, full[:, pos:pos + s], rtol=1e-5,
                                       atol=1e-6)
            pos += s


def test_append_past_capacity_raises_and_keeps_len():
    cache = ops.KVCache(B, 6, KVH, D, torch.float32, "cpu")
    (q, k, v), (q1, k1, v1), (q2, k2, v2) = qkv_steps([5, 1, 2])
    with torch.no_grad():
        ops.kv_cache_append(cache, q, k, v)
        with pytest.raises(ValueError):
            ops.kv_cache_append(cache, q2, k2, v2)
        assert cache.len == 5
        kept = cache.k.clone()
        with pytest.raises(ValueError):
            ops.attention_cached(q2, k2, v2, cache)
        assert cache.len == 5 and torch.equal(cache.k[:, :5], kept[:, :5])
        ops.kv_cache_append(cache, q1, k1, v1)
        assert cache.len == 6 and cache.capacity == 6


def test_grad_enabled_input_raises():
    cache = ops.KVCache(B, 6, KVH, D, torch.float32, "cpu")
    (q, k, v), = qkv_steps([2])
    k = k.clone().requires_grad_()
    with pytest.raises(RuntimeError):
        ops.kv_cache_append(cache, q, k, v)
    with pytest.raises(RuntimeError):
        ops.attention_cached(q, k, v, cache)
    assert cache.len == 0
    with torch.no_grad():
        ops.attention_cached(q, k, v, cache)
    assert cache.len == 2
    with pytest.raises(RuntimeError):
        ops.attention_decode(q[:, :1].clone().requires_grad_(), cache)


def test_decode_needs_one_query_and_a_filled_cache():
    cache = ops.KVCache(B, 6, KVH, D, torch.float32, "cpu")
    (q, k, v), = qkv_steps([2])
    with torch.no_grad():
        with pytest.raises(ValueError):
            ops.attention_decode(q[:, :1], cache)
        ops.kv_cache_append(cache, q, k, v)
        with pytest.raises(ValueError):
            ops.attention_decode(q, cache)


def test_sdpa_switch_selects_the_former_route(monkeypatch):
    chunks = [4, 1, 1]
    cos, sin = tables(sum(chunks))
    outs = {}
    for mode in ("", "sdpa"):
        monkeypatch.setenv("FMS_AMD_DECODE", mode)
        cache = ops.KVCache(B, sum(chunks), KVH, D, torch.float32, "cpu")
        pos, o = 0, []
        with torch.no_grad():
            for q, k, v in qkv_steps(chunks, seed=2):
                s = q.shape[1]
                o.append(ops.attention_cached(q, k, v, cache,
                                              cos[pos:pos + s],
                                              sin[pos:pos + s]))
                pos += s
        assert cache.len == pos
        assert (cache._cat.get("k") is not None) == (mode == "sdpa")
        outs[mode] = torch.cat(o, dim=1)
    torch.testing.assert_close(outs[""], outs["sdpa"], rtol=0, atol=1e-6)


# --------------------------------------------------------------------------
# generation
# --------------------------------------------------------------------------
class _Spy:
    """Records the KVCache objects generate() allocates."""

    def __init__(self, monkeypatch):
        self.made = []
        real = ops.KVCache

        class Recording(real):
            def __init__(inner, *a, **kw):
                super().__init__(*a, **kw)
                self.made.append(inner)
        monkeypatch.setattr(ops, "KVCache", Recording)


def _greedy_matches_full_forward(m, x, new):
    toks = m.generate(x, new, do_sample=False)
    assert toks.shape == (x.shape[0], x.shape[1] + new)
    with torch.no_grad():
        for i in range(new):
            n = x.shape[1] + i
            logits = m(toks[:, :n])
            assert torch.equal(toks[:, n], logits[:, -1].argmax(-1)), i


def test_llama_greedy_generation(narrow_model_factory, monkeypatch):
    torch.manual_seed(0)
    spy = _Spy(monkeypatch)
    m = narrow_model_factory.create().eval()
    x = torch.randint(0, 32, (2, 6))
    _greedy_matches_full_forward(m, x, 4)
    assert len(spy.made) == len(m.layers)
    for c in spy.made:
        assert c.k.shape == (2, 10, 1, 8) and c.v.shape == c.k.shape
        assert c.len == 9          # the last token is sampled, not appended


def test_gpt_bigcode_greedy_generation(monkeypatch):
    from fms_fsdp_amd.config import get_model_config
    from fms_fsdp_amd.models.gpt_bigcode import GPTBigCode
    torch.manual_seed(3)
    spy = _Spy(monkeypatch)
    m = GPTBigCode(get_model_config("gpt_bigcode_test"))
    m.reset_parameters()
    m.eval()
    _greedy_matches_full_forward(m, torch.randint(0, 256, (2, 16)), 3)
    assert len(spy.made) == len(m.layers)
    assert all(c.k.shape[2] == 1 and c.len == 18 for c in spy.made)


def test_mixtral_greedy_generation(monkeypatch):
    from fms_fsdp_amd.config import get_model_config
    from fms_fsdp_amd.models.mixtral import Mixtral
    torch.manual_seed(4)
    spy = _Spy(monkeypatch)
    m = Mixtral(get_model_config("mixtral_test"))
    m.reset_parameters()
    m.eval()
    _greedy_matches_full_forward(m, torch.randint(0, 256, (2, 16)), 3)
    assert len(spy.made) == len(m.layers)
    assert all(c.len == 18 for c in spy.made)


def test_dict_cache_keeps_the_former_path(narrow_model_factory):
    """A plain dict still grows by torch.cat inside Attention.forward."""
    torch.manual_seed(0)
    m = narrow_model_factory.create().eval()
    attn = m.layers[0].attn
    cos, sin = m.rot_emb.get(5, torch.device("cpu"))
    cache = {}
    with torch.no_grad():
        attn(torch.randn(1, 4, 16), cos[:4], sin[:4], cache)
        attn(torch.randn(1, 1, 16), cos[4:5], sin[4:5], cache)
    assert cache["k"].shape == (1, 5, 1, 8)


# --------------------------------------------------------------------------
# split plan
# --------------------------------------------------------------------------
N_CU = 256
PLAN_LENS = [1, 31, 32, 33, 64, 255, 256, 257, 320, 1024, 4096, 16384, 65536,
             1 << 20]
PLAN_UNITS = [(96, 32), (96, 8), (96, 1), (1, 8), (1, 1), (4, 2), (3, 1)]

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "attn_decode_plan.h"
int main(int argc, char** argv) {
  printf("tile %d\n", (int)ATTN_DECODE_KEY_TILE);
  for (int i = 1; i + 3 < argc; i += 4) {
    const long long b = atoll(argv[i]), kvh = atoll(argv[i + 1]),
                    n = atoll(argv[i + 2]), cu = atoll(argv[i + 3]);
    printf("%lld %lld %lld %lld %lld %lld %lld\n", b, kvh, n, cu,
           (long long)attn_decode_plan(b, kvh, n, cu),
           (long long)attn_decode_tiles(n),
           (long long)attn_decode_clamp_splits(1000000, n));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("attn_decode_plan")
    src, exe = d / "main.cpp", d / "plan_main"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", HIP_DIR, str(src), "-o", str(exe)])
    cases = [(b, kvh, n, N_CU) for b, kvh in PLAN_UNITS for n in PLAN_LENS]
    args = [str(v) for case in cases for v in case]
    out = subprocess.check_output([str(exe)] + args, text=True).splitlines()
    table = {"tile": int(out[0].split()[1])}
    for line in out[1:]:
        b, kvh, n, cu, splits, tiles, clamped = map(int, line.split())
        table[(b, kvh, n)] = (splits, tiles, clamped)
    assert len(table) == len(cases) + 1
    return table


def test_plan_is_one_at_stage2_shapes(plan):
    for n in PLAN_LENS:
        assert plan[(96, 32, n)][0] == 1
    for kvh in (8, 1):          # llama3-8B, StarCoder at stage-2 lengths
        for n in (64, 320):
            assert plan[(96, kvh, n)][0] == 1


def test_plan_never_exceeds_the_tile_count(plan):
    tile = plan["tile"]
    for b, kvh in PLAN_UNITS:
        for n in PLAN_LENS:
            splits, tiles, clamped = plan[(b, kvh, n)]
            assert tiles == -(-n // tile)
            assert 1 <= splits <= tiles
            assert clamped == tiles        # a huge request is clamped


def test_plan_is_non_decreasing_in_kv_len(plan):
    for b, kvh in PLAN_UNITS:
        got = [plan[(b, kvh, n)][0] for n in PLAN_LENS]
        assert got == sorted(got), (b, kvh, got)


def test_plan_splits_a_long_single_row(plan):
    """b1 kvh8 with 16k keys: 8 workgroups would leave 248 of 256 CUs
    idle."""
    assert plan[(1, 8, 16384)][0] > 1
    assert plan[(1, 8, 16384)][0] * 8 >= N_CU
