"""_C.kv_append (kv_append_kernel, attn_decode.hip): split + RoPE + cache
append in one launch. Rotated q and the k rows written must carry the bits
of _C.rope_fwd on the same inputs, the v rows the bits of their source, and
no cache row outside [pos, pos + s) may change. Inputs are slices of a
fused (b, s, (h+2kvh)*d) projection and, separately, contiguous tensors."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B = 2
TAIL = 3        # cache rows behind the appended ones


def dev():
    return torch.device("cuda:0")


def ext():
    from fms_fsdp_amd import _C
    return _C


def inputs(s, d, h, kvh, fused, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 7 * s + d + 31 * h)
    buf = torch.randn(B, s, (h + 2 * kvh) * d, generator=g).to(dev(), BF)
    q, k, v = buf.split([h * d, kvh * d, kvh * d], dim=-1)
    q, k, v = (q.view(B, s, h, d), k.view(B, s, kvh, d),
               v.view(B, s, kvh, d))
    if not fused:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return q, k, v


def tables(pos, s, d):
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.outer(torch.arange(pos, pos + s, dtype=torch.float32), inv)
    return fr.cos().to(dev()).contiguous(), fr.sin().to(dev()).contiguous()


def sentinel_cache(cap, kvh, d):
    n = B * cap * kvh * d
    pat = (torch.arange(n, device=dev()) % 251 - 125).to(BF)
    return pat.view(B, cap, kvh, d).clone(), (-pat).view(B, cap, kvh, d).clone()


def untouched(cache, before, pos, s):
    return (torch.equal(cache[:, :pos], before[:, :pos])
            and torch.equal(cache[:, pos + s:], before[:, pos + s:]))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "contig"])
@pytest.mark.parametrize("h,kvh", [(4, 4), (8, 2), (6, 1)])
@pytest.mark.parametrize("d", [16, 64, 128])
@pytest.mark.parametrize("pos", [0, 7])
@pytest.mark.parametrize("s", [1, 5, 128])
def test_bits_of_rope_fwd_and_untouched_rows(s, pos, d, h, kvh, fused):
    q, k, v = inputs(s, d, h, kvh, fused)
    cos, sin = tables(pos, s, d)
    cap = pos + s + TAIL
    kc, vc = sentinel_cache(cap, kvh, d)
    kc0, vc0 = kc.clone(), vc.clone()
    qo = ext().kv_append(q, k, v, kc, vc, pos, cos, sin)
    q_ref, k_ref = ext().rope_fwd(q.contiguous(), k.contiguous(), cos, sin,
                                  False)
    assert qo.is_contiguous() and qo.shape == q.shape
    assert torch.equal(qo, q_ref)
    assert torch.equal(kc[:, pos:pos + s], k_ref)
    assert torch.equal(vc[:, pos:pos + s], v)
    assert untouched(kc, kc0, pos, s) and untouched(vc, vc0, pos, s)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "contig"])
@pytest.mark.parametrize("s,pos,d,h", [(1, 7, 64, 6), (5, 0, 128, 6),
                                        (128, 7, 16, 6)])
def test_without_tables_k_and_v_are_copied(s, pos, d, h, fused):
    kvh = 1
    q, k, v = inputs(s, d, h, kvh, fused, seed=1)
    cap = pos + s + TAIL
    kc, vc = sentinel_cache(cap, kvh, d)
    kc0, vc0 = kc.clone(), vc.clone()
    q0 = q.clone()
    qo = ext().kv_append(q, k, v, kc, vc, pos)
    assert qo.data_ptr() == q.data_ptr() and torch.equal(q, q0)
    assert torch.equal(kc[:, pos:pos + s], k)
    assert torch.equal(vc[:, pos:pos + s], v)
    assert untouched(kc, kc0, pos, s) and untouched(vc, vc0, pos, s)


def test_bad_arguments_raise_and_write_nothing():
    s, pos, d, h, kvh = 5, 7, 64, 8, 2
    q, k, v = inputs(s, d, h, kvh, True)
    cos, sin = tables(pos, s, d)
    cap = pos + s + TAIL
    kc, vc = sentinel_cache(cap, kvh, d)
    kc0, vc0 = kc.clone(), vc.clone()
    e = ext()
    # k with its base 8 bytes off the 16-byte grid
    raw = torch.zeros(k.numel() + 4, device=dev(), dtype=BF)
    off8 = raw[4:].view(B, s, kvh, d)
    assert off8.data_ptr() % 16 == 8
    bad = [
        lambda: e.kv_append(q, k, v, kc, vc, cap - s + 1, cos, sin),
        lambda: e.kv_append(q, k, v, kc, vc, -1, cos, sin),
        lambda: e.kv_append(q, k, v, kc, vc, pos, cos[:4], sin[:4]),
        lambda: e.kv_append(q, k, v, kc, vc, pos, cos, None),
        lambda: e.kv_append(q, k, v, kc.half(), vc.half(), pos, cos, sin),
        lambda: e.kv_append(q, k, v, kc[:, :, :, :32], vc[:, :, :, :32], pos,
                            cos, sin),
        lambda: e.kv_append(q, k, v[:, :, :1], kc, vc, pos, cos, sin),
        lambda: e.kv_append(q.transpose(1, 2), k, v, kc, vc, pos, cos, sin),
        lambda: e.kv_append(q, off8, v, kc, vc, pos, cos, sin),
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0)
    e.kv_append(q, k, v, kc, vc, pos, cos, sin)
    assert torch.equal(vc[:, pos:pos + s], v)


def test_ops_append_advances_len_and_matches_the_kernel():
    from fms_fsdp_amd import ops
    s, d, h, kvh = 5, 64, 8, 2
    cache = ops.KVCache(B, 9, kvh, d, BF, dev())
    with torch.no_grad():
        for pos, n in ((0, s), (s, 1)):
            q, k, v = inputs(n, d, h, kvh, True, seed=pos)
            cos, sin = tables(pos, n, d)
            qr = ops.kv_cache_append(cache, q, k, v, cos, sin)
            q_ref, k_ref = ext().rope_fwd(q.contiguous(), k.contiguous(), cos,
                                          sin, False)
            assert cache.len == pos + n
            assert torch.equal(qr, q_ref)
            assert torch.equal(cache.k[:, pos:pos + n], k_ref)
            assert torch.equal(cache.v[:, pos:pos + n], v)
