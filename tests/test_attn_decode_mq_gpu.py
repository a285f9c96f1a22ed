"""_C.attn_decode_mq (attn_decode_mq_kernel, attn_decode.hip) against float64
softmax attention with the causal mask aligned bottom right, computed in
torch on the GPU from the same bf16 q and cache contents.

q (b, s, h, d) holds the last s of the n cache rows; capacity = n + 37 and
the rows behind n are poisoned with NaN. s in {2, 5, 8, 33}, (h, kvh) in
{(4,4), (8,2), (16,1), (48,1)}: s*G = 2 is a near-empty column block, 32 an
exactly full one, 33 leaves one column in a second block, G = 48 splits a
query across blocks. n in {s+1, 33, 64, 65, 130, 300}, n > s: one cached
key, the window across a tile edge, more tiles than waves; s 33, n 64 has a
wave whose only tile is wholly masked for some columns of its block. d in
{64, 128} and b in {1, 3} follow the parity rule in `cases()`, so every s
and every head configuration meets both d and both b. Every case runs
splits 1 and, where the clamp (the tiles of n - s + 1 keys) allows, 2.

The rule is test_attn_decode_gpu.py's, the arithmetic being the same:
  o:   R = 2^-8, A = 2^-9 + A_REDUCE, mag = sum_j softmax_j |v_j| over the
       visible keys;
  lse: R = 0, A = A_REDUCE, mag = |lse| + max_j |score_j| over the visible
       keys;
and max-abs error over max-abs reference < 3e-2. NaN or inf fails."""

import functools
import math

import pytest
import torch

import oracle_rule as rule

pytestmark = pytest.mark.gpu

FWD_TOL = 3e-2
A_O = 2.0 ** -9 + rule.A_REDUCE
S_LIST = [2, 5, 8, 33]
HEADS = [(4, 4), (8, 2), (16, 1), (48, 1)]
PAD = 37
BF = torch.bfloat16


def cases():
    out = []
    for i, s in enumerate(S_LIST):
        for j, (h, kvh) in enumerate(HEADS):
            for n in sorted({s + 1, 33, 64, 65, 130, 300}):
                if n > s:
                    d = (64, 128)[(i + j) % 2]
                    b = (1, 3)[(i + j // 2 + j) % 2]
                    out.append((b, s, h, kvh, d, n))
    return out


CASES = cases()
for _k, _vals in ((1, S_LIST), (slice(2, 4), HEADS)):
    for _v in _vals:
        assert {c[4] for c in CASES if c[_k] == _v} == {64, 128}
        assert {c[0] for c in CASES if c[_k] == _v} == {1, 3}


def dev():
    return torch.device("cuda:0")


def ext():
    from fms_fsdp_amd import _C
    return _C


def make(b, s, h, kvh, d, n, seed=0, poison=float("nan")):
    g = torch.Generator(device="cpu").manual_seed(
        seed * 1000003 + n * 131 + h * 7 + s)
    q = torch.randn(b, s, h, d, generator=g).to(dev(), BF)
    kc = torch.randn(b, n + PAD, kvh, d, generator=g).to(dev(), BF)
    vc = torch.randn(b, n + PAD, kvh, d, generator=g).to(dev(), BF)
    kc[:, n:] = poison
    vc[:, n:] = poison
    return q, kc, vc


def oracle(q, kc, vc, n):
    """float64: (o, mag_o, lse, mag_lse) in the shapes the kernel returns."""
    b, s, h, d = q.shape
    G = h // kc.shape[2]
    k = kc[:, :n].double().repeat_interleave(G, dim=2)      # (b, n, h, d)
    v = vc[:, :n].double().repeat_interleave(G, dim=2)
    sc = torch.einsum("bihd,bjhd->bihj", q.double(), k) / math.sqrt(d)
    qi = torch.arange(s, device=q.device)[:, None, None]
    seen = torch.arange(n, device=q.device) <= n - s + qi   # (s, 1, n)
    sc = sc.masked_fill(~seen, float("-inf"))
    p = torch.softmax(sc, dim=-1)
    o = torch.einsum("bihj,bjhd->bihd", p, v)
    mag = torch.einsum("bihj,bjhd->bihd", p, v.abs())
    lse = torch.logsumexp(sc, dim=-1)
    smax = sc.masked_fill(~seen, 0.0).abs().amax(dim=-1)
    return o, mag, lse, lse.abs() + smax


@functools.lru_cache(maxsize=None)
def case_data(case):
    q, kc, vc = make(*case)
    return q, kc, vc, oracle(q, kc, vc, case[5])


def check(name, o, lse, ref):
    o_ref, o_mag, lse_ref, lse_mag = ref
    err = ((o.double() - o_ref).abs().max() / o_ref.abs().max()).item()
    print(f"[maxnorm] {name}: {err:.3g}")
    assert err < FWD_TOL, (name, err)
    rule.check(f"{name} o", o, o_ref, o_mag, A_O)
    rule.check(f"{name} lse", lse, lse_ref, lse_mag, rule.A_REDUCE, R=0.0)


@pytest.mark.parametrize("case", CASES,
                         ids=lambda c: "b%d_s%d_h%d_kvh%d_d%d_n%d" % c)
def test_matches_float64(case):
    b, s, h, kvh, d, n = case
    q, kc, vc, ref = case_data(case)
    for splits in (1, 2):
        if splits > (n - s) // 32 + 1:
            continue
        o, lse = ext().attn_decode_mq(q, kc, vc, n, splits)
        assert o.shape == q.shape and o.dtype == BF
        assert lse.shape == (b, s, h) and lse.dtype == torch.float32
        check(f"{case} splits{splits}", o, lse, ref)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("heads,s,n", [((8, 2), 5, 130), ((4, 4), 33, 65)])
def test_causality_and_poison_by_bits(heads, s, n, splits):
    b, (h, kvh), d = 3, heads, 128
    q, kc, vc = make(b, s, h, kvh, d, n)
    o, lse = ext().attn_decode_mq(q, kc, vc, n, splits)
    o2, lse2 = ext().attn_decode_mq(q, kc, vc, n, splits)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    check(f"bits s{s} n{n} splits{splits}", o, lse, oracle(q, kc, vc, n))
    # whatever lies behind kv_len is never seen
    for poison in (0.0, float("inf")):
        _, kp, vp = make(b, s, h, kvh, d, n, poison=poison)
        op, lsep = ext().attn_decode_mq(q, kp, vp, n, splits)
        assert torch.equal(op, o) and torch.equal(lsep, lse), poison
    # the newest cache row is seen by the last query alone
    kn, vn = kc.clone(), vc.clone()
    kn[:, n - 1] = -kn[:, n - 1] * 3
    vn[:, n - 1] = 7.0
    on, lsen = ext().attn_decode_mq(q, kn, vn, n, splits)
    assert not torch.equal(on[:, s - 1], o[:, s - 1])
    assert torch.equal(on[:, :s - 1], o[:, :s - 1])
    assert torch.equal(lsen[:, :s - 1], lse[:, :s - 1])
    # batch rows are isolated
    qb, kb, vb = q.clone(), kc.clone(), vc.clone()
    qb[0] = -qb[0] * 3
    kb[0, :n] = kb[0, :n].flip(0)
    vb[0, :n] = 7.0
    ob, lseb = ext().attn_decode_mq(qb, kb, vb, n, splits)
    assert not torch.equal(ob[0], o[0])
    assert torch.equal(ob[1:], o[1:]) and torch.equal(lseb[1:], lse[1:])


def filled_cache(kc, vc, n):
    from fms_fsdp_amd import ops
    b, cap, kvh, d = kc.shape
    cache = ops.KVCache(b, cap, kvh, d, BF, dev())
    cache.k.copy_(kc)
    cache.v.copy_(vc)
    cache.len = n
    return cache


def test_ops_attention_cached_routes():
    from fms_fsdp_amd import ops
    b, s, h, kvh, d, n0 = 3, 5, 8, 2, 128, 33
    _, kc, vc = make(b, s, h, kvh, d, n0)
    g = torch.Generator(device="cpu").manual_seed(5)
    q, k, v = (torch.randn(b, s, hh, d, generator=g).to(dev(), BF)
               for hh in (h, kvh, kvh))
    with torch.no_grad():
        # s > 1 on a non-empty cache: the multi-query kernel
        cache = filled_cache(kc, vc, n0)
        o = ops.attention_cached(q, k, v, cache)
        assert cache.len == n0 + s
        assert torch.equal(cache.k[:, n0:n0 + s], k)
        assert torch.equal(
            o, ext().attn_decode_mq(q, cache.k, cache.v, cache.len)[0])
        # fp16 bridges through bf16
        qh, kh, vh = q.half(), k.half(), v.half()
        oh = ops.attention_cached(qh, kh, vh, filled_cache(kc, vc, n0))
        want = ops.attention_cached(qh.bfloat16(), kh.bfloat16(),
                                    vh.bfloat16(), filled_cache(kc, vc, n0))
        assert oh.dtype == torch.float16 and torch.equal(oh, want.half())
        # s == 1: the decode kernel, as before
        o1 = ops.attention_cached(q[:, :1], k[:, :1], v[:, :1], cache)
        assert torch.equal(o1, ext().attn_decode(
            q[:, :1].contiguous(), cache.k, cache.v, cache.len)[0])
        # prefill into an empty cache: attention_causal, as before
        empty = ops.KVCache(b, n0, kvh, d, BF, dev())
        op = ops.attention_cached(q, k, v, empty)
        assert empty.len == s
        assert torch.equal(op, ops.attention_causal(q, k, v))


def test_bad_arguments_raise_and_launch_nothing():
    case = (3, 5, 8, 2, 64, 65)
    q, kc, vc, ref = case_data(case)
    n = case[5]
    cap = kc.shape[1]
    half = kc.half()
    mq = ext().attn_decode_mq
    bad = [
        ("s 0", lambda: mq(q[:, :0].contiguous(), kc, vc, n)),
        ("s > kv_len", lambda: mq(q, kc, vc, 4)),
        ("kv_len > capacity", lambda: mq(q, kc, vc, cap + 1)),
        ("d 32", lambda: mq(q[..., :32].contiguous(),
                            kc[..., :32].contiguous(),
                            vc[..., :32].contiguous(), n)),
        ("h % kvh", lambda: mq(q[:, :, :7].contiguous(), kc, vc, n)),
        ("G > 64", lambda: mq(
            torch.zeros(3, 5, 130, 64, device=dev(), dtype=BF), kc, vc, n)),
        ("fp16 cache", lambda: mq(q, half, half, n)),
        ("negative splits", lambda: mq(q, kc, vc, n, -1)),
    ]
    for name, call in bad:
        with pytest.raises(RuntimeError):
            call()
        o, lse = mq(q, kc, vc, n)
        check(f"after {name}", o, lse, ref)
