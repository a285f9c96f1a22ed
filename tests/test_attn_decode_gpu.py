"""_C.attn_decode (attn_decode.hip) against float64 softmax attention
computed in torch, on the GPU, from the same bf16 q and cache contents.

Shapes. kv_len in {1, 31, 32, 33, 64, 65, 127, 129, 300} (around the 32-key
tile and the 4-wave round: one tile, a full tile, a tile plus one key, more
tiles than waves), (h, kvh) in {(4,4), (8,2), (8,1), (16,1), (48,1)}
(G = 1, 4, 8, 16 and 48, the last one crossing the 32-column block),
d in {64, 128}, b in {1, 3}; capacity = kv_len + 37, so the batch stride is
not kv_len*kvh*d. The covering subset: EVERY (kv_len, heads) pair once,
with d and b assigned by the parity rule in `cases()` so that every kv_len
and every head configuration meets both d and both b (asserted below).

The elementwise rule (tests/oracle_rule.py): |got - ref| <= R|ref| + A*mag.
  o:   R = 2^-8 (the one bf16 rounding of the output),
       mag = sum_j softmax_j |v_j|,
       A = 2^-9 + A_REDUCE. The kernel rounds P to bf16 for the PV mfma
       (relative 2^-9 per term of the numerator) and sums l from the fp32
       P, so the denominator carries no bf16 rounding: 2^-9 * mag. The rest
       of the chain is fp32 (mfma accumulation of the scores, exp2, the
       rescales, the wave merge and the split combine): A_REDUCE, the
       rule's figure for an fp32 reduction. scale*log2e is applied in fp32
       after the mfma, q is never rounded again.
  lse: R = 0, A = A_REDUCE, mag = |lse| + max_j |score_j|.
NaN or inf anywhere fails (worst_ratio returns inf for them)."""

import functools
import math

import pytest
import torch

import oracle_rule as rule

pytestmark = pytest.mark.gpu

FWD_TOL = 3e-2
A_O = 2.0 ** -9 + rule.A_REDUCE

KV_LENS = [1, 31, 32, 33, 64, 65, 127, 129, 300]
HEADS = [(4, 4), (8, 2), (8, 1), (16, 1), (48, 1)]
PAD = 37
BF = torch.bfloat16


def cases():
    out = []
    for i, n in enumerate(KV_LENS):
        for j, (h, kvh) in enumerate(HEADS):
            d = (64, 128)[(i + j) % 2]
            b = (1, 3)[(i + j // 2 + j) % 2]
            out.append((b, h, kvh, d, n))
    return out


CASES = cases()
for _n in KV_LENS:
    assert {c[3] for c in CASES if c[4] == _n} == {64, 128}
    assert {c[0] for c in CASES if c[4] == _n} == {1, 3}
for _h, _kvh in HEADS:
    assert {c[3] for c in CASES if c[1:3] == (_h, _kvh)} == {64, 128}
    assert {c[0] for c in CASES if c[1:3] == (_h, _kvh)} == {1, 3}


def dev():
    return torch.device("cuda:0")


def ext():
    from fms_fsdp_amd import _C
    return _C


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def make(b, h, kvh, d, n, seed=0, poison=0.0):
    """bf16 q (b,1,h,d) and a cache pair of capacity n + PAD whose rows
    behind n hold `poison`."""
    g = torch.Generator(device="cpu").manual_seed(seed * 1000003 + n * 131 + h)
    q = torch.randn(b, 1, h, d, generator=g).to(dev(), BF)
    kc = torch.randn(b, n + PAD, kvh, d, generator=g).to(dev(), BF)
    vc = torch.randn(b, n + PAD, kvh, d, generator=g).to(dev(), BF)
    kc[:, n:] = poison
    vc[:, n:] = poison
    return q, kc, vc


def oracle(q, kc, vc, n):
    """float64: (o, mag_o, lse, mag_lse) in the shapes the kernel returns."""
    b, _, h, d = q.shape
    G = h // kc.shape[2]
    k = kc[:, :n].double().repeat_interleave(G, dim=2)      # (b, n, h, d)
    v = vc[:, :n].double().repeat_interleave(G, dim=2)
    s = torch.einsum("bhd,bjhd->bhj", q[:, 0].double(), k) / math.sqrt(d)
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bhj,bjhd->bhd", p, v)
    mag = torch.einsum("bhj,bjhd->bhd", p, v.abs())
    lse = torch.logsumexp(s, dim=-1)
    return (o.unsqueeze(1), mag.unsqueeze(1), lse,
            lse.abs() + s.abs().amax(dim=-1))


@functools.lru_cache(maxsize=None)
def case_data(case):
    q, kc, vc = make(*case)
    return q, kc, vc, oracle(q, kc, vc, case[4])


def check(name, o, lse, ref):
    o_ref, o_mag, lse_ref, lse_mag = ref
    err = relerr(o, o_ref)
    print(f"[maxnorm] {name}: {err:.3g}")
    assert err < FWD_TOL, (name, err)
    rule.check(f"{name} o", o, o_ref, o_mag, A_O)
    rule.check(f"{name} lse", lse, lse_ref, lse_mag, rule.A_REDUCE, R=0.0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d_h%d_kvh%d_d%d_n%d" % c)
def test_matches_float64(case):
    q, kc, vc, ref = case_data(case)
    o, lse = ext().attn_decode(q, kc, vc, case[4])
    assert o.shape == q.shape and o.dtype == BF
    assert lse.shape == (case[0], case[1]) and lse.dtype == torch.float32
    check(str(case), o, lse, ref)


@pytest.mark.parametrize("n", [1, 33, 129])
@pytest.mark.parametrize("splits", [1, 2])
def test_rows_behind_kv_len_are_never_seen(n, splits):
    """Zeros, NaN and +inf behind kv_len give the same bits."""
    b, h, kvh, d = 3, 8, 2, 128
    outs = []
    for poison in (0.0, float("nan"), float("inf")):
        q, kc, vc = make(b, h, kvh, d, n, poison=poison)
        o, lse = ext().attn_decode(q, kc, vc, n, splits)
        assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
        outs.append((o, lse))
    for o, lse in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1])
    check(f"poison n{n} s{splits}", *outs[2],
          oracle(*make(b, h, kvh, d, n), n))


@pytest.mark.parametrize("heads,d", [((8, 2), 128), ((48, 1), 64)])
def test_splits(heads, d):
    n, b = 300, 3                    # 10 key tiles
    case = (b, *heads, d, n)
    q, kc, vc, ref = case_data(case)
    got = {}
    for splits in (1, 2, 3, 10, 64):
        o, lse = ext().attn_decode(q, kc, vc, n, splits)
        o2, lse2 = ext().attn_decode(q, kc, vc, n, splits)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), splits
        check(f"{case} splits{splits}", o, lse, ref)
        got[splits] = (o, lse)
    # a request above the tile count runs as the tile count
    assert torch.equal(got[64][0], got[10][0])
    assert torch.equal(got[64][1], got[10][1])
    # the planned call is one of the counts above at this size
    o, lse = ext().attn_decode(q, kc, vc, n)
    check(f"{case} planned", o, lse, ref)


@pytest.mark.parametrize("splits", [1, 3])
def test_batch_rows_are_isolated(splits):
    b, h, kvh, d, n = 3, 8, 2, 64, 129
    q, kc, vc = make(b, h, kvh, d, n)
    o, lse = ext().attn_decode(q, kc, vc, n, splits)
    q2, kc2, vc2 = q.clone(), kc.clone(), vc.clone()
    q2[0] = -q2[0] * 3
    kc2[0] = kc2[0].flip(0)
    vc2[0] = 7.0
    o2, lse2 = ext().attn_decode(q2, kc2, vc2, n, splits)
    assert not torch.equal(o[0], o2[0])
    assert torch.equal(o[1:], o2[1:]) and torch.equal(lse[1:], lse2[1:])


def test_bad_arguments_raise_and_launch_nothing():
    case = (3, 8, 2, 64, 65)
    q, kc, vc, ref = case_data(case)
    n = case[4]
    cap = kc.shape[1]
    half = kc.half()
    wide = torch.randn(3, cap, 2, 128, device=dev()).to(BF)
    bad = [
        ("kv_len 0", lambda: ext().attn_decode(q, kc, vc, 0)),
        ("kv_len > capacity", lambda: ext().attn_decode(q, kc, vc, cap + 1)),
        ("d 32", lambda: ext().attn_decode(q[..., :32].contiguous(),
                                           kc[..., :32].contiguous(),
                                           vc[..., :32].contiguous(), n)),
        ("h % kvh", lambda: ext().attn_decode(q[:, :, :7].contiguous(), kc,
                                              vc, n)),
        ("fp16 cache", lambda: ext().attn_decode(q, half, half, n)),
        ("strided cache", lambda: ext().attn_decode(q, wide[..., :64],
                                                    wide[..., 64:], n)),
        ("G > 64", lambda: ext().attn_decode(
            torch.zeros(3, 1, 130, 64, device=dev(), dtype=BF), kc, vc, n)),
        ("two queries", lambda: ext().attn_decode(
            torch.cat([q, q], dim=1), kc, vc, n)),
        ("negative splits", lambda: ext().attn_decode(q, kc, vc, n, -1)),
    ]
    for name, call in bad:
        with pytest.raises(RuntimeError):
            call()
        o, lse = ext().attn_decode(q, kc, vc, n)
        check(f"after {name}", o, lse, ref)


def test_ops_attention_decode_uses_the_kernel():
    from fms_fsdp_amd import ops
    b, h, kvh, d, n = 3, 8, 2, 128, 33
    q, kc, vc = make(b, h, kvh, d, n)
    cache = ops.KVCache(b, n + PAD, kvh, d, BF, dev())
    cache.k.copy_(kc)
    cache.v.copy_(vc)
    cache.len = n
    with torch.no_grad():
        o = ops.attention_decode(q, cache)
        assert torch.equal(o, ext().attn_decode(q, kc, vc, n)[0])
        # fp16 bridges through bf16 over the same cache
        oh = ops.attention_decode(q.half(), cache)
        want = ops.attention_decode(q.half().bfloat16(), cache).half()
    assert oh.dtype == torch.float16 and torch.equal(oh, want)
