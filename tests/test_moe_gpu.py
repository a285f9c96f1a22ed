"""The routed MoE MLP kernels (ops/hip/moe.hip) against float64, stage by
stage under the rule of oracle_rule.py, and the Mixtral module under
ops.moe_mode("fused") against its own per-expert loop."""

import functools

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from test_mamba_decode_gpu import relerr
from test_ssd_kernels_gpu import ext, randn

pytestmark = pytest.mark.gpu

R_BF = 2.0 ** -8

# (emb, H, nE, k, T, BM). Expert 1 never gets a row. Between them: one
# token; a segment ending inside a tile; several row tiles per expert under
# both BM; two BK steps in gate_up (emb 128) and in down (H 128); two column
# tiles in gate_up (H 128 at BM 128, H 192 at BM 32) and in down (emb 192 at
# BM 128, emb 320 at BM 32), the last one partly past the matrix.
CASES = [(64, 128, 4, 2, 1, 32), (64, 128, 8, 1, 5, 32),
         (128, 64, 4, 2, 70, 32), (64, 128, 8, 2, 300, 32),
         (128, 64, 4, 1, 5, 128), (64, 128, 4, 2, 70, 128),
         (128, 64, 8, 2, 300, 128), (64, 128, 4, 2, 300, 128),
         (320, 192, 4, 2, 5, 32), (192, 64, 4, 2, 70, 128)]


@functools.lru_cache(maxsize=None)
def chain(emb, H, nE, k, T, BM):
    """Inputs and every stage's output of one case, computed once."""
    torch.manual_seed(emb + H + nE + k + T + BM)
    C = ext()
    c = dict(x=randn(T, emb), logits=randn(T, nE).float(),
             wg1=[randn(2 * H, emb, scale=emb ** -0.5) for _ in range(nE)],
             w2=[randn(emb, H, scale=H ** -0.5) for _ in range(nE)])
    c["logits"][:, 1] -= 30.0
    c["ids"], c["wts"] = C.moe_route(c["logits"], k)
    c["row_pair"], c["tile_expert"] = C.moe_sort(c["ids"], nE, BM)
    c["h"] = C.moe_gate_up(c["x"], c["row_pair"], c["tile_expert"], c["wg1"],
                           k, BM)
    c["ys"] = C.moe_down(c["h"], c["row_pair"], c["tile_expert"], c["wts"],
                         c["w2"], T, BM)
    c["out"] = C.moe_combine(c["ys"], k)
    c["pos"] = (c["row_pair"] >= 0).nonzero().flatten()   # real sorted rows
    c["pair"] = c["row_pair"][c["pos"]].long()
    return c


@pytest.mark.parametrize("case", CASES)
def test_route(case):
    emb, H, nE, k, T, BM = case
    logits = torch.cat([chain(*case)["logits"],
                        torch.full((1, nE), 0.25, device="cuda")])
    ids, wts = ext().moe_route(logits, k)
    ids, p = ids.long(), torch.softmax(logits.double(), -1)
    assert ids.shape == (T + 1, k) and int(ids.min()) >= 0 \
        and int(ids.max()) < nE
    chosen = p.gather(1, ids)
    rest = p.scatter(1, ids, -1.0)
    assert int((rest < 0).sum()) == (T + 1) * k, "an expert was chosen twice"
    assert bool((chosen.min(1).values >= rest.max(1).values).all())
    assert ids[T].tolist() == list(range(k))      # all equal: lowest first
    assert not bool((ids[:T] == 1).any())
    ref = chosen / chosen.sum(-1, keepdim=True)
    rule.check("moe wts", wts, ref, ref, rule.A_REDUCE, R=0.0)


@pytest.mark.parametrize("case", CASES)
def test_sort(case):
    emb, H, nE, k, T, BM = case
    c = chain(*case)
    rp, te = c["row_pair"], c["tile_expert"]
    assert rp.numel() == te.numel() * BM
    assert c["pair"].sort().values.tolist() == list(range(T * k))
    expert = c["ids"].flatten().long()[c["pair"]]
    assert torch.equal(te.long()[c["pos"] // BM], expert)
    key = expert * (T * k) + c["pair"]       # expert order, then pair order
    assert bool((key[1:] > key[:-1]).all())
    used = torch.zeros_like(te, dtype=torch.bool)
    used[c["pos"] // BM] = True
    assert torch.equal(te >= 0, used)
    assert int(te.min()) >= -1 and int(rp.min()) >= -1
    again = ext().moe_sort(c["ids"], nE, BM)
    assert torch.equal(again[0], rp) and torch.equal(again[1], te)


@pytest.mark.parametrize("case", CASES)
def test_gate_up(case):
    emb, H, nE, k, T, BM = case
    c = chain(*case)
    xs = c["x"].double()[c["pair"] // k]
    w = torch.stack(c["wg1"]).double()[c["ids"].flatten().long()[c["pair"]]]
    gu = torch.einsum("pe,pne->pn", xs, w)
    mg, mu = torch.einsum("pe,pne->pn", xs.abs(), w.abs()).chunk(2, -1)
    g, u = gu.chunk(2, -1)
    sg = g * torch.sigmoid(g)
    ref = sg * u
    mag = ref.abs() + 1.1 * u.abs() * mg + sg.abs() * mu
    rule.check("moe h", c["h"][c["pos"]], ref, mag, rule.A_REDUCE, R=R_BF)


@pytest.mark.parametrize("case", CASES)
def test_down_combine(case):
    emb, H, nE, k, T, BM = case
    c = chain(*case)
    C = ext()
    inv = torch.empty_like(c["pair"])
    inv[c["pair"]] = c["pos"]                # pair -> sorted row
    hp = c["h"][inv].double().view(T, k, H)
    w = torch.stack(c["w2"]).double()[c["ids"].long()]      # (T, k, emb, H)
    wts = c["wts"].double()[..., None]
    ref = (wts * torch.einsum("tkh,tkmh->tkm", hp, w)).sum(1)
    mag = (wts * torch.einsum("tkh,tkmh->tkm", hp.abs(), w.abs())).sum(1)
    rule.check("moe out", c["out"], ref, mag, rule.A_REDUCE, R=R_BF)
    ys = C.moe_down(c["h"], c["row_pair"], c["tile_expert"], c["wts"],
                    c["w2"], T, BM)
    assert torch.equal(C.moe_combine(ys, k), c["out"])


def test_module():
    from fms_fsdp_amd.config import get_model_config
    from fms_fsdp_amd.models.mixtral import Mixtral
    C = ext()
    torch.manual_seed(0)
    cfg = get_model_config("mixtral_test")
    with torch.device("cuda"):
        m = Mixtral(cfg)
        m.reset_parameters()
    m = m.bfloat16().requires_grad_(False)
    tok = torch.randint(0, cfg.src_vocab_size, (2, 128), device="cuda")
    prev = ops.moe_mode()
    try:
        with torch.no_grad():
            ops.moe_mode("loop")
            n0 = C.moe_calls()
            want = m(tok)
            _, emb_l = m.generate(tok[:, :16], 4, do_sample=False,
                                  include_embeds=True)
            assert C.moe_calls() == n0
            ops.moe_mode("fused")
            got = m(tok)
            assert C.moe_calls() == n0 + cfg.nlayers
            _, emb_f = m.generate(tok[:, :16], 4, do_sample=False,
                                  include_embeds=True)
            assert C.moe_calls() == n0 + 5 * cfg.nlayers
        assert relerr(got, want) < 2e-2
        assert relerr(emb_f[:, 0], emb_l[:, 0]) < 2e-2
        m.requires_grad_(True)      # training keeps the loop
        m(tok)
        assert C.moe_calls() == n0 + 5 * cfg.nlayers
    finally:
        ops.moe_mode(prev)


@pytest.mark.parametrize("bad", ["H", "top_k", "dtype", "stride"])
def test_binding_checks(bad):
    emb, nE = 64, 8
    H = 96 if bad == "H" else 128
    x = randn(5, emb, dtype=torch.float32 if bad == "dtype" else torch.bfloat16)
    wg1 = [randn(2 * H, emb) for _ in range(nE)]
    w2 = [randn(emb, H) for _ in range(nE)]
    if bad == "stride":
        wg1[3] = randn(2 * H, 2 * emb)[:, :emb]
    n0 = ext().moe_calls()
    with pytest.raises(RuntimeError):
        ext().moe_mlp(x, randn(5, nE).float(), wg1, w2,
                      5 if bad == "top_k" else 2)
    assert ext().moe_calls() == n0
