"""The LayerNorm + embedding add + GELU kernels (ops/hip/layernorm.hip)
against reference.layernorm_act in float64 under the rule of oracle_rule.py,
the MLPSpeculator under ops.speculator_mode("fused") against its own torch
chain, and the bindings' argument checks."""

import math

import pytest
import torch

import oracle_rule as rule
from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_mamba_decode_gpu import relerr
from test_ssd_kernels_gpu import ext, randn

pytestmark = pytest.mark.gpu

EPS = 1e-6
SX = 0.5 ** (0.5 / 3)           # the speculator's mixing weights, 3 heads
SE = math.sqrt(1 - SX ** 2)

# (T, H, V, has_emb, gelu, out_scale, row_offset): the smallest shape (255
# masked threads); two grid-stride trips, a partial last chunk group (33
# chunks) and every token about 300 times; NC = 2 with a row mean of 8 std;
# NC = 4; the ln_input instantiation at NC = 2 with a partial chunk.
CASES = [(5, 8, 50, True, True, 1.0, 0.0),
         (2051, 264, 7, True, True, 1.0, 0.0),
         (67, 4096, 50, True, True, 1.0, 8.0),
         (37, 8192, 50, True, True, 1.0, 0.0),
         (37, 2056, 0, False, False, 1 / math.sqrt(2), 8.0)]


@pytest.mark.parametrize("T,H,V,has_emb,gelu,out_scale,offset", CASES)
def test_kernels_against_float64(T, H, V, has_emb, gelu, out_scale, offset):
    torch.manual_seed(T + H)
    C = ext()
    x = (randn(T, H, dtype=torch.float32) + offset).bfloat16()
    w = (1 + randn(H, dtype=torch.float32, scale=0.3)).bfloat16()
    b, dy = randn(H, scale=0.3), randn(T, H)
    emb = tok = None
    sx, se = 1.0, 0.0
    if has_emb:
        emb, sx, se = randn(V, H), SX, SE
        tok = torch.randint(0, V, (T,), device="cuda")
    y, mean, rstd = C.ln_act_fwd(x, emb, tok, w, b, sx, se, EPS, gelu,
                                 out_scale)
    grads = C.ln_act_bwd(dy, x, emb, tok, w, b, mean, rstd, sx, se, gelu,
                         out_scale)
    dx, dz, dw, db = grads

    # oracle: the gathered rows stand in for emb, so autograd yields dz
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    z64 = (emb.double()[tok] if has_emb
           else torch.zeros_like(x64)).requires_grad_()
    ref = reference.layernorm_act(x64, w64, b64, EPS, z64,
                                  torch.arange(T, device="cuda"), sx, se,
                                  gelu, out_scale)
    ref.backward(dy.double())
    with torch.no_grad():
        v = x64 * sx + z64 * se
        mag_v = (x64 * sx).abs() + (z64 * se).abs()
        mu = v.mean(-1, keepdim=True)
        r = torch.rsqrt((v - mu).square().mean(-1, keepdim=True) + EPS)
        nh = (v - mu) * r
        n = nh * w64 + b64
        mag_n = (mag_v + mag_v.mean(-1, keepdim=True)) * r * w64.abs() \
            + b64.abs()
        gn = dy.double() * out_scale
        mag_y, mag_gn = out_scale * mag_n, gn.abs()
        if gelu:
            gn = gn * (0.5 * (1 + torch.erf(n / math.sqrt(2)))
                       + n * torch.exp(-0.5 * n * n) / math.sqrt(2 * math.pi))
            mag_y = ref.abs() + 1.13 * out_scale * mag_n
            mag_gn = gn.abs() + 0.8 * dy.double().abs() * out_scale * mag_n
        mag_a = mag_gn * w64.abs()
        mag_dv = r * (mag_a + mag_a.mean(-1, keepdim=True) + nh.abs()
                      * (mag_a * nh.abs()).mean(-1, keepdim=True))
    A = rule.A_REDUCE
    rule.check("ln y", y, ref, mag_y, A)
    rule.check("ln mean", mean, mu[:, 0], mag_v.mean(-1), A)
    rule.check("ln rstd", rstd, r[:, 0], r[:, 0], A)
    rule.check("ln dx", dx, x64.grad, sx * mag_dv, A)
    if has_emb:
        rule.check("ln dz", dz, z64.grad, se * mag_dv, A)
    else:
        assert dz is None
    rule.check("ln dw", dw, w64.grad, (mag_gn * nh.abs()).sum(0), A)
    rule.check("ln db", db, b64.grad, mag_gn.sum(0), A)

    assert torch.equal(C.ln_act_fwd(x, emb, tok, w, b, sx, se, EPS, gelu,
                                    out_scale)[0], y)
    again = C.ln_act_bwd(dy, x, emb, tok, w, b, mean, rstd, sx, se, gelu,
                         out_scale)
    assert all(torch.equal(g, a) for g, a in zip(grads, again)
               if g is not None)


def test_speculator_fused_matches_torch():
    from fms_fsdp_amd.models.speculator import MLPSpeculator
    C = ext()
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = MLPSpeculator(256, 128, 512, 3)
    m.reset_parameters()
    m = m.bfloat16()
    state = randn(2, 16, 256)
    inds = torch.randint(0, 512, (2, 16 + 2), device="cuda")
    logits = {}
    prev = ops.speculator_mode()
    try:
        for mode, calls in (("torch", 0), ("fused", m.n_predict + 1)):
            ops.speculator_mode(mode)
            m.zero_grad()
            n0 = C.ln_act_calls()
            logits[mode] = m(state, inds)
            assert C.ln_act_calls() == n0 + calls
            logits[mode].float().square().mean().backward()
            for name, p in m.named_parameters():
                assert p.grad is not None and \
                    bool(torch.isfinite(p.grad).all()), (mode, name)
    finally:
        ops.speculator_mode(prev)
    assert relerr(logits["fused"], logits["torch"]) < 2e-2


@pytest.mark.parametrize("bad", ["H12", "H8200", "fp32", "emb_no_tok",
                                 "emb_width", "stride"])
def test_binding_checks(bad):
    H = {"H12": 12, "H8200": 8200}.get(bad, 64)
    x = randn(5, H, dtype=torch.float32 if bad == "fp32" else torch.bfloat16)
    if bad == "stride":
        x = randn(5, 2 * H)[:, :H]
    emb = randn(7, H + 8 if bad == "emb_width" else H)
    tok = None if bad == "emb_no_tok" else \
        torch.randint(0, 7, (5,), device="cuda")
    n0 = ext().ln_act_calls()
    with pytest.raises(RuntimeError):
        ext().ln_act_fwd(x, emb, tok, randn(H), randn(H), SX, SE, EPS, True,
                         1.0)
    assert ext().ln_act_calls() == n0
