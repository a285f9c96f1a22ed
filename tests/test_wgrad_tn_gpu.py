"""`_C.wgrad_tn`: the weight grad dW = dy^T @ x computed from operands
transposed by transpose.hip, overwriting or accumulating into a grad view,
and its routing in `ops.linear_flat`.

Every result is held to the rule of tests/oracle_rule.py against float64:
ref from the bf16 inputs (for the accumulate call also from the bf16
contents of the view before it), mag = sum |dy||x| (+ |c|), A = A_REDUCE
(an fp32 reduction over the tokens), R = one bf16 rounding. The old
addmm route is held to the same rule, which shows the inputs are inside
it for the reference alone.

Shapes (tokens, out, in): 256 x 192 x 128, and tokens 200, which leaves a
partial 64-row tile in both transposes."""

import pytest
import torch

import oracle_rule as rule

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [(256, 192, 128), (200, 192, 128)]
MODES = [1, 2, 3]         # dy transposed (NN), x transposed (TT), both (TN)


def ext():
    from fms_fsdp_amd import _C
    return _C


_CASES = {}


def case(tokens, out, inn):
    """Inputs and float64 references of one shape: computed once, shared,
    never modified."""
    key = (tokens, out, inn)
    if key not in _CASES:
        torch.manual_seed(tokens)
        dy = torch.randn(tokens, out, device="cuda:0").to(BF)
        x = torch.randn(tokens, inn, device="cuda:0").to(BF)
        ref = dy.double().t() @ x.double()
        mag = dy.double().abs().t() @ x.double().abs()
        _CASES[key] = dict(dy=dy, x=x, ref=ref, mag=mag)
    return _CASES[key]


def old_route(dy, x, gview, accumulate):
    if accumulate:
        gview.addmm_(dy.t(), x)
    else:
        torch.addmm(gview, dy.t(), x, beta=0, out=gview)


def check_route(name, run, c):
    gview = torch.full_like(c["ref"], float("nan"), dtype=BF)
    run(c["dy"], c["x"], gview, False)
    assert torch.isfinite(gview).all(), f"{name}: beta=0 read the old gview"
    rule.check(f"{name} overwrite", gview, c["ref"], c["mag"], rule.A_REDUCE)
    first = gview.clone()
    run(c["dy"], c["x"], gview, True)
    rule.check(f"{name} accumulate", gview, c["ref"] + first.double(),
               c["mag"] + first.double().abs(), rule.A_REDUCE)


@pytest.mark.parametrize("tokens,out,inn", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_wgrad_tn(tokens, out, inn, mode):
    check_route(f"wgrad_tn mode {mode} {tokens}x{out}x{inn}",
                lambda dy, x, g, acc: ext().wgrad_tn(dy, x, g, acc, mode),
                case(tokens, out, inn))


@pytest.mark.parametrize("tokens,out,inn", SHAPES)
def test_old_route_same_rule(tokens, out, inn):
    check_route(f"addmm {tokens}x{out}x{inn}", old_route,
                case(tokens, out, inn))


def test_wgrad_tn_strided_operand():
    """dy as a column slice of a wider buffer: read in place."""
    c = case(256, 192, 128)
    wide = torch.zeros(256, 192 + 64, device="cuda:0", dtype=BF)
    wide[:, 32:32 + 192] = c["dy"]
    dy = wide[:, 32:32 + 192]
    gview = torch.full_like(c["ref"], float("nan"), dtype=BF)
    ext().wgrad_tn(dy, c["x"], gview, False, 3)
    rule.check("wgrad_tn strided dy", gview, c["ref"], c["mag"],
               rule.A_REDUCE)


def test_wgrad_tn_rejects():
    c = case(256, 192, 128)
    g = torch.zeros(192, 128, device="cuda:0", dtype=BF)
    with pytest.raises(RuntimeError):
        ext().wgrad_tn(c["dy"], c["x"], g, False, 0)
    with pytest.raises(RuntimeError):
        ext().wgrad_tn(c["dy"], c["x"], g.t(), False, 3)
    with pytest.raises(RuntimeError):
        ext().wgrad_tn(c["dy"][:-8], c["x"], g, False, 3)


# --------------------------------------------------------------------------
# routing through ops.linear_flat with a fake flat grad view
# --------------------------------------------------------------------------
def run_linear_flat(tokens, out, inn, with_residual):
    from fms_fsdp_amd import ops
    torch.manual_seed(7)
    dev = "cuda:0"
    w = (torch.randn(out, inn, device=dev) * 0.02).to(BF).requires_grad_()
    w._flat_grad_view = torch.full((out, inn), float("nan"), device=dev,
                                   dtype=BF)
    w._wgrad_fresh = True
    fired = []
    w._wgrad_done = lambda: fired.append(1)
    x = torch.randn(2, tokens // 2, inn, device=dev).to(BF).requires_grad_()
    res = (torch.randn(2, tokens // 2, out, device=dev).to(BF)
           .requires_grad_() if with_residual else None)
    dy = torch.randn(2, tokens // 2, out, device=dev).to(BF)
    before = ext().wgrad_tn_calls()
    ops.linear_flat(x, w, res).backward(dy)
    return dict(x=x, dy=dy, dx=x.grad,
                dres=None if res is None else res.grad,
                gview=w._flat_grad_view, fired=len(fired),
                fresh=w._wgrad_fresh, wgrad=w.grad,
                tn_calls=ext().wgrad_tn_calls() - before)


def smallest_routed_shape():
    from fms_fsdp_amd import ops
    tokens = ops._WGRAD_TN_MIN_TOKENS
    inn = 4096
    out = -(-ops._WGRAD_TN_MIN_WEIGHT // inn)
    return tokens, out, inn


def test_linear_flat_routes_and_matches_old(monkeypatch):
    tokens, out, inn = smallest_routed_shape()
    monkeypatch.delenv("FMS_AMD_WGRAD", raising=False)
    new = run_linear_flat(tokens, out, inn, True)
    monkeypatch.setenv("FMS_AMD_WGRAD", "nt")
    old = run_linear_flat(tokens, out, inn, True)
    assert new["tn_calls"] == 1 and old["tn_calls"] == 0
    for r in (new, old):
        assert r["fired"] == 1 and r["fresh"] is False and r["wgrad"] is None
        assert torch.isfinite(r["gview"]).all()
    assert torch.equal(new["dx"], old["dx"])
    assert torch.equal(new["dres"], old["dres"])
    # the wgrad itself: same inputs (same seed), the float64 rule
    dy64 = new["dy"].double().view(tokens, out)
    x64 = new["x"].detach().double().view(tokens, inn)
    ref, mag = dy64.t() @ x64, dy64.abs().t() @ x64.abs()
    rule.check("linear_flat routed wgrad", new["gview"], ref, mag,
               rule.A_REDUCE)
    rule.check("linear_flat nt wgrad", old["gview"], ref, mag, rule.A_REDUCE)


def test_routing_rule(monkeypatch):
    """The measured rule on the 7B block's own shapes: (tokens, out, in)
    -> mode."""
    from fms_fsdp_amd import ops
    monkeypatch.delenv("FMS_AMD_WGRAD", raising=False)

    def mode(tokens, out, inn, dtype=BF):
        dy = torch.empty(tokens, out, device="cuda:0", dtype=dtype)
        x = torch.empty(tokens, inn, device="cuda:0", dtype=dtype)
        return ops._wgrad_mode(dy, x)

    assert mode(8192, 12288, 4096) == 3       # qkv
    assert mode(8192, 22016, 4096) == 3       # gate|up
    assert mode(8192, 4096, 11008) == 3       # down
    assert mode(8192, 4096, 4096) == 0        # proj: square, loses
    assert mode(4096, 22016, 4096) == 0       # below the token crossover
    assert mode(8192, 12288, 4096, torch.float32) == 0
    assert mode(8192, 12292, 4096) == 0       # out % 8
    wide = torch.empty(8192, 12288 + 8, device="cuda:0", dtype=BF)
    x = torch.empty(8192, 4096, device="cuda:0", dtype=BF)
    assert ops._wgrad_mode(wide[:, 8:], x) == 3      # row-strided: in place
    assert ops._wgrad_mode(wide[:, 4:-4], x) == 0    # 8-byte aligned only
    monkeypatch.setenv("FMS_AMD_WGRAD", "nt")
    assert mode(8192, 12288, 4096) == 0


def test_linear_flat_excluded_shape_takes_old_route(monkeypatch):
    monkeypatch.delenv("FMS_AMD_WGRAD", raising=False)
    r = run_linear_flat(256, 192, 128, False)
    assert r["tn_calls"] == 0
    assert r["fired"] == 1 and r["fresh"] is False
    assert torch.isfinite(r["gview"]).all()
