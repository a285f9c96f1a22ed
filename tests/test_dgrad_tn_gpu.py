"""`_C.dgrad_tn`: the input grad dx = dy @ W computed as dy @ WT^T from a
weight transposed by transpose.hip right before the GEMM, and its routing
in `ops.linear_flat`.

Every result is held to the rule of tests/oracle_rule.py against float64:
ref = dy.double() @ w.double() from the bf16 inputs, mag = |dy| @ |w|,
A = A_REDUCE (an fp32 reduction over `out`), R = one bf16 rounding. The old
route `dy @ w` is held to the same rule, which shows the inputs are inside
it for the reference alone.

Shapes (tokens, out, in): 256 x 192 x 128, and 200 x 200 x 136, which
leaves a partial 64-tile in both directions of the weight transpose and a
token count that is no tile multiple."""

import pytest
import torch

import oracle_rule as rule

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
SHAPES = [(256, 192, 128), (200, 200, 136)]


def ext():
    from fms_fsdp_amd import _C
    return _C


_CASES = {}


def case(tokens, out, inn):
    """Inputs and float64 references of one shape: computed once, shared,
    never modified."""
    key = (tokens, out, inn)
    if key not in _CASES:
        torch.manual_seed(tokens + out)
        dy = torch.randn(tokens, out, device=DEV).to(BF)
        w = (torch.randn(out, inn, device=DEV) * 0.05).to(BF)
        ref = dy.double() @ w.double()
        mag = dy.double().abs() @ w.double().abs()
        _CASES[key] = dict(dy=dy, w=w, ref=ref, mag=mag)
    return _CASES[key]


@pytest.mark.parametrize("tokens,out,inn", SHAPES)
def test_dgrad_tn(tokens, out, inn):
    c = case(tokens, out, inn)
    dx = ext().dgrad_tn(c["dy"], c["w"])
    assert dx.shape == (tokens, inn) and dx.dtype == BF
    assert dx.is_contiguous()
    rule.check(f"dgrad_tn {tokens}x{out}x{inn}", dx, c["ref"], c["mag"],
               rule.A_REDUCE)


@pytest.mark.parametrize("tokens,out,inn", SHAPES)
def test_old_route_same_rule(tokens, out, inn):
    c = case(tokens, out, inn)
    rule.check(f"dy @ w {tokens}x{out}x{inn}", c["dy"] @ c["w"], c["ref"],
               c["mag"], rule.A_REDUCE)


def test_dgrad_tn_dy_column_slice():
    """dy as a column slice of a wider buffer (a slice of the fused dqkv):
    read in place."""
    c = case(256, 192, 128)
    wide = torch.full((256, 192 + 64), float("nan"), device=DEV, dtype=BF)
    wide[:, 32:32 + 192] = c["dy"]
    dy = wide[:, 32:32 + 192]
    assert not dy.is_contiguous()
    rule.check("dgrad_tn strided dy", ext().dgrad_tn(dy, c["w"]), c["ref"],
               c["mag"], rule.A_REDUCE)


def test_dgrad_tn_weight_in_flat_buffer():
    """w as a 128-element-aligned slice of a flat 1-D buffer, the way
    FlatUnit hands the weights out."""
    c = case(200, 200, 136)
    n = 200 * 136
    flat = torch.full((128 * 3 + n + 128,), float("nan"), device=DEV,
                      dtype=BF)
    w = flat[128 * 3:128 * 3 + n].view(200, 136)
    w.copy_(c["w"])
    rule.check("dgrad_tn flat-buffer w", ext().dgrad_tn(c["dy"], w),
               c["ref"], c["mag"], rule.A_REDUCE)


def test_dgrad_tn_rejects():
    c = case(256, 192, 128)
    dy, w = c["dy"], c["w"]
    with pytest.raises(RuntimeError):       # out % 8
        ext().dgrad_tn(dy[:, :188], w[:188])
    with pytest.raises(RuntimeError):       # a transposed view of a weight
        ext().dgrad_tn(dy[:, :128], w.t())
    with pytest.raises(RuntimeError):       # fp32
        ext().dgrad_tn(dy.float(), w.float())
    with pytest.raises(RuntimeError):
        ext().dgrad_tn(dy, w.float())
    with pytest.raises(RuntimeError):       # inner sizes differ
        ext().dgrad_tn(dy[:, :184], w)
    with pytest.raises(RuntimeError):       # dy with a column stride
        ext().dgrad_tn(torch.empty(192, 256, device=DEV, dtype=BF).t(), w)


def test_dgrad_tn_deterministic():
    c = case(200, 200, 136)
    outs = [ext().dgrad_tn(c["dy"], c["w"]) for _ in range(4)]
    assert all(torch.equal(outs[0], o) for o in outs[1:])


# --------------------------------------------------------------------------
# routing through ops.linear_flat with a fake flat grad view
# --------------------------------------------------------------------------
def run_linear_flat(tokens, out, inn, with_residual=True, x_grad=True):
    from fms_fsdp_amd import ops
    torch.manual_seed(7)
    w = (torch.randn(out, inn, device=DEV) * 0.02).to(BF).requires_grad_()
    w._flat_grad_view = torch.full((out, inn), float("nan"), device=DEV,
                                   dtype=BF)
    w._wgrad_fresh = True
    fired = []
    w._wgrad_done = lambda: fired.append(1)
    x = torch.randn(2, tokens // 2, inn, device=DEV).to(BF)
    x.requires_grad_(x_grad)
    res = (torch.randn(2, tokens // 2, out, device=DEV).to(BF)
           .requires_grad_() if with_residual else None)
    dy = torch.randn(2, tokens // 2, out, device=DEV).to(BF)
    before = ext().dgrad_tn_calls()
    before_w = ext().wgrad_tn_calls()
    ops.linear_flat(x, w, res).backward(dy)
    return dict(x=x, w=w, dy=dy, dx=x.grad,
                dres=None if res is None else res.grad,
                gview=w._flat_grad_view, fired=len(fired),
                tn_calls=ext().dgrad_tn_calls() - before,
                wgrad_tn_calls=ext().wgrad_tn_calls() - before_w)


def lower_thresholds(monkeypatch, tokens, out, inn):
    from fms_fsdp_amd import ops
    monkeypatch.setattr(ops, "_DGRAD_TN_MIN_TOKENS", tokens)
    monkeypatch.setattr(ops, "_DGRAD_TN_MIN_WEIGHT", out * inn)


def test_linear_flat_routes(monkeypatch):
    tokens, out, inn = 256, 192, 128
    monkeypatch.delenv("FMS_AMD_DGRAD", raising=False)
    lower_thresholds(monkeypatch, tokens, out, inn)
    r = run_linear_flat(tokens, out, inn)
    assert r["tn_calls"] == 1 and r["fired"] == 1
    dy64 = r["dy"].double().view(tokens, out)
    x64 = r["x"].detach().double().view(tokens, inn)
    w64 = r["w"].detach().double()
    rule.check("linear_flat routed dx", r["dx"].view(tokens, inn),
               dy64 @ w64, dy64.abs() @ w64.abs(), rule.A_REDUCE)
    assert torch.equal(r["dres"], r["dy"])
    rule.check("linear_flat wgrad beside the routed dgrad", r["gview"],
               dy64.t() @ x64, dy64.abs().t() @ x64.abs(), rule.A_REDUCE)


def test_linear_flat_env_keeps_old_route(monkeypatch):
    tokens, out, inn = 256, 192, 128
    lower_thresholds(monkeypatch, tokens, out, inn)
    monkeypatch.setenv("FMS_AMD_DGRAD", "nn")
    r = run_linear_flat(tokens, out, inn)
    assert r["tn_calls"] == 0
    assert torch.equal(r["dx"].view(tokens, inn),
                       r["dy"].view(tokens, out) @ r["w"].detach())


def test_linear_flat_below_thresholds_keeps_old_route(monkeypatch):
    tokens, out, inn = 256, 192, 128
    monkeypatch.delenv("FMS_AMD_DGRAD", raising=False)
    for t, o in ((tokens + 8, out), (tokens, out + 8)):
        lower_thresholds(monkeypatch, t, o, inn)
        r = run_linear_flat(tokens, out, inn)
        assert r["tn_calls"] == 0
        assert torch.equal(r["dx"].view(tokens, inn),
                           r["dy"].view(tokens, out) @ r["w"].detach())


def test_linear_flat_no_dgrad_when_x_needs_none(monkeypatch):
    tokens, out, inn = 256, 192, 128
    monkeypatch.delenv("FMS_AMD_DGRAD", raising=False)
    lower_thresholds(monkeypatch, tokens, out, inn)
    r = run_linear_flat(tokens, out, inn, x_grad=False)
    assert r["tn_calls"] == 0 and r["wgrad_tn_calls"] == 0
    assert r["dx"] is None and r["fired"] == 1
    assert torch.equal(r["dres"], r["dy"])
    assert torch.isfinite(r["gview"]).all()


def test_routing_rule(monkeypatch):
    """The measured rule on the 7B block's own shapes."""
    from fms_fsdp_amd import ops
    monkeypatch.delenv("FMS_AMD_DGRAD", raising=False)

    def routed(tokens, out, inn, dtype=BF):
        dy = torch.empty(tokens, out, device=DEV, dtype=dtype)
        w = torch.empty(out, inn, device=DEV, dtype=dtype)
        return ops._dgrad_mode(dy, w)

    assert routed(8192, 12288, 4096)          # qkv
    assert routed(8192, 22016, 4096)          # gate|up
    assert routed(8192, 4096, 11008)          # down
    assert not routed(8192, 4096, 4096)       # proj: square, no gain
    assert not routed(4096, 22016, 4096)      # below the token rule
    assert not routed(8192, 12288, 4096, torch.float32)
    assert not routed(8192, 12292, 4096)      # out % 8
    w = torch.empty(12288, 4096, device=DEV, dtype=BF)
    wide = torch.empty(8192, 12288 + 8, device=DEV, dtype=BF)
    assert ops._dgrad_mode(wide[:, 8:], w)    # row-strided dy: in place
    assert not ops._dgrad_mode(wide[:, 8:4104], w)    # inner sizes differ
    assert not ops._dgrad_mode(
        torch.empty(8192, 4096, device=DEV, dtype=BF), w.t())   # w.t() view
    monkeypatch.setenv("FMS_AMD_DGRAD", "nn")
    assert not routed(8192, 12288, 4096)


# --------------------------------------------------------------------------
# a two-layer Llama under ShardedModel, one step on each route
# --------------------------------------------------------------------------
NLAYERS = 2


def llama_step(ac):
    """-> ({param name: its slice of the flat grad buffer}, dgrad_tn calls,
    loss) of one forward + backward from a fixed seed."""
    from fms_fsdp_amd.models import Llama, LlamaBlock, LlamaConfig
    from fms_fsdp_amd.parallel import ShardedModel
    from fms_fsdp_amd.parallel.policies import apply_selective_ac
    torch.manual_seed(0)
    cfg = LlamaConfig(src_vocab_size=512, emb_dim=256, nheads=2, kvheads=2,
                      nlayers=NLAYERS, max_expected_seq_len=256)
    with torch.device(DEV):
        m = Llama(cfg)
        m.reset_parameters()
    if ac:
        apply_selective_ac(m, LlamaBlock, 1)
    sm = ShardedModel(m, LlamaBlock, sharding_strategy="fsdp",
                      param_dtype=BF)
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 512, (2, 256), generator=g).to(DEV)
    y = torch.randint(0, 512, (2, 256), generator=g).to(DEV)
    before = ext().dgrad_tn_calls()
    sm.zero_grad()
    loss = sm(x, labels=y)
    loss.backward()
    grads = {}
    for u in sm.all_units:
        for n, p, off in zip(u.param_names, u.params, u.offsets):
            sl = u.flat_grad[off:off + p.numel()]
            grads[f"{u.name}.{n}"] = sl.detach().clone().view(p.shape)
    return grads, ext().dgrad_tn_calls() - before, float(loss.detach())


def compare_grads(name, new, old):
    """The two routes round the same fp32-accurate sums, so a routed dx
    differs from the old one by at most one bf16 rounding per element (R =
    2^-8, relative). Every grad is linear in those dx and lies behind at
    most 4 routed dgrads per layer, whose relative perturbations add to
    first order: |new - old| <= R |old| + 4 NLAYERS R mag, with mag[i, j] =
    sum_t |dy[t, i]| |x[t, j]| for a weight grad. That sum is not at hand
    for a whole model. Row i of a weight grad shares dy[:, i], and the x[:,
    j] are normalised activations of one scale, so mag varies little along
    a row and is at least every |old| of the row: the row's largest |old|
    stands in for it, per row (a 1-D norm weight counts as one row). A row
    that is zero on the old route (an embedding row of an unused token)
    must be zero on the new one."""
    assert sorted(new) == sorted(old)
    R = rule.rounding(BF)
    for n in sorted(old):
        o = old[n].double()
        assert torch.isfinite(new[n]).all(), n
        assert o.abs().max() > 0, n
        scale = o.abs().amax(dim=-1, keepdim=True).expand_as(o).clone()
        rule.check(f"{name} {n}", new[n], o, scale, A=4 * NLAYERS * R, R=R)


def test_llama_step_both_routes(monkeypatch):
    from fms_fsdp_amd import ops
    monkeypatch.setattr(ops, "_DGRAD_TN_MIN_TOKENS", 8)
    monkeypatch.setattr(ops, "_DGRAD_TN_MIN_WEIGHT", 64)
    monkeypatch.setenv("FMS_AMD_DGRAD", "nn")
    old, old_calls, old_loss = llama_step(ac=False)
    monkeypatch.delenv("FMS_AMD_DGRAD")
    new, new_calls, new_loss = llama_step(ac=False)
    assert old_calls == 0 and new_calls == 4 * NLAYERS
    assert abs(new_loss - old_loss) <= 1e-5 * abs(old_loss)   # same forward
    compare_grads("llama new vs old", new, old)
    # recomputed blocks hand the backward re-wrapped tensors: same route
    ac, ac_calls, _ = llama_step(ac=True)
    assert ac_calls == 4 * NLAYERS
    compare_grads("llama AC new vs old", ac, old)
