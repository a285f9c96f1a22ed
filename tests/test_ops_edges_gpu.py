"""The non-attention, non-SSD kernels at the sizes and edges training
runs them at: row loops that iterate, grid-stride loops that stride,
partial blocks and chunks, strided views, every dtype instantiation.
Each output is held to the one rule of tests/oracle_rule.py against a
float64 reference computed on the GPU from the kernel's own inputs."""

import pytest
import torch
import torch.nn.functional as F

import oracle_rule as rule

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
A_RED, A_CH = rule.A_REDUCE, rule.A_CHAIN
# results below the smallest normal fp32 may be flushed to zero
FLUSH = 2.0 ** -126


def dev():
    return torch.device("cuda:0")


def ext():
    from fms_fsdp_amd import _C
    return _C


def randn(*shape, dtype=BF, scale=1.0):
    return (torch.randn(*shape, device=dev()) * scale).to(dtype)


# ---------------------------------------------------------------------
# rmsnorm
# ---------------------------------------------------------------------
EPS = 1e-6


def _rms64(x64, w64):
    r = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + EPS)
    return x64 * r * w64, r


@pytest.mark.parametrize("rows,H", [(2051, 256), (5, 8)])
def test_rmsnorm_fwd(rows, H):
    torch.manual_seed(rows)
    x, w = randn(rows, H), randn(H)
    y, rinv = ext().rmsnorm_fwd(x, w, EPS)
    y_r, r_r = _rms64(x.double(), w.double())
    tag = f"[{rows}x{H}]"
    rule.check("rmsnorm_fwd.y" + tag, y, y_r, y_r.abs(), A_RED)
    rule.check("rmsnorm_fwd.rinv" + tag, rinv, r_r[:, 0], r_r[:, 0], A_RED)


@pytest.mark.parametrize("rows,H", [(2051, 256), (5, 8)])
def test_add_rmsnorm_fwd(rows, H):
    torch.manual_seed(rows + 1)
    x, res, w = randn(rows, H), randn(rows, H), randn(H)
    y, s, rinv = ext().add_rmsnorm_fwd(x, res, w, EPS)
    tag = f"[{rows}x{H}]"
    s_r = x.double() + res.double()
    rule.check("add_rmsnorm_fwd.s" + tag, s, s_r,
               x.double().abs() + res.double().abs(), A_CH)
    # y is defined on the bf16 residual stream the kernel emits
    y_r, r_r = _rms64(s.double(), w.double())
    rule.check("add_rmsnorm_fwd.y" + tag, y, y_r, y_r.abs(), A_RED)
    rule.check("add_rmsnorm_fwd.rinv" + tag, rinv, r_r[:, 0], r_r[:, 0],
               A_RED)


@pytest.mark.parametrize("with_dextra", [False, True])
@pytest.mark.parametrize("rows,H", [(2051, 256), (5, 8)])
def test_rmsnorm_bwd(rows, H, with_dextra):
    torch.manual_seed(rows + 2)
    x, w, dy = randn(rows, H), randn(H), randn(rows, H)
    de = randn(rows, H) if with_dextra else None
    _, rinv = ext().rmsnorm_fwd(x, w, EPS)
    dx, dw = ext().rmsnorm_bwd(dy, x, w, rinv, de)
    x64 = x.double().requires_grad_()
    w64 = w.double().requires_grad_()
    y_r, r = _rms64(x64, w64)
    dx_r, dw_r = torch.autograd.grad(y_r, (x64, w64), dy.double())
    with torch.no_grad():
        r = r.detach()
        a = (dy.double() * w64).abs()
        # dx = r*w*dy - (r^3/H) * x * sum_j dy_j w_j x_j  (+ dextra)
        m_dx = r * a + r.pow(3) / H * x64.abs() * \
            (a * x64.abs()).sum(-1, keepdim=True)
        if with_dextra:
            dx_r = dx_r + de.double()
            m_dx = m_dx + de.double().abs()
        m_dw = (dy.double() * x64 * r).abs().sum(0)
    tag = f"[{rows}x{H},dextra={int(with_dextra)}]"
    rule.check("rmsnorm_bwd.dx" + tag, dx, dx_r, m_dx, A_RED)
    rule.check("rmsnorm_bwd.dw" + tag, dw, dw_r, m_dw, A_RED)


# ---------------------------------------------------------------------
# cross-entropy (in place: logits -> dlogits, loss accumulated)
# ---------------------------------------------------------------------
def _ce_case(tag, logits, labels):
    rows, V = logits.shape
    keep = labels != -100
    count = keep.sum().clamp(min=1).float()
    loss_sum = torch.zeros((), device=dev())
    work = logits.clone()
    ext().ce_fwd_bwd(work, labels, loss_sum, count, -100)

    x = logits.double()
    M = x.max(-1, keepdim=True).values
    l = torch.exp(x - M).sum(-1, keepdim=True)
    p = torch.exp(x - M) / l
    onehot = torch.zeros_like(p)
    safe = labels.clamp(min=0)
    onehot[torch.arange(rows, device=dev()), safe] = 1.0
    kd = keep[:, None].double()
    denom = count.double()
    ref = (p - onehot) / denom * kd
    mag = (p + onehot) / denom * kd
    mag = rule.widen(mag, torch.full_like(mag, FLUSH))
    rule.check("ce_fwd_bwd.dlogits" + tag, work, ref, mag, A_RED)
    assert (work[~keep].view(torch.int16) == 0).all()
    xl = x[torch.arange(rows, device=dev()), safe]
    per_row = (M[:, 0] + torch.log(l[:, 0]) - xl) * keep.double()
    m_row = (M[:, 0].abs() + torch.log(l[:, 0]).abs() + xl.abs()) \
        * keep.double()
    rule.check("ce_fwd_bwd.loss_sum" + tag, loss_sum, per_row.sum(), m_row.sum(),
               A_RED)


def test_ce_many_rows():
    torch.manual_seed(10)
    rows, V = 2051, 1024
    logits = randn(rows, V, dtype=torch.float32, scale=3.0)
    logits[5::97] *= 30          # the online max rescales many times
    logits = logits.bfloat16()
    labels = torch.randint(0, V, (rows,), device=dev())
    labels[0::5] = 0
    labels[1::5] = V - 1
    labels[3::7] = -100          # ignored rows scattered through the batch
    labels[2040:2049] = -100
    assert (labels[2048:] != -100).any()
    _ce_case("[2051x1024]", logits, labels)


def test_ce_wide_vocab():
    torch.manual_seed(11)
    rows, V = 16, 50280          # V % 8 == 0, V % 16 != 0
    logits = randn(rows, V, scale=3.0)
    labels = torch.randint(0, V, (rows,), device=dev())
    labels[0], labels[1], labels[2] = 0, V - 1, -100
    _ce_case("[16x50280]", logits, labels)


def test_ce_all_ignored():
    torch.manual_seed(12)
    rows, V = 2051, 1024
    work = randn(rows, V, scale=3.0)
    labels = torch.full((rows,), -100, device=dev(), dtype=torch.int64)
    loss_sum = torch.zeros((), device=dev())
    ext().ce_fwd_bwd(work, labels, loss_sum, torch.ones((), device=dev()),
                     -100)
    assert loss_sum.item() == 0.0
    assert (work.view(torch.int16) == 0).all()


# ---------------------------------------------------------------------
# sq_norm_accum
# ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF, torch.float16])
def test_sq_norm_accum(dtype):
    torch.manual_seed(20)
    n = 3_000_004                 # > 2048*256 quads: the stride loop runs
    a, b = randn(n, dtype=dtype), randn(n, dtype=dtype, scale=0.5)
    out = torch.zeros((), device=dev())
    ext().sq_norm_accum(a, out)
    ext().sq_norm_accum(b, out)
    ref = a.double().pow(2).sum() + b.double().pow(2).sum()
    rule.check(f"sq_norm_accum[{str(dtype)[6:]}]", out, ref, ref, A_RED)


# ---------------------------------------------------------------------
# adamw
# ---------------------------------------------------------------------
@pytest.mark.parametrize("pub", [None, BF, torch.float16])
@pytest.mark.parametrize("gdt", [torch.float32, BF, torch.float16])
def test_adamw(gdt, pub):
    torch.manual_seed(30)
    n = 3076                      # 769 quads: a partial last block
    lr, b1, b2, eps, wd = 0.1, 0.9, 0.95, 1e-8, 0.1
    p = randn(n, dtype=torch.float32)
    m = torch.zeros(n, device=dev())
    v = torch.zeros(n, device=dev())
    scale = torch.tensor(0.37, device=dev())
    shard = torch.zeros(n, device=dev(), dtype=pub) if pub else None
    p64, m64, v64 = p.double(), m.double(), v.double()
    p0 = p64.clone()
    mag_p, mag_m = p64.abs(), m64.abs()
    gs = scale.double()
    tag = f"[g={str(gdt)[6:]},pub={str(pub)[6:] if pub else None}]"
    for step in range(1, 4):
        g = randn(n, dtype=gdt)
        ext().adamw(p, g, m, v, float(step), lr, b1, b2, eps, wd, scale,
                    shard)
        g64 = g.double() * gs
        p64 = p64 * (1 - lr * wd)
        m64 = b1 * m64 + (1 - b1) * g64
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        upd = lr / (1 - b1 ** step) * m64 / \
            ((v64 / (1 - b2 ** step)).sqrt() + eps)
        p64 = p64 - upd
        mag_m = b1 * mag_m + (1 - b1) * g64.abs()
        mag_p = mag_p + upd.abs()
        rule.check(f"adamw.p{tag}", p, p64, mag_p, A_CH)
        rule.check(f"adamw.m{tag}", m, m64, mag_m, A_CH)
        rule.check(f"adamw.v{tag}", v, v64, v64, A_CH)
        if pub:
            assert torch.equal(shard.view(torch.int16),
                               p.to(pub).view(torch.int16))
    # lr = 0.1: three steps moved p visibly
    assert (p64 - p0).abs().median() > 0.05


# ---------------------------------------------------------------------
# swiglu
# ---------------------------------------------------------------------
@pytest.mark.parametrize("rows,H", [(3, 8), (257, 1000)])
def test_swiglu(rows, H):
    torch.manual_seed(40 + rows)
    gu = randn(rows, 2 * H, scale=2.0)
    dy = randn(rows, H)
    h = ext().swiglu_fwd(gu)
    dgu = ext().swiglu_bwd(dy, gu)
    g, u = gu.double().chunk(2, -1)
    s = torch.sigmoid(g)
    d = dy.double()
    tag = f"[{rows}x{H}]"
    h_r = g * s * u
    rule.check("swiglu_fwd.h" + tag, h, h_r, h_r.abs(), A_CH)
    dg_r = d * u * s * (1 + g * (1 - s))
    m_dg = (d * u).abs() * s * (1 + g.abs() * (1 - s))
    du_r = d * g * s
    rule.check("swiglu_bwd.dg" + tag, dgu[:, :H], dg_r, m_dg, A_CH)
    rule.check("swiglu_bwd.du" + tag, dgu[:, H:], du_r, du_r.abs(), A_CH)


# ---------------------------------------------------------------------
# rope
# ---------------------------------------------------------------------
def _rope64(t, cos, sin, conj):
    d2 = t.shape[-1] // 2
    t1, t2 = t.double()[..., :d2], t.double()[..., d2:]
    c = cos.double().view(1, -1, 1, d2)
    s = sin.double().view(1, -1, 1, d2) * (-1.0 if conj else 1.0)
    ref = torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], -1)
    mag = torch.cat([(t1 * c).abs() + (t2 * s).abs(),
                     (t2 * c).abs() + (t1 * s).abs()], -1)
    return ref, mag


@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("d", [16, 64])
def test_rope_strided(d, conj):
    torch.manual_seed(50 + d)
    b, s, h, kvh = 2, 77, 4, 2
    fr = torch.outer(torch.arange(s).float(),
                     1.0 / (10000.0 ** (torch.arange(0, d, 2).float() / d)))
    cos, sin = fr.cos().to(dev()), fr.sin().to(dev())
    hq, hk = h * d, kvh * d
    qkv = randn(b, s, hq + 2 * hk)
    q = qkv[..., :hq].view(b, s, h, d)
    k = qkv[..., hq:hq + hk].view(b, s, kvh, d)
    assert not q.is_contiguous() and not k.is_contiguous()
    qo, ko = ext().rope_fwd(q, k, cos, sin, conj)
    tag = f"[d={d},conj={int(conj)}]"
    rule.check("rope_fwd.q" + tag, qo, *_rope64(q, cos, sin, conj), A_CH)
    rule.check("rope_fwd.k" + tag, ko, *_rope64(k, cos, sin, conj), A_CH)

    # scatter into the k slice of a fused buffer; the rest stays untouched
    src = randn(b, s, kvh, d)
    buf = torch.full((b, s, hq + 2 * hk), 123.0, device=dev(), dtype=BF)
    before = buf.clone()
    dst = buf[..., hq:hq + hk].view(b, s, kvh, d)
    ext().rope_into(src, dst, cos, sin, conj)
    rule.check("rope_into" + tag, dst, *_rope64(src, cos, sin, conj), A_CH)
    bits, old = buf.view(torch.int16), before.view(torch.int16)
    assert torch.equal(bits[..., :hq], old[..., :hq])
    assert torch.equal(bits[..., hq + hk:], old[..., hq + hk:])


# ---------------------------------------------------------------------
# causal conv1d + silu
# ---------------------------------------------------------------------
def _conv_lin(x, w, bias):
    W = w.shape[1]
    return F.conv1d(F.pad(x.transpose(1, 2), (W - 1, 0)), w.unsqueeze(1),
                    bias, groups=w.shape[0]).transpose(1, 2)


@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("L", [1, 5, 64, 100])
@pytest.mark.parametrize("W", [2, 3, 4])
def test_causal_conv1d(W, L, C):
    torch.manual_seed(W * 1000 + L * 10 + C)
    b = 3
    x, w, dy = randn(b, L, C), randn(C, W, scale=0.5), randn(b, L, C)
    bias = randn(C, dtype=torch.float32)
    y = ext().cconv_fwd(x, w, bias)
    dx, dw, db = ext().cconv_bwd(dy, x, w, bias)

    x64 = x.double().requires_grad_()
    w64 = w.double().requires_grad_()
    b64 = bias.double().requires_grad_()
    z = _conv_lin(x64, w64, b64)
    y_r = z * torch.sigmoid(z)
    dx_r, dw_r, db_r = torch.autograd.grad(y_r, (x64, w64, b64), dy.double())
    with torch.no_grad():
        sg = torch.sigmoid(z)
        dsilu = sg * (1 + z * (1 - sg))
        m_z = _conv_lin(x64.abs(), w64.abs(), b64.abs())
        # an error e in the pre-activation moves y by silu'(z) * e
        m_y = m_z * dsilu.abs() + y_r.abs()
        # |g| without the cancellation inside silu'(z) = sg*(1 + z*(1-sg))
        g_abs = dy.double().abs() * sg * (1 + z.abs() * (1 - sg))
    xa = x64.detach().abs().requires_grad_()
    wa = w64.detach().abs().requires_grad_()
    ba = b64.detach().abs().requires_grad_()
    m_dx, m_dw, m_db = torch.autograd.grad(_conv_lin(xa, wa, ba),
                                           (xa, wa, ba), g_abs)
    # g = dy * silu'(z) passes through a bf16 buffer between the backward
    # kernels, so every summand of dx/dw/db carries a bf16 rounding of its
    # own: 2^-8 * (sum of the summands' magnitudes) on top of the rule
    m_dx = rule.widen(m_dx, 2.0 ** -8 * m_dx)
    m_dw = rule.widen(m_dw, 2.0 ** -8 * m_dw)
    m_db = rule.widen(m_db, 2.0 ** -8 * m_db)
    tag = f"[W={W},L={L},C={C}]"
    rule.check("cconv_fwd.y" + tag, y, y_r, m_y, A_RED)
    rule.check("cconv_bwd.dx" + tag, dx, dx_r, m_dx, A_RED)
    rule.check("cconv_bwd.dw" + tag, dw, dw_r, m_dw, A_RED)
    rule.check("cconv_bwd.db" + tag, db, db_r, m_db, A_RED)


# ---------------------------------------------------------------------
# segsum_exp
# ---------------------------------------------------------------------
@pytest.mark.parametrize("Q", [8, 72])
def test_segsum_exp(Q):
    torch.manual_seed(60 + Q)
    N = 3
    cs = -(torch.rand(N, Q, device=dev()) * 0.5).cumsum(-1).float()
    L = ext().segsum_exp_fwd(cs)
    c64 = cs.double().requires_grad_()
    mask = torch.tril(torch.ones(Q, Q, dtype=torch.bool, device=dev()))
    diff = c64[:, :, None] - c64[:, None, :]
    L_r = torch.exp(diff.masked_fill(~mask, -torch.inf))
    rule.check(f"segsum_exp_fwd[Q={Q}]", L, L_r, L_r.abs(), A_CH)
    assert (L.view(torch.int16)[:, ~mask] == 0).all()
    g = randn(N, Q, Q)
    dcs = ext().segsum_exp_bwd(g, cs)
    (dcs_r,) = torch.autograd.grad(L_r, c64, g.double())
    prod = (g.double() * L_r.detach()).abs()
    rule.check(f"segsum_exp_bwd[Q={Q}]", dcs, dcs_r,
               prod.sum(2) + prod.sum(1), A_RED)


# ---------------------------------------------------------------------
# preconditions: invalid arguments only, refused before any launch
# ---------------------------------------------------------------------
def test_ce_rejects_bad_arguments():
    C = ext()
    R = pytest.raises(RuntimeError)
    f32 = torch.float32
    loss, den = torch.zeros((), device=dev()), torch.ones((), device=dev())
    lab = torch.zeros(4, device=dev(), dtype=torch.int64)
    with R:
        C.ce_fwd_bwd(randn(4, 1004), lab, loss, den, -100)      # V % 8
    with R:
        C.ce_fwd_bwd(randn(4, 1024), lab[:3], loss, den, -100)
    with R:
        C.ce_fwd_bwd(randn(4, 1024), lab, loss.double(), den, -100)
    with R:
        C.ce_fwd_bwd(randn(4, 1024), lab, loss, den.bfloat16(), -100)
    with R:
        C.ce_fwd_bwd(randn(4, 1024, dtype=f32), lab, loss, den, -100)
    torch.cuda.synchronize()


def test_rmsnorm_bwd_rejects_bad_arguments():
    C = ext()
    R = pytest.raises(RuntimeError)
    f32 = torch.float32
    rows, H = 4, 16
    x, dy, w = randn(rows, H), randn(rows, H), randn(H)
    rinv = torch.ones(rows, device=dev())
    with R:
        C.rmsnorm_bwd(randn(rows, 12), randn(rows, 12), randn(12), rinv,
                      None)                                     # H % 8
    with R:
        C.rmsnorm_bwd(dy, x, w.float(), rinv, None)
    with R:
        C.rmsnorm_bwd(dy, x, randn(2 * H)[::2], rinv, None)
    with R:
        C.rmsnorm_bwd(dy, x, randn(H + 8), rinv, None)
    with R:
        C.rmsnorm_bwd(dy, x, w, rinv.bfloat16(), None)
    with R:
        C.rmsnorm_bwd(dy, x, w, rinv[:3], None)
    with R:
        C.rmsnorm_bwd(dy, x, w, rinv, randn(rows, H, dtype=f32))
    with R:
        C.rmsnorm_bwd(dy, x, w, rinv, randn(rows - 1, H))
    with R:
        C.rmsnorm_bwd(dy, x, w, rinv, randn(H, rows).t())
    torch.cuda.synchronize()


def test_adamw_rejects_bad_arguments():
    C = ext()
    R = pytest.raises(RuntimeError)
    f32 = torch.float32
    n = 64
    p, g = randn(n, dtype=f32), randn(n, dtype=f32)
    m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    sc = torch.ones((), device=dev())
    a = (1.0, 1e-3, 0.9, 0.95, 1e-8, 0.1)
    with R:
        C.adamw(p, g[:60], m, v, *a, None, None)
    with R:
        C.adamw(p, randn(2 * n, dtype=f32)[::2], m, v, *a, None, None)
    with R:
        C.adamw(p, g, m[:60], v, *a, None, None)
    with R:
        C.adamw(p, g, m, v.bfloat16(), *a, None, None)
    with R:
        C.adamw(p, g, m.double(), v, *a, None, None)
    with R:
        C.adamw(p, g, m, v, *a, sc.bfloat16(), None)
    with R:
        C.adamw(p, g, m, v, *a, sc.double(), None)
    with R:
        C.adamw(p, g, m, v, *a, None, randn(n - 4))
    with R:
        C.adamw(p, g, m, v, *a, None, randn(2 * n)[::2])
    torch.cuda.synchronize()
