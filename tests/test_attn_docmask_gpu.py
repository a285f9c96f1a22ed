"""Document-masked causal attention on the GPU: attn_fwd_kernel<D, true>,
attn_bwd_dq_recompute_kernel<D, true> and the masked key-lane dkv kernel
behind _C.attn_fwd_doc / _C.attn_bwd_doc, and the public paths above them.

One document and 128-aligned documents are bit-identical to the unmasked
kernels (on the row, resp. on each document's slice); unaligned boundaries
go against the fp32 masked SDPA reference with the metric and tolerances of
test_attn_bwd_nows_gpu.py.

Outputs are torch.empty inside the bindings, so every call is preceded by
allocating and freeing NaN-filled tensors of the output sizes and dtypes,
and the outputs are checked for NaN."""

import functools

import pytest
import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference

pytestmark = pytest.mark.gpu

MIB = 1 << 20
BWD_TOL = 6e-2
FWD_TOL = 3e-2
BF, F32 = torch.bfloat16, torch.float32

ONE_DOC_SHAPES = [
    (1, 128, 2, 2, 128),
    (3, 640, 4, 4, 64),
    (2, 512, 12, 4, 64),
    (1, 1152, 16, 4, 128),
]
# (s, starts): every document a multiple of 128 long
ALIGNED = [(384, (0, 128, 256)), (640, (0, 256))]
# (h, kvh, d): MHA and GQA at both head dims
HEADS = [(2, 2, 64), (2, 2, 128), (4, 2, 64), (4, 2, 128)]
# (s, one start set per batch row)
UNALIGNED = {
    "inside_a_wave": (256, ((0, 37),)),
    "multiple_of_32": (256, ((0, 96),)),
    "defer_max": (256, ((0, 200),)),
    "one_token_docs": (256, ((0, 60, 61, 62, 63, 64, 65, 66),)),
    "last_alone": (256, ((0, 255),)),
    "several_blocks": (640, ((0, 130, 515),)),
    "two_rows": (256, ((0, 37), (0, 96, 200))),
}
SPAN = (640, ((0, 130, 515),))
MEM_SHAPE = (1, 2048, 4, 4, 64)     # a workspace would be 32 MiB


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def poison(*specs):
    """Fill blocks of the given (shape, dtype) with NaN and hand them back
    to the caching allocator."""
    junk = [torch.full(shape, float("nan"), device=dev(), dtype=dtype)
            for shape, dtype in specs]
    torch.cuda.synchronize()
    del junk


class ws_limit:
    def __init__(self, nbytes):
        self.nbytes = nbytes

    def __enter__(self):
        from fms_fsdp_amd import _C
        self.prev = _C.attn_bwd_ws_limit(self.nbytes)

    def __exit__(self, *exc):
        from fms_fsdp_amd import _C
        _C.attn_bwd_ws_limit(self.prev)


class sched_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from fms_fsdp_amd import _C
        self.prev = _C.attn_sched_mode(self.mode)

    def __exit__(self, *exc):
        from fms_fsdp_amd import _C
        _C.attn_sched_mode(self.prev)


class dkv_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from fms_fsdp_amd import _C
        self.prev = _C.attn_dkv_mode(self.mode)

    def __exit__(self, *exc):
        from fms_fsdp_amd import _C
        _C.attn_dkv_mode(self.prev)


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=2468):
    b, s, h, kvh, d = shape
    g = torch.Generator(device=dev()).manual_seed(seed)
    mk = lambda nh: torch.randn(b, s, nh, d, device=dev(), generator=g,
                                dtype=torch.bfloat16)
    return mk(h), mk(kvh), mk(kvh), mk(h)   # q, k, v, do


@functools.lru_cache(maxsize=None)
def doc_mask(s, rows):
    """rows: one tuple of document starts per batch row."""
    start = torch.zeros(len(rows), s, dtype=torch.int32)
    for r, starts in enumerate(rows):
        for a in starts:
            start[r, a:] = a
    return ops.doc_mask_from_starts(start.to(dev()))


def poison_outputs(shape):
    b, s, h, kvh, d = shape
    kv_dtype = BF if kvh == h else F32
    poison(((b, s, h, d), BF), ((b, s, kvh, d), kv_dtype),
           ((b, s, kvh, d), kv_dtype), ((b, h, s), F32), ((b, h, s), F32))


def run_masked(q, k, v, do, mask):
    """fwd + bwd through the masked bindings."""
    from fms_fsdp_amd import _C
    shape = (*q.shape[:3], k.shape[2], q.shape[3])
    poison_outputs(shape)
    o, lse = _C.attn_fwd_doc(q, k, v, mask.start)
    poison_outputs(shape)
    dq, dk, dv = _C.attn_bwd_doc(do, q, k, v, o, lse, None, mask.start,
                                 mask.end)
    torch.cuda.synchronize()
    out = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    for name, t in out.items():
        assert not torch.isnan(t).any(), name
    return out


def run_unmasked(q, k, v, do):
    """fwd + workspace-free bwd through the unmasked bindings."""
    from fms_fsdp_amd import _C
    shape = (*q.shape[:3], k.shape[2], q.shape[3])
    with ws_limit(0):
        poison_outputs(shape)
        o, lse = _C.attn_fwd(q, k, v)
        poison_outputs(shape)
        dq, dk, dv = _C.attn_bwd(do, q, k, v, o, lse, None)
        torch.cuda.synchronize()
    out = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    for name, t in out.items():
        assert not torch.isnan(t).any(), name
    return out


def masked_reference(q, k, v, do, mask):
    """fp32 masked SDPA autograd."""
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    o = reference.attention_causal(qf, kf, vf, doc_mask=mask)
    o.backward(do.float())
    return dict(o=o.detach(), dq=qf.grad, dk=kf.grad, dv=vf.grad)


def check_against_reference(got, ref, what):
    errs = {n: relerr(got[n], ref[n]) for n in ("o", "dq", "dk", "dv")}
    print(what, errs)
    assert errs["o"] < FWD_TOL, errs
    assert max(errs["dq"], errs["dk"], errs["dv"]) < BWD_TOL, errs


def exact_names(h, kvh):
    """GQA dk/dv accumulate through fp32 atomics: order-dependent."""
    return ["o", "lse", "dq"] + (["dk", "dv"] if kvh == h else [])


# ---- 1. one document ---------------------------------------------------
@pytest.mark.parametrize("shape", ONE_DOC_SHAPES, ids=str)
def test_one_document_is_the_unmasked_kernel(shape):
    b, s, h, kvh, d = shape
    q, k, v, do = inputs(shape)
    got = run_masked(q, k, v, do, doc_mask(s, ((0,),) * b))
    plain = run_unmasked(q, k, v, do)
    for name in exact_names(h, kvh):
        assert torch.equal(got[name], plain[name]), name
    if kvh != h:
        ref = masked_reference(q, k, v, do, doc_mask(s, ((0,),) * b))
        check_against_reference(got, ref, shape)


# ---- 2. documents of whole 128-row tiles -------------------------------
@pytest.mark.parametrize("heads", [(2, 2, 128), (4, 2, 64)], ids=str)
@pytest.mark.parametrize("s,starts", ALIGNED, ids=str)
def test_aligned_documents_equal_their_slices(s, starts, heads):
    h, kvh, d = heads
    shape = (2, s, h, kvh, d)
    q, k, v, do = inputs(shape)
    got = run_masked(q, k, v, do, doc_mask(s, (starts,) * 2))
    for a, e in zip(starts, starts[1:] + (s,)):
        cut = lambda t: t[:, a:e].contiguous()
        alone = run_unmasked(cut(q), cut(k), cut(v), cut(do))
        for name in exact_names(h, kvh):
            mine = got[name][:, :, a:e] if name == "lse" else got[name][:, a:e]
            assert torch.equal(mine, alone[name]), (name, a, e)
    if kvh != h:
        ref = masked_reference(q, k, v, do, doc_mask(s, (starts,) * 2))
        check_against_reference(got, ref, (shape, starts))


# ---- 3. unaligned boundaries against the fp32 masked reference ----------
@pytest.mark.parametrize("heads", HEADS, ids=str)
@pytest.mark.parametrize("case", list(UNALIGNED))
def test_unaligned_boundaries_match_reference(case, heads):
    s, rows = UNALIGNED[case]
    h, kvh, d = heads
    shape = (len(rows), s, h, kvh, d)
    q, k, v, do = inputs(shape)
    mask = doc_mask(s, rows)
    got = run_masked(q, k, v, do, mask)
    check_against_reference(got, masked_reference(q, k, v, do, mask),
                            (case, heads))


# ---- 4. both workgroup orders -------------------------------------------
@pytest.mark.parametrize("heads", [(2, 2, 128), (4, 2, 64)], ids=str)
def test_balanced_bit_identical_to_legacy(heads):
    s, rows = SPAN
    h, kvh, d = heads
    q, k, v, do = inputs((1, s, h, kvh, d))
    mask = doc_mask(s, rows)
    with sched_mode("balanced"):
        bal = run_masked(q, k, v, do, mask)
    with sched_mode("legacy"):
        leg = run_masked(q, k, v, do, mask)
    for name in exact_names(h, kvh):
        assert torch.equal(bal[name], leg[name]), name


# ---- 5. public paths ----------------------------------------------------
def test_attention_causal_padded():
    b, s, h, kvh, d = 2, 200, 2, 2, 128
    q, k, v, do = inputs((b, s, h, kvh, d), seed=1357)
    mask = doc_mask(s, ((0, 70),) * b)
    ref = masked_reference(q, k, v, do, mask)
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    poison(((b, 256, h, d), BF), ((b, h, 256), F32))
    o = ops.attention_causal(qg, kg, vg, doc_mask=mask)
    poison(((b, 256, h, d), BF), ((b, 256, kvh, d), BF), ((b, 256, kvh, d), BF),
           ((b, h, 256), F32))
    o.backward(do)
    torch.cuda.synchronize()
    got = dict(o=o.detach(), dq=qg.grad, dk=kg.grad, dv=vg.grad)
    for name, t in got.items():
        assert t.shape[1] == s
        assert not torch.isnan(t).any(), name
    check_against_reference(got, ref, "attention_causal s=200")


def test_attention_causal_fp16_and_fp32():
    b, s, h, kvh, d = 1, 256, 2, 2, 64
    q, k, v, do = inputs((b, s, h, kvh, d))
    mask = doc_mask(s, ((0, 37),))
    ref = masked_reference(q, k, v, do, mask)
    o16 = ops.attention_causal(q.half(), k.half(), v.half(), doc_mask=mask)
    assert o16.dtype == torch.float16 and not torch.isnan(o16).any()
    assert relerr(o16, ref["o"]) < FWD_TOL
    o32 = ops.attention_causal(q.float(), k.float(), v.float(), doc_mask=mask)
    torch.testing.assert_close(o32, ref["o"])


@pytest.mark.parametrize("shape,rows", [
    ((2, 256, 4, 4, 128), ((0, 37), (0, 96, 200))),
    ((2, 256, 4, 2, 64), ((0, 37), (0, 96, 200))),
], ids=["mha_d128", "gqa_d64"])
def test_qkv_rope_attention(shape, rows):
    b, s, h, kvh, d = shape
    hq, hk = h * d, kvh * d
    E = hq + 2 * hk
    g = torch.Generator(device=dev()).manual_seed(4321)
    qkv = torch.randn(b, s, E, device=dev(), generator=g, dtype=BF)
    do = torch.randn(b, s, h, d, device=dev(), generator=g, dtype=BF)
    pos = torch.arange(s, dtype=torch.float32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    ang = torch.outer(pos, inv)
    cos, sin = ang.cos().to(dev()), ang.sin().to(dev())
    mask = doc_mask(s, rows)

    a = qkv.clone().requires_grad_()
    poison(((b, s, h, d), BF), ((b, h, s), F32))
    o = ops.qkv_rope_attention(a, cos, sin, h, kvh, d, doc_mask=mask)
    poison(((b, s, E), BF), ((b, s, h, d), BF), ((b, s, kvh, d), BF),
           ((b, h, s), F32))
    o.backward(do)
    torch.cuda.synchronize()
    assert not torch.isnan(o).any() and not torch.isnan(a.grad).any()

    af = qkv.float().requires_grad_()
    qf, kf, vf = af.split([hq, hk, hk], dim=-1)
    qr, kr = reference.rope_apply(qf.view(b, s, h, d), kf.view(b, s, kvh, d),
                                  cos, sin)
    of = reference.attention_causal(qr, kr, vf.view(b, s, kvh, d),
                                    doc_mask=mask)
    of.backward(do.float())
    errs = dict(o=relerr(o, of),
                dq=relerr(a.grad[..., :hq], af.grad[..., :hq]),
                dk=relerr(a.grad[..., hq:hq + hk], af.grad[..., hq:hq + hk]),
                dv=relerr(a.grad[..., hq + hk:], af.grad[..., hq + hk:]))
    print(shape, errs)
    assert errs["o"] < FWD_TOL, errs
    assert max(errs["dq"], errs["dk"], errs["dv"]) < BWD_TOL, errs


@pytest.mark.parametrize("heads", [(2, 2, 128), (4, 2, 64)], ids=str)
def test_dkv_mode_does_not_govern_masked_calls(heads):
    s, rows = SPAN
    h, kvh, d = heads
    q, k, v, do = inputs((1, s, h, kvh, d))
    mask = doc_mask(s, rows)
    with dkv_mode("keylane"):
        keylane = run_masked(q, k, v, do, mask)
    with dkv_mode("legacy"):
        legacy = run_masked(q, k, v, do, mask)
    for name in exact_names(h, kvh):
        assert torch.equal(keylane[name], legacy[name]), name
    check_against_reference(legacy, masked_reference(q, k, v, do, mask),
                            ("dkv legacy", heads))


def test_no_workspace_is_allocated_at_the_default_limit():
    from fms_fsdp_amd import _C
    b, s, h, kvh, d = MEM_SHAPE
    q, k, v, do = inputs(MEM_SHAPE)
    mask = doc_mask(s, ((0,),))
    ws_bytes = b * h * s * s * 2
    assert ws_bytes == 32 * MIB
    assert _C.attn_bwd_ws_limit() >= ws_bytes    # unmasked would take it
    o, lse = _C.attn_fwd_doc(q, k, v, mask.start)
    args = (do, q, k, v, o, lse, None, mask.start, mask.end)
    _C.attn_bwd_doc(*args)                        # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = _C.attn_bwd_doc(*args)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise MiB", rise / MIB)
    assert rise < ws_bytes // 4, rise
    for t in out:
        assert not torch.isnan(t).any()


@pytest.mark.parametrize("ac", [False, True], ids=["plain", "checkpointed"])
def test_llama_on_gpu_masks_at_the_eos(ac):
    """bf16 model through the fused qkv+rope+attention path (s % 128 == 0,
    head_dim 64). Every other op works row by row, the MHA kernels have no
    atomics and the masked attention does not leak (test below), so the
    second document's logits do not change by a bit."""
    from fms_fsdp_amd.models import Llama, LlamaConfig
    torch.manual_seed(0)
    cfg = LlamaConfig(src_vocab_size=64, emb_dim=128, nheads=2, nlayers=2,
                      max_expected_seq_len=256)
    with torch.device(dev()):
        model = Llama(cfg)
        model.reset_parameters()
    model = model.bfloat16()
    for layer in model.layers:
        layer._ac_enabled = ac
    eos, cut = 0, 131                   # first document = positions 0..130
    g = torch.Generator().manual_seed(5)
    t = torch.randint(1, 64, (2, 256), generator=g)
    t[:, cut - 1] = eos
    t2 = t.clone()
    t2[:, :cut - 1] = (t[:, :cut - 1] % 63) + 1
    t, t2 = t.to(dev()), t2.to(dev())

    plain, plain2 = model(t), model(t2)
    assert not torch.equal(plain[:, cut:], plain2[:, cut:])
    model.doc_mask_token = eos
    masked, masked2 = model(t), model(t2)
    assert not torch.isnan(masked).any()
    assert torch.equal(masked[:, cut:], masked2[:, cut:])
    assert not torch.equal(masked[:, :cut], masked2[:, :cut])
    assert not torch.equal(masked[:, cut:], plain[:, cut:])

    labels = torch.roll(t, -1, dims=1)
    labels[:, :cut] = -100
    loss = model(t, labels=labels)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for name, p in model.named_parameters():
        assert p.grad is not None and not torch.isnan(p.grad).any(), name
    # first-document tokens other than the eos got no gradient
    used = torch.zeros(64, dtype=torch.bool, device=dev())
    used[t[:, cut:].reshape(-1)] = True
    assert torch.count_nonzero(model.embedding.weight.grad[~used]) == 0
    assert (~used).any()


# ---- 6. leakage -----------------------------------------------------------
def test_second_document_does_not_see_the_first():
    s, rows = SPAN
    a, e = rows[0][1], rows[0][2]           # second document = [130, 515)
    shape = (1, s, 2, 2, 128)
    mask = doc_mask(s, rows)
    base = run_masked(*inputs(shape), mask)
    changed = [t.clone() for t in inputs(shape)]
    for t, other in zip(changed, inputs(shape, seed=97531)):
        t[:, :a] = other[:, :a]
    assert not torch.equal(changed[0], inputs(shape)[0])
    again = run_masked(*changed, mask)
    for name in ("o", "dq", "dk", "dv"):
        assert torch.equal(again[name][:, a:e], base[name][:, a:e]), name
        assert not torch.equal(again[name][:, :a], base[name][:, :a]), name
