"""Op dispatch: hand-written CDNA4 HIP kernels on GPU, fp32 PyTorch
reference on CPU.

On a ROCm GPU the in-tree extension `fms_fsdp_amd._C` (built by
`__graft_entry__.build()` / `setup.py build_ext --inplace`) is REQUIRED:
ops raise RuntimeError rather than silently falling back to eager
(per-project rule: no silent PyTorch fallback on the GPU path).
"""

import os
from typing import NamedTuple

import torch

from . import reference

# fp16 policy note (reference fpSixteen, mixed_precision.py:5-9): fp16 is
# supported as the STORAGE/COMM dtype; op-internal compute bridges through
# bf16 (identical MFMA rate on CDNA4, wider exponent, fp32 accumulation
# inside every kernel) so the HIP kernels stay single-dtype. The casts are
# autograd-tracked, so gradients flow back to the fp16 tensors.
#
# fp32 activations on GPU (bf16_working / fp32 policies) take the fp32
# reference implementations by DESIGN: "working precision fp32" means the
# math genuinely runs in fp32 (the bf16 MFMA kernels would silently drop
# precision), and at fp32 rates the eager ops are not the bottleneck. The
# default (bf16) path never touches this branch.

_C = None
_C_err = None
try:
    from fms_fsdp_amd import _C  # built in-tree, travels with the repo snapshot
except ImportError as e:  # pragma: no cover - exercised only when unbuilt
    _C_err = e


def _require_ext(op):
    if _C is None:
        raise RuntimeError(
            f"fms_fsdp_amd._C HIP extension is required for {op} on GPU but "
            f"could not be imported ({_C_err}). Build it with "
            f"`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950)."
        )
    return _C


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------
# Norm weights follow the direct-wgrad protocol of linear_flat (below):
# a weight the sharded runtime attached to its flat grad buffer
# (`_flat_grad_view`, `_wgrad_done`, `_wgrad_fresh`) gets its grad written
# into that view by the backward kernel itself (bf16, overwrite on the
# first touch since zero_grad, accumulate after) and autograd sees None.
# Per norm and step that removes the fp32 zero-fill, the cast, autograd's
# accumulate and the zero-fill of the slice in zero_grad.
def _direct_wgrad_on(weight):
    return (getattr(weight, "_flat_grad_view", None) is not None
            and weight.requires_grad and torch.is_grad_enabled())


def _stash_wgrad_target(ctx, weight):
    # attribute holders stashed at forward time: saved_tensors can return
    # attr-less re-wrapped tensors (e.g. under AC recompute)
    ctx.gview = weight._flat_grad_view
    ctx.wobj = weight
    ctx.cb = getattr(weight, "_wgrad_done", None)


def _take_wgrad_fresh(ctx):
    """True if this is the first write since zero_grad; clears the flag."""
    fresh = getattr(ctx.wobj, "_wgrad_fresh", False)
    ctx.wobj._wgrad_fresh = False
    return fresh


class _WgradSinkFn(torch.autograd.Function):
    """Identity on a direct-wgrad weight whose backward lands the incoming
    grad in the flat grad view. Puts the paths that never reach a
    grad-writing kernel (CPU reference, fp32 activations, the fp16
    bridge) under the same protocol."""

    @staticmethod
    def forward(ctx, weight):
        _stash_wgrad_target(ctx, weight)
        return weight.view_as(weight)

    @staticmethod
    def backward(ctx, dw):
        if _take_wgrad_fresh(ctx):
            ctx.gview.copy_(dw)
        else:
            ctx.gview.add_(dw)
        if ctx.cb is not None:
            ctx.cb()
        return None


def _rmsnorm_backward(ctx, dy, dextra):
    x2d, weight, rinv = ctx.saved_tensors
    if dy is None:
        dy = torch.zeros_like(x2d)
    dy = dy.contiguous().view_as(x2d)
    if dextra is not None:
        dextra = dextra.contiguous().view_as(x2d)
    if ctx.direct:
        dx = _C.rmsnorm_bwd_into(dy, x2d, weight, rinv, dextra,
                                 ctx.gview.view(-1),
                                 not _take_wgrad_fresh(ctx))
        if ctx.cb is not None:
            ctx.cb()
        return dx.view(ctx.shape), None
    dx, dw = _C.rmsnorm_bwd(dy, x2d, weight, rinv, dextra)
    return dx.view(ctx.shape), dw.to(weight.dtype)


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps, direct=False):
        ext = _require_ext("rmsnorm")
        x2d = x.contiguous().view(-1, x.shape[-1])
        y, rinv = ext.rmsnorm_fwd(x2d, weight, eps)
        ctx.save_for_backward(x2d, weight, rinv)
        ctx.shape = x.shape
        ctx.direct = direct
        if direct:
            _stash_wgrad_target(ctx, weight)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        dx, dw = _rmsnorm_backward(ctx, dy, None)
        return dx, dw, None, None


class _RMSNormResidualFn(torch.autograd.Function):
    """(rmsnorm(x), x): the second output carries the residual stream past
    the norm, so its grad arrives here and rides the dx kernel's `dextra`
    operand instead of a separate elementwise add."""

    @staticmethod
    def forward(ctx, x, weight, eps, direct=False):
        ext = _require_ext("rmsnorm")
        x2d = x.contiguous().view(-1, x.shape[-1])
        y, rinv = ext.rmsnorm_fwd(x2d, weight, eps)
        ctx.save_for_backward(x2d, weight, rinv)
        ctx.shape = x.shape
        ctx.direct = direct
        if direct:
            _stash_wgrad_target(ctx, weight)
        ctx.set_materialize_grads(False)
        # x_res is a view of an input made inside a custom Function:
        # autograd raises if a caller later modifies it in place (a
        # `residual.add_` epilogue would). Treat it as read-only.
        return y.view(x.shape), x2d.view(x.shape)

    @staticmethod
    def backward(ctx, dy, dres):
        dx, dw = _rmsnorm_backward(ctx, dy, dres)
        return dx, dw, None, None


def _rmsnorm_dispatch(fn, x, weight, eps):
    """GPU kernel path of rmsnorm / rmsnorm_residual; None where the
    reference implementation applies (CPU, fp32 activations)."""
    if not (x.is_cuda and x.dtype != torch.float32):
        return None
    if x.dtype == torch.float16:
        if _direct_wgrad_on(weight):
            weight = _WgradSinkFn.apply(weight)
        # only the norm goes through the bf16 bridge: the residual
        # stream stays the caller's exact fp16 x, and autograd adds its
        # grad in fp16
        y = _RMSNormFn.apply(x.bfloat16(), weight.bfloat16(), eps).half()
        return y if fn is _RMSNormFn else (y, x)
    direct = _direct_wgrad_on(weight) and weight.dtype == torch.bfloat16
    if not direct and _direct_wgrad_on(weight):
        weight = _WgradSinkFn.apply(weight)
    return fn.apply(x, weight, eps, direct)


def rmsnorm(x, weight, eps=1e-6):
    y = _rmsnorm_dispatch(_RMSNormFn, x, weight, eps)
    if y is not None:
        return y
    if _direct_wgrad_on(weight):
        weight = _WgradSinkFn.apply(weight)
    return reference.rmsnorm(x, weight, eps)


def rmsnorm_residual(x, weight, eps=1e-6):
    """(rmsnorm(x), x_res) with x_res the values of x: feed x_res as the
    residual of the projection that follows the norm, and the backward
    adds the residual-stream grad inside the norm's dx kernel. fp16, fp32
    and CPU inputs get x itself back and the add stays autograd's. Do not
    modify x_res in place."""
    out = _rmsnorm_dispatch(_RMSNormResidualFn, x, weight, eps)
    if out is not None:
        return out
    if _direct_wgrad_on(weight):
        weight = _WgradSinkFn.apply(weight)
    return reference.rmsnorm(x, weight, eps), x


class _AddRMSNormFn(torch.autograd.Function):
    """Fused s = x + res; y = rmsnorm(s): one HBM pass instead of two.
    Backward fuses the residual grad into the rmsnorm dx kernel."""

    @staticmethod
    def forward(ctx, x, res, weight, eps):
        ext = _require_ext("add_rmsnorm")
        x2d = x.contiguous().view(-1, x.shape[-1])
        r2d = res.contiguous().view_as(x2d)
        y, s, rinv = ext.add_rmsnorm_fwd(x2d, r2d, weight, eps)
        ctx.save_for_backward(s, weight, rinv)
        ctx.shape = x.shape
        return y.view(x.shape), s.view(x.shape)

    @staticmethod
    def backward(ctx, dy, ds):
        s, weight, rinv = ctx.saved_tensors
        dx, dw = _C.rmsnorm_bwd(dy.contiguous().view_as(s), s, weight, rinv,
                                ds.contiguous().view_as(s))
        dx = dx.view(ctx.shape)
        return dx, dx, dw.to(weight.dtype), None


def add_rmsnorm(x, res, weight, eps=1e-6):
    """(rmsnorm(x + res), x + res)"""
    if x.is_cuda and x.dtype != torch.float32:
        if x.dtype == torch.float16:
            y, s = _AddRMSNormFn.apply(x.bfloat16(), res.bfloat16(),
                                       weight.bfloat16(), eps)
            return y.half(), s.half()
        return _AddRMSNormFn.apply(x, res, weight, eps)
    s = (x.float() + res.float()).to(x.dtype)
    return reference.rmsnorm(s, weight, eps), s


# --------------------------------------------------------------------------
# RoPE (half-rotation convention; cos/sin tables (s, d/2) fp32)
# --------------------------------------------------------------------------
def _row_view_ok(t):
    """(b, s, h, d) bf16 view the strided kernels accept directly:
    contiguous within each (b, s) row, uniform row stride (a last-dim
    slice of a fused qkv projection qualifies — no copy needed)."""
    return (t.dim() == 4 and t.stride(3) == 1 and t.stride(2) == t.shape[3]
            and t.stride(1) >= t.shape[2] * t.shape[3]
            and t.stride(0) == t.shape[1] * t.stride(1))


def _as_row_view(t):
    return t if _row_view_ok(t) else t.contiguous()


class _RoPEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin):
        ext = _require_ext("rope")
        cos = cos.float().contiguous()   # tables may arrive bf16 after a
        sin = sin.float().contiguous()   # module-wide .bfloat16() cast
        # strided reads handle fused-qkv slices without a copy
        qo, ko = ext.rope_fwd(_as_row_view(q), _as_row_view(k), cos, sin,
                              False)
        ctx.save_for_backward(cos, sin)
        return qo, ko

    @staticmethod
    def backward(ctx, dq, dk):
        cos, sin = ctx.saved_tensors
        dqo, dko = _C.rope_fwd(_as_row_view(dq), _as_row_view(dk), cos, sin,
                               True)
        return dqo, dko, None, None


def rope_apply(q, k, cos, sin):
    if q.is_cuda and q.dtype != torch.float32:
        if q.dtype == torch.float16:
            qo, ko = _RoPEFn.apply(q.bfloat16(), k.bfloat16(), cos, sin)
            return qo.half(), ko.half()
        return _RoPEFn.apply(q, k, cos, sin)
    return reference.rope_apply(q, k, cos, sin)


# --------------------------------------------------------------------------
# Linear with wgrad written DIRECTLY into the sharded runtime's flat grad
# buffer (hipBLASLt beta=1 accumulate) instead of autograd's
# temp-then-add accumulation. The FSDP FlatUnit attaches
# `weight._flat_grad_view` (a view of the unit's flat bf16 grad buffer)
# and `weight._wgrad_done` (the unit's grad-countdown callback); models
# opt weights in by setting `weight._direct_wgrad = True`. Saves one
# full read+write pass over every projection grad per step (the
# CUDAFunctor_add kernels: ~8.5 ms/step on Llama2-7B, profiles/).
#
# The wgrad dW = dy^T @ x finds both operands strided along the tokens
# (BLAS "NT"), hipBLASLt's slowest class on MI355X. _C.wgrad_tn first
# transposes dy and x with transpose.hip into transient token-contiguous
# copies, and the same product then runs in the forward's class ("TN").
# It pays where the GEMM saves more than the two copy-speed transposes
# cost. Measured (profiles/7b_1gpu_step_wgrad_tn.md): at 8192 tokens the
# 7B block's qkv, gate|up and down projections gain 54-188 us each and
# the square 4096 x 4096 one loses 18 us; at 4096 tokens and below, on
# hipBLASLt's default algorithms, wins and losses are mixed. Hence:
# tokens >= 8192 and a weight of at least 4096 x 8192 elements.
# FMS_AMD_WGRAD=nt keeps every wgrad on the old route.
#
# The dgrad dx = dy @ W finds W strided along the reduction (BLAS "NN"),
# the second slowest class. _C.dgrad_tn transposes W with transpose.hip
# into a transient copy right before its GEMM and runs dy @ WT^T, again
# the forward's class. The copy is made per backward use and freed by
# stream-ordered reuse: no cache, nothing to invalidate when the
# optimizer, a gather or a checkpoint load writes the weight. An earlier
# attempt at this route lost 29 ms/step; it transposed with torch's
# generic w.t().contiguous() kernel per GEMM, several times slower than
# transpose.hip. Measured with transpose.hip
# (profiles/7b_1gpu_step_dgrad_tn.md): at 8192 tokens the whole op
# (transpose + GEMM) gains 17, 37 and 113 us on qkv, gate|up and down, and
# loses 5 us on the square 4096 x 4096 projection, whose 67 MB transpose
# runs at only 2.0 TB/s; at 4096 tokens and below every projection but
# one loses, the transpose being a fixed cost. Hence the wgrad's rule:
# tokens >= 8192 and a weight of at least 4096 x 8192 elements.
# FMS_AMD_DGRAD=nn keeps every dgrad on the old route.
# --------------------------------------------------------------------------
_WGRAD_TN_MIN_TOKENS = 8192
_WGRAD_TN_MIN_WEIGHT = 4096 * 8192   # out * in
_DGRAD_TN_MIN_TOKENS = 8192
_DGRAD_TN_MIN_WEIGHT = 4096 * 8192   # out * in


def _wgrad_mode(dy2, x2):
    """_C.wgrad_tn mode for this wgrad; 0 = plain addmm on the operands
    as they are."""
    if _C is None or os.environ.get("FMS_AMD_WGRAD") == "nt":
        return 0
    if not (dy2.is_cuda and x2.is_cuda and dy2.dtype == torch.bfloat16
            and x2.dtype == torch.bfloat16):
        return 0
    tokens, out = dy2.shape
    inn = x2.shape[1]
    if tokens % 8 or out % 8 or inn % 8:
        return 0
    if tokens < _WGRAD_TN_MIN_TOKENS or out * inn < _WGRAD_TN_MIN_WEIGHT:
        return 0
    for t in (dy2, x2):     # what transpose.hip reads without a copy
        if (t.stride(1) != 1 or t.stride(0) % 8 or t.stride(0) < t.shape[1]
                or t.data_ptr() % 16):
            return 0
    return 3


def _dgrad_mode(dy2, w):
    """True where the dgrad dx = dy2 @ w goes through _C.dgrad_tn; False =
    the plain matmul on the operands as they are."""
    if _C is None or os.environ.get("FMS_AMD_DGRAD") == "nn":
        return False
    if not (dy2.is_cuda and w.is_cuda and dy2.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16 and dy2.dim() == 2 and w.dim() == 2):
        return False
    tokens, out = dy2.shape
    inn = w.shape[1]
    if out != w.shape[0] or out % 8 or inn % 8:
        return False
    if tokens < _DGRAD_TN_MIN_TOKENS or out * inn < _DGRAD_TN_MIN_WEIGHT:
        return False
    if dy2.stride(1) != 1 or dy2.stride(0) < out:   # the GEMM reads it as is
        return False
    # what transpose.hip reads without a copy
    return not (w.stride(1) != 1 or w.stride(0) % 8 or w.stride(0) < inn
                or w.data_ptr() % 16)


class _DirectWgradLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, residual):
        ctx.save_for_backward(x, weight)
        # attribute holders stashed at forward time: saved_tensors can
        # return attr-less re-wrapped tensors (e.g. under AC recompute)
        ctx.gview = weight._flat_grad_view
        ctx.wobj = weight
        ctx.cb = getattr(weight, "_wgrad_done", None)
        ctx.res_shape = residual.shape if residual is not None else None
        x2 = x.reshape(-1, x.shape[-1])
        if residual is not None:
            y = torch.addmm(residual.reshape(x2.shape[0], -1), x2,
                            weight.t())
        else:
            y = x2 @ weight.t()
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        if not ctx.needs_input_grad[0]:
            dx = None
        elif _dgrad_mode(dy2, w):
            dx = _C.dgrad_tn(dy2, w).view(x.shape)
        else:
            dx = (dy2 @ w).view(x.shape)
        # wgrad straight into the flat grad buffer. First touch since
        # zero_grad overwrites (beta=0) so the runtime never has to
        # zero-fill these slices; later touches accumulate (beta=1).
        fresh = getattr(ctx.wobj, "_wgrad_fresh", False)
        mode = _wgrad_mode(dy2, x2)
        if mode:
            _C.wgrad_tn(dy2, x2, ctx.gview, not fresh, mode)
        elif fresh:
            torch.addmm(ctx.gview, dy2.t(), x2, beta=0, out=ctx.gview)
        else:
            ctx.gview.addmm_(dy2.t(), x2)
        if fresh:
            ctx.wobj._wgrad_fresh = False
        if ctx.cb is not None:
            ctx.cb()
        dres = dy.reshape(ctx.res_shape) if ctx.res_shape is not None else None
        return dx, None, dres


def linear_flat(x, weight, residual=None):
    """F.linear (optionally fused with a residual add in the GEMM
    epilogue) that lands the weight grad directly in the sharded
    runtime's flat grad buffer when the weight is attached to one.
    Falls back to plain autograd ops otherwise (plain/unsharded models,
    frozen weights, no-grad inference)."""
    if (getattr(weight, "_flat_grad_view", None) is not None
            and weight.requires_grad and torch.is_grad_enabled()):
        return _DirectWgradLinearFn.apply(x, weight, residual)
    x2 = x.reshape(-1, x.shape[-1])
    if residual is not None:
        y = torch.addmm(residual.reshape(x2.shape[0], -1), x2, weight.t())
    else:
        y = x2 @ weight.t()
    return y.view(*x.shape[:-1], weight.shape[0])


# --------------------------------------------------------------------------
# Causal flash attention (MFMA tiled, GQA)
# --------------------------------------------------------------------------
class DocMask(NamedTuple):
    """Document boundaries of packed rows, two int32 (b, s) tensors that
    describe one mask from either side: query i sees key j iff
    start[b, i] <= j <= i, equivalently j <= i < end[b, j].

    start[b, i] is the position of the first token of i's document
    (0 <= start <= i, non-decreasing); end[b, j] is the start of the next
    document after j's, or s for the last one. Build it once per model
    forward and share it between the layers."""
    start: torch.Tensor
    end: torch.Tensor


def doc_mask_from_starts(doc_start):
    """DocMask from the (b, s) first-position-of-my-document array. Pure
    tensor ops, no host sync; CPU or GPU."""
    b, s = doc_start.shape
    start = doc_start.long()
    pos = torch.arange(s, device=start.device).expand(b, s)
    # position i opens a document iff start[i] == i; end[j] is the first
    # such i > j: a reversed running minimum, shifted by one
    opens = torch.where(start == pos, pos, torch.full_like(pos, s))
    nxt = torch.cat([opens[:, 1:], torch.full_like(pos[:, :1], s)], dim=1)
    end = torch.cummin(nxt.flip(1), dim=1).values.flip(1)
    return DocMask(start.int().contiguous(), end.int().contiguous())


def doc_mask_from_tokens(tokens, eos_token):
    """DocMask of (b, s) token rows packed back to back, every document
    ending in eos_token (the eos belongs to the document it ends):
    start[i] = 1 + max{j < i : tokens[j] == eos}, or 0."""
    b, s = tokens.shape
    pos = torch.arange(s, device=tokens.device).expand(b, s)
    after = torch.where(tokens == eos_token, pos + 1, torch.zeros_like(pos))
    prev = torch.cat([torch.zeros_like(after[:, :1]), after[:, :-1]], dim=1)
    return doc_mask_from_starts(torch.cummax(prev, dim=1).values)


def _pad_doc_mask(doc_mask, s_pad):
    """Pad rows form a document of their own behind the real ones: start =
    s, end = s_pad. Real keys keep end <= s, so pad queries see none."""
    b, s = doc_mask.start.shape
    if s == s_pad:
        return doc_mask.start.contiguous(), doc_mask.end.contiguous()
    start = doc_mask.start.new_full((b, s_pad), s)
    end = doc_mask.end.new_full((b, s_pad), s_pad)
    start[:, :s] = doc_mask.start
    end[:, :s] = doc_mask.end
    return start, end


class _FlashAttnFn(torch.autograd.Function):
    """Kernel operates on seq multiples of 128; arbitrary lengths are
    zero-padded at the END (causality keeps pad keys invisible to real
    queries) and sliced back. With doc_start/doc_end (a DocMask's two
    arrays, already padded) the document-masked kernels run."""

    @staticmethod
    def _pad(t, s_pad):
        b, s, h, d = t.shape
        if s == s_pad:
            return t.contiguous()
        out = torch.zeros(b, s_pad, h, d, dtype=t.dtype, device=t.device)
        out[:, :s] = t
        return out

    @staticmethod
    def forward(ctx, q, k, v, doc_start=None, doc_end=None):
        ext = _require_ext("attention")
        s = q.shape[1]
        s_pad = (s + 127) // 128 * 128
        qp = _FlashAttnFn._pad(q, s_pad)
        kp = _FlashAttnFn._pad(k, s_pad)
        vp = _FlashAttnFn._pad(v, s_pad)
        if doc_start is None:
            o, lse = ext.attn_fwd(qp, kp, vp)
            ctx.save_for_backward(qp, kp, vp, o, lse)
        else:
            o, lse = ext.attn_fwd_doc(qp, kp, vp, doc_start)
            ctx.save_for_backward(qp, kp, vp, o, lse, doc_start, doc_end)
        ctx.s = s
        return o[:, :s] if s != s_pad else o

    @staticmethod
    def backward(ctx, do):
        qp, kp, vp, o, lse, *doc = ctx.saved_tensors
        s, s_pad = ctx.s, qp.shape[1]
        dop = _FlashAttnFn._pad(do, s_pad)
        if doc:
            dq, dk, dv = _C.attn_bwd_doc(dop, qp, kp, vp, o, lse, None, *doc)
        else:
            dq, dk, dv = _C.attn_bwd(dop, qp, kp, vp, o, lse, None)
        if s != s_pad:
            dq, dk, dv = dq[:, :s], dk[:, :s], dv[:, :s]
        return dq, dk, dv, None, None


class _QKVRopeAttnFn(torch.autograd.Function):
    """Fused qkv-split + RoPE + causal flash attention over the FUSED qkv
    projection (b, s, (h+2kv)*d).

    Removes the per-layer copy traffic the modular path pays: q/k are
    rotated straight out of their strided qkv slices (strided rope
    reads), v feeds the attention kernels as a strided view (vstride
    plumbed into the HIP kernels), and the backward writes dq/dk/dv into
    ONE preallocated fused dqkv buffer — no autograd `cat` of the split,
    no zero-fill, no `.contiguous()` copies. Replaces the reference's
    separate rope+SDPA calls (fms MultiHeadAttention).
    """

    @staticmethod
    def forward(ctx, qkv, cos, sin, nheads, kvheads, head_dim,
                doc_start=None, doc_end=None):
        ext = _require_ext("attention")
        b, s, _ = qkv.shape
        d = head_dim
        hq, hk = nheads * d, kvheads * d
        q = qkv[..., :hq].view(b, s, nheads, d)
        k = qkv[..., hq:hq + hk].view(b, s, kvheads, d)
        v = qkv[..., hq + hk:].view(b, s, kvheads, d)
        cos = cos.float().contiguous()
        sin = sin.float().contiguous()
        qr, kr = ext.rope_fwd(q, k, cos, sin, False)   # strided reads
        if doc_start is None:
            o, lse = ext.attn_fwd(qr, kr, v)           # strided v
            ctx.save_for_backward(qkv, qr, kr, o, lse, cos, sin)
        else:
            o, lse = ext.attn_fwd_doc(qr, kr, v, doc_start)
            ctx.save_for_backward(qkv, qr, kr, o, lse, cos, sin, doc_start,
                                  doc_end)
        ctx.dims = (nheads, kvheads, d)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, qr, kr, o, lse, cos, sin, *doc = ctx.saved_tensors
        nheads, kvheads, d = ctx.dims
        b, s, _ = qkv.shape
        hq, hk = nheads * d, kvheads * d
        v = qkv[..., hq + hk:].view(b, s, kvheads, d)
        dqkv = torch.empty_like(qkv)
        dq_sl = dqkv[..., :hq].view(b, s, nheads, d)
        dk_sl = dqkv[..., hq:hq + hk].view(b, s, kvheads, d)
        dv_sl = dqkv[..., hq + hk:].view(b, s, kvheads, d)
        # document-masked calls differ in the attention kernels only
        bwd = ((lambda *a: _C.attn_bwd_doc(*a, *doc)) if doc
               else _C.attn_bwd)
        if nheads == kvheads:
            # dv written straight into the fused buffer by the kernel
            dq, dk, _ = bwd(do.contiguous(), qr, kr, v, o, lse, dv_sl)
        else:
            dq, dk, dv = bwd(do.contiguous(), qr, kr, v, o, lse, None)
            dv_sl.copy_(dv)
        # inverse rotation scattered into the fused buffer slices
        _C.rope_into(dq, dq_sl, cos, sin, True)
        _C.rope_into(dk, dk_sl, cos, sin, True)
        return dqkv, None, None, None, None, None, None, None


def qkv_rope_attention(qkv, cos, sin, nheads, kvheads, head_dim,
                       doc_mask=None):
    """Fused GPU path; callers gate on seq%128==0 and head_dim in
    (64, 128) and fall back to the modular split+rope+attention path
    otherwise (decode/KV-cache, odd lengths, CPU). doc_mask (DocMask)
    keeps attention inside each document."""
    doc = () if doc_mask is None else (doc_mask.start.contiguous(),
                                       doc_mask.end.contiguous())
    if qkv.dtype == torch.float16:
        return _QKVRopeAttnFn.apply(qkv.bfloat16(), cos, sin, nheads,
                                    kvheads, head_dim, *doc).half()
    return _QKVRopeAttnFn.apply(qkv, cos, sin, nheads, kvheads, head_dim,
                                *doc)


def attention_causal(q, k, v, doc_mask=None):
    """Causal attention, q (b,s,h,d), k/v (b,s,kvh,d). doc_mask (DocMask)
    additionally keeps every query inside its own document."""
    if q.is_cuda:
        if os.environ.get("FMS_AMD_ALLOW_TORCH_SDPA") == "1":
            if doc_mask is not None:
                return reference.attention_causal(q, k, v, doc_mask)
            import torch.nn.functional as F
            o = F.scaled_dot_product_attention(
                q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                is_causal=True, enable_gqa=(k.shape[2] != q.shape[2]))
            return o.transpose(1, 2)
        if q.dtype == torch.float32:
            return reference.attention_causal(q, k, v, doc_mask)
        doc = () if doc_mask is None else _pad_doc_mask(
            doc_mask, (q.shape[1] + 127) // 128 * 128)
        if q.dtype == torch.float16:
            return _FlashAttnFn.apply(q.bfloat16(), k.bfloat16(),
                                      v.bfloat16(), *doc).half()
        return _FlashAttnFn.apply(q, k, v, *doc)
    return reference.attention_causal(q, k, v, doc_mask)


# --------------------------------------------------------------------------
# KV-cache decode: preallocated in-place cache, fused append, split-KV
# attention for one query position (attn_decode.hip)
# --------------------------------------------------------------------------
class KVCache:
    """Preallocated K/V history of one attention layer: `k` and `v` of
    shape (b, capacity, kvheads, head_dim) and the host int `len`, the
    number of rows in use. The capacity is fixed here; an append past it
    raises and never reallocates. The length is the same for every batch
    row (all generate() needs): per-row lengths are not supported, and
    neither is graph capture, since `len` lives on the host.

    fp16 on a GPU is stored in bf16, the type the kernels compute in."""

    def __init__(self, batch, capacity, kvheads, head_dim, dtype, device):
        device = torch.device(device)
        if dtype == torch.float16 and device.type == "cuda":
            dtype = torch.bfloat16
        self.k = torch.empty(batch, capacity, kvheads, head_dim, dtype=dtype,
                             device=device)
        self.v = torch.empty_like(self.k)
        self.len = 0
        self._cat = {}      # the FMS_AMD_DECODE=sdpa route's grown tensors

    @property
    def capacity(self):
        return self.k.shape[1]


def _decode_no_grad(*tensors):
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(
            "the KV-cache ops have no backward: call them under "
            "torch.no_grad() or with inputs that do not require grad")


def _append_view(t):
    """What kv_append_kernel reads without a copy: (b, s, h, d) with
    contiguous heads, one uniform distance between the (b, s) rows (taken
    from b at s == 1, where a fused-projection slice reports an arbitrary
    s stride) and a row stride and base that keep 16-byte alignment."""
    b, s, h, d = t.shape
    rs = t.stride(1) if s > 1 else (t.stride(0) if b > 1 else h * d)
    ok = (t.stride(3) == 1 and t.stride(2) == d and rs >= h * d
          and (s == 1 or b == 1 or t.stride(0) == s * rs)
          and rs % 8 == 0 and t.data_ptr() % 16 == 0)
    return t if ok else t.contiguous()


def kv_cache_append(cache, q, k, v, cos=None, sin=None):
    """Append s positions to the cache in place: q (b,s,h,d), k/v
    (b,s,kvh,d), all three possibly last-dim slices of the fused qkv
    projection. With cos/sin (the table rows of positions [len, len+s)) q
    and k are rotated; rotated k and raw v land in cache rows
    [len, len+s), `len` advances and the rotated q comes back contiguous.
    Without tables (learned positions) it only appends and returns q."""
    _decode_no_grad(q, k, v)
    s = q.shape[1]
    if cache.len + s > cache.capacity:
        raise ValueError(
            f"KVCache overflow: {cache.len} + {s} rows exceed the capacity "
            f"{cache.capacity}")
    if q.is_cuda and q.dtype == torch.float16:
        qr = kv_cache_append(cache, q.bfloat16(), k.bfloat16(), v.bfloat16(),
                             cos, sin)
        return qr.half()
    if q.is_cuda and q.dtype == torch.bfloat16:
        ext = _require_ext("kv_cache_append")
        if cos is not None:
            cos = cos.float().contiguous()
            sin = sin.float().contiguous()
        qr = ext.kv_append(_append_view(q), _append_view(k), _append_view(v),
                           cache.k, cache.v, cache.len, cos, sin)
        if cos is None:
            qr = q
    else:
        qr = reference.kv_cache_append(cache.k, cache.v, cache.len, q, k, v,
                                       cos, sin)
    cache.len += s
    return qr


def attention_decode(q, cache):
    """q (b,1,h,d) attends to cache rows [0, len). The newest key is
    already inside, so there is no causal mask."""
    _decode_no_grad(q)
    if q.shape[1] != 1:
        raise ValueError("attention_decode takes one query position")
    if cache.len < 1:
        raise ValueError("attention_decode on an empty cache")
    if q.is_cuda and q.dtype == torch.float16:
        return attention_decode(q.bfloat16(), cache).half()
    if q.is_cuda and q.dtype == torch.bfloat16:
        if os.environ.get("FMS_AMD_ALLOW_TORCH_SDPA") == "1":
            import torch.nn.functional as F
            n = cache.len
            o = F.scaled_dot_product_attention(
                q.transpose(1, 2), cache.k[:, :n].transpose(1, 2),
                cache.v[:, :n].transpose(1, 2),
                enable_gqa=(cache.k.shape[2] != q.shape[2]))
            return o.transpose(1, 2)
        ext = _require_ext("attention_decode")
        o, _ = ext.attn_decode(q.contiguous(), cache.k, cache.v, cache.len, 0)
        return o
    return reference.attention_decode(q, cache.k, cache.v, cache.len)


def _attention_cached_sdpa(q, k, v, cache, cos, sin):
    """FMS_AMD_DECODE=sdpa: the former route (rope, torch.cat-grown K/V,
    torch SDPA), kept for same-process A/B against the kernels."""
    import torch.nn.functional as F
    if cos is not None:
        q, k = rope_apply(q, k, cos, sin)
    if cache._cat.get("k") is not None:
        k = torch.cat([cache._cat["k"], k], dim=1)
        v = torch.cat([cache._cat["v"], v], dim=1)
    cache._cat["k"], cache._cat["v"] = k, v
    cache.len = k.shape[1]
    o = F.scaled_dot_product_attention(
        q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
        is_causal=(q.shape[1] == k.shape[1]),
        enable_gqa=(k.shape[2] != q.shape[2]))
    return o.transpose(1, 2)


def attention_cached(q, k, v, cache, cos=None, sin=None):
    """Attention of s new positions over a KVCache: append (with RoPE when
    tables are given), then
      - prefill (the cache was empty): attention_causal on views of the
        cache rows just written;
      - s == 1: attention_decode;
      - s > 1 on a non-empty cache (chunked prefill): the fp32 reference
        with the causal mask aligned bottom right. Rare; correct, not
        fast.
    No backward (inference only)."""
    _decode_no_grad(q, k, v)
    if os.environ.get("FMS_AMD_DECODE") == "sdpa":
        return _attention_cached_sdpa(q, k, v, cache, cos, sin)
    if q.is_cuda and q.dtype == torch.float16:
        return attention_cached(q.bfloat16(), k.bfloat16(), v.bfloat16(),
                                cache, cos, sin).half()
    was_empty = cache.len == 0
    s = q.shape[1]
    qr = kv_cache_append(cache, q, k, v, cos, sin)
    if s == 1:
        return attention_decode(qr, cache)
    n = cache.len
    if was_empty:
        kc, vc = cache.k[:, :n], cache.v[:, :n]
        if kc.shape[0] == 1:
            # a batch of one counts as contiguous whatever its batch
            # stride, so no copy is made, yet it reports the capacity's
            # stride, which the kernel's view check refuses: rebuild the
            # batch dim with the stride of n rows
            kc, vc = kc[0].unsqueeze(0), vc[0].unsqueeze(0)
        return attention_causal(qr, kc, vc)
    return reference.attention_cached(qr, cache.k[:, :n], cache.v[:, :n])


def attn_bwd_workspace_limit(mb=None):
    """Get/set the largest dS workspace (MiB) the attention backward may
    allocate; larger shapes run the O(s)-memory recompute path. 0 = never
    use the workspace, None = query. Returns the previous value in MiB, or
    None (and does nothing) without the extension or without a GPU."""
    if _C is None or not torch.cuda.is_available():
        return None
    prev = _C.attn_bwd_ws_limit(None if mb is None else int(mb) << 20)
    return prev >> 20


# --------------------------------------------------------------------------
# SwiGLU epilogue: silu(g) * u over fused (..., 2H) gate|up
# --------------------------------------------------------------------------
class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ext = _require_ext("swiglu")
        gu = gu.contiguous()
        h = ext.swiglu_fwd(gu.view(-1, gu.shape[-1]))
        ctx.save_for_backward(gu)
        return h.view(*gu.shape[:-1], gu.shape[-1] // 2)

    @staticmethod
    def backward(ctx, dy):
        (gu,) = ctx.saved_tensors
        dgu = _C.swiglu_bwd(dy.contiguous().view(-1, dy.shape[-1]),
                            gu.view(-1, gu.shape[-1]))
        return dgu.view(gu.shape)


def swiglu(gu):
    if gu.is_cuda and gu.dtype != torch.float32:
        if gu.dtype == torch.float16:
            return _SwiGLUFn.apply(gu.bfloat16()).half()
        return _SwiGLUFn.apply(gu)
    return reference.swiglu(gu)


# --------------------------------------------------------------------------
# Fused linear + chunked cross-entropy (never materializes full fp32 logits)
# --------------------------------------------------------------------------
class _LinearCEFn(torch.autograd.Function):
    """Computes mean CE of linear(x, W) vs labels, chunked over rows.

    Forward also produces dx and dW (scaled for grad_output=1); backward
    rescales. This trades one saved dx/dW pair for never holding the
    (b*s, V) fp32 softmax (SURVEY.md hard-part 6: llama3 V=128256 logits
    would be ~8 GB fp32 at b2 s8192).
    """

    # rows per chunk: 8192 x 128256 bf16 logits = 2.1 GB transient — easily
    # afforded by 288 GB HBM, and the lm-head GEMMs run at full M
    CHUNK = 8192

    @staticmethod
    def forward(ctx, x, weight, labels, ignore_index):
        ext = _require_ext("cross_entropy")
        e = x.shape[-1]
        x2d = x.contiguous().view(-1, e)
        lab = labels.contiguous().view(-1)
        n = x2d.shape[0]
        dx = torch.empty_like(x2d)
        dw = torch.zeros_like(weight, dtype=torch.float32)
        loss_sum = torch.zeros((), device=x.device, dtype=torch.float32)
        count = (lab != ignore_index).sum()
        denom = count.clamp(min=1).float()

        for i in range(0, n, _LinearCEFn.CHUNK):
            xc = x2d[i:i + _LinearCEFn.CHUNK]
            lc = lab[i:i + _LinearCEFn.CHUNK]
            logits = torch.mm(xc, weight.t())          # hipBLASLt GEMM, bf16
            # in-place: logits -> dlogits (softmax - onehot)/denom, adds loss
            ext.ce_fwd_bwd(logits, lc, loss_sum, denom, ignore_index)
            torch.mm(logits, weight, out=dx[i:i + _LinearCEFn.CHUNK])
            dw.add_(torch.mm(logits.t(), xc).float())
        ctx.save_for_backward(dx, dw)
        ctx.xshape = x.shape
        ctx.wdtype = weight.dtype
        return loss_sum / denom

    @staticmethod
    def backward(ctx, gout):
        dx, dw = ctx.saved_tensors
        return (dx.view(ctx.xshape) * gout, (dw * gout).to(ctx.wdtype),
                None, None)


def linear_cross_entropy(x, weight, labels, ignore_index=-100):
    if x.is_cuda and x.dtype != torch.float32:
        if x.dtype == torch.float16:
            return _LinearCEFn.apply(x.bfloat16(), weight.bfloat16(),
                                     labels, ignore_index)
        return _LinearCEFn.apply(x, weight, labels, ignore_index)
    return reference.linear_cross_entropy(x, weight, labels, ignore_index)


# --------------------------------------------------------------------------
# Fused causal depthwise conv1d + silu (mamba xBC conv)
# --------------------------------------------------------------------------
class _CausalConv1dFn(torch.autograd.Function):
    """With doc_start/doc_end (a DocMask's two arrays) the conv restarts
    at every document of a packed row: the masked kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, doc_start=None, doc_end=None):
        ext = _require_ext("causal_conv1d")
        x = x.contiguous()
        wb = weight.contiguous().bfloat16()
        bf = bias.float().contiguous()
        if doc_start is None:
            y = ext.cconv_fwd(x, wb, bf)
            ctx.save_for_backward(x, wb, bf)
        else:
            y = ext.cconv_fwd_doc(x, wb, bf, doc_start)
            ctx.save_for_backward(x, wb, bf, doc_start, doc_end)
        ctx.wdtype = weight.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wb, bf, *doc = ctx.saved_tensors
        if doc:
            dx, dw, db = _C.cconv_bwd_doc(dy.contiguous(), x, wb, bf, *doc)
        else:
            dx, dw, db = _C.cconv_bwd(dy.contiguous(), x, wb, bf)
        return dx, dw.to(ctx.wdtype), db.to(ctx.wdtype), None, None


def _doc_arrays(doc_mask):
    """() for no mask, else the DocMask's contiguous (start, end)."""
    if doc_mask is None:
        return ()
    return doc_mask.start.contiguous(), doc_mask.end.contiguous()


def causal_conv1d(x, weight, bias, doc_mask=None):
    """x (b, l, C). doc_mask (DocMask): a token's window stops at the
    first token of its document instead of reaching into the previous
    one."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        return _CausalConv1dFn.apply(x, weight, bias, *_doc_arrays(doc_mask))
    return reference.causal_conv1d(x, weight, bias, doc_mask)


# --------------------------------------------------------------------------
# Mamba2 recurrent decode: per-layer state cache, conv update and SSD step
# (causal_conv1d.hip cconv_update_kernel, ssd_step.hip). Inference only.
# --------------------------------------------------------------------------
class MambaCache:
    """Recurrent state of one Mamba2 layer: `conv` (b, d_conv-1, conv_dim),
    the last d_conv-1 raw conv inputs, oldest first, in the activation
    dtype; `ssm` (b, nheads, headdim, d_state) fp32 (mamba_ssm's layout);
    and the host int `len`, the number of tokens consumed. Both start at
    zero, which is a fresh sequence. The size does not depend on the
    length; all batch rows advance together.

    fp16 on a GPU is stored in bf16, the type the kernels compute in."""

    def __init__(self, batch, conv_dim, d_conv, nheads, headdim, d_state,
                 dtype, device):
        device = torch.device(device)
        if dtype == torch.float16 and device.type == "cuda":
            dtype = torch.bfloat16
        self.conv = torch.zeros(batch, d_conv - 1, conv_dim, dtype=dtype,
                                device=device)
        self.ssm = torch.zeros(batch, nheads, headdim, d_state,
                               dtype=torch.float32, device=device)
        self.len = 0


def _step_view(t):
    """What the step kernels read without a copy: (b, T, cols) with a unit
    last stride, one uniform distance between the (b, t) rows (taken from
    b at T == 1, as in _append_view) and a row stride and base that keep
    16-byte alignment."""
    b, T, cols = t.shape
    rs = t.stride(1) if T > 1 else (t.stride(0) if b > 1 else cols)
    ok = (t.stride(2) == 1 and rs >= cols
          and (T == 1 or b == 1 or t.stride(0) == T * rs)
          and rs % 8 == 0 and t.data_ptr() % 16 == 0)
    return t if ok else t.contiguous()


def causal_conv1d_update(conv_state, x, weight, bias):
    """T >= 1 new rows x (b, T, C) of the causal conv behind conv_state
    (b, W-1, C), updated in place: y = silu(conv + bias) over
    [state | x], and the state ends as the last W-1 rows of [state | x].
    On the GPU y equals causal_conv1d on the whole sequence bit for bit.
    No backward (inference only)."""
    _decode_no_grad(x, weight, bias)
    if x.shape[1] < 1:
        raise ValueError("causal_conv1d_update needs at least one row")
    if x.is_cuda and x.dtype == torch.float16:
        return causal_conv1d_update(conv_state, x.bfloat16(), weight,
                                    bias).half()
    if x.is_cuda and x.dtype == torch.bfloat16:
        ext = _require_ext("causal_conv1d_update")
        return ext.cconv_update(conv_state, _step_view(x),
                                weight.detach().contiguous().bfloat16(),
                                bias.detach().float().contiguous())
    return reference.causal_conv1d_update(conv_state, x, weight, bias)


def ssd_state_update(state, x, dt, B, C, z, dt_bias, A_log, D, H, G, P, N):
    """T >= 1 tokens of the SSD recurrence from `state` (b, H, P, N) fp32,
    updated in place (reference.ssd_state_update has the definition).
    x/z (b, T, H*P), B/C (b, T, G*N) and dt (b, T, H) may be last-dim
    slices of the projections; returns the gated out (b, T, H*P).
    No backward (inference only)."""
    _decode_no_grad(x, dt, B, C, z, dt_bias, A_log, D)
    if x.shape[1] < 1:
        raise ValueError("ssd_state_update needs at least one token")
    if x.is_cuda and x.dtype == torch.float16:
        return ssd_state_update(
            state, x.bfloat16(), dt.bfloat16(), B.bfloat16(), C.bfloat16(),
            z.bfloat16(), dt_bias, A_log, D, H, G, P, N).half()
    if x.is_cuda and x.dtype == torch.bfloat16:
        ext = _require_ext("ssd_state_update")
        b, T, _ = dt.shape
        if dt.stride(2) != 1 or (T > 1 and b > 1
                                 and dt.stride(0) != T * dt.stride(1)):
            dt = dt.contiguous()
        return ext.ssd_step(
            state, _step_view(x), dt, _step_view(B), _step_view(C),
            _step_view(z), dt_bias.detach().float().contiguous(),
            A_log.detach().float().contiguous(),
            D.detach().float().contiguous(), H, G, P, N)
    return reference.ssd_state_update(state, x, dt, B, C, z, dt_bias, A_log,
                                      D, H, G, P, N)


# --------------------------------------------------------------------------
# Fused exp(segsum) for the Mamba2 SSD scan: L[n,i,j] = exp(cs_i - cs_j)
# lower-triangular, emitted bf16 in one pass.
# --------------------------------------------------------------------------
class _SegsumExpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cs):
        ext = _require_ext("segsum_exp")
        cs = cs.contiguous()
        L = ext.segsum_exp_fwd(cs)
        ctx.save_for_backward(cs)
        return L

    @staticmethod
    def backward(ctx, gL):
        (cs,) = ctx.saved_tensors
        return _C.segsum_exp_bwd(gL.contiguous().to(torch.bfloat16), cs)


def segsum_exp(cs):
    """cs (..., Q) fp32 cumulative sums -> bf16 (..., Q, Q) decay matrix."""
    if cs.is_cuda:
        return _SegsumExpFn.apply(cs)
    Q = cs.shape[-1]
    out = cs[..., :, None] - cs[..., None, :]
    mask = torch.tril(torch.ones(Q, Q, dtype=torch.bool, device=cs.device), 0)
    return torch.exp(out.masked_fill(~mask, -torch.inf))


# --------------------------------------------------------------------------
# Fused SSD scan pieces (Mamba2): every fp32 elementwise chain around the
# batched GEMMs is a HIP kernel with a custom backward (north-star item:
# hand-written selective-scan; reference reaches mamba_ssm's kernels from
# main_training_mamba.py:8-9,67). GPU-only: the CPU path keeps the plain
# torch ssd_chunked as the numerics oracle.
#
# xdt / scores_decay / ygate take an optional doc_mask (DocMask of the
# (b, l) rows behind the flat b*l dimension): the scan then resets at
# every document start (docs/kernels.md "Document mask"). Its start array
# rides through the autograd functions as a non-differentiable input.
# Tensors that are not on the GPU go to the float64-capable oracles of
# ops/reference.py.
# --------------------------------------------------------------------------
def _doc_start_arg(doc_mask, rows, Q):
    """() for no mask, else (start (b, l) int32 contiguous,) after checking
    that its rows are the `rows` tokens, cut into chunks of Q."""
    if doc_mask is None:
        return ()
    start = doc_mask.start.contiguous()
    if start.numel() != rows or start.shape[-1] % Q:
        raise ValueError(
            f"doc_mask of shape {tuple(start.shape)} does not describe "
            f"{rows} tokens in chunks of {Q}")
    return (start,)



class _SSDPrepFn(torch.autograd.Function):
    """(dt2d strided bf16 (b*l, H), dt_bias, A_log) ->
    dtf (N,Q) fp32, dacs (N,Q) fp32 with N=(b*l/Q)*H, n = bc*H + h:
    dtf = softplus(dt + bias); dacs = chunk-cumsum(dtf * -exp(A_log))."""

    @staticmethod
    def forward(ctx, dt2d, dt_bias, A_log, chunk):
        ext = _require_ext("ssd_prep")
        bias_f = dt_bias.detach().float().contiguous()
        alog_f = A_log.detach().float().contiguous()
        dtf, dacs = ext.ssd_prep_fwd(dt2d, bias_f, alog_f, chunk)
        ctx.save_for_backward(dt2d, bias_f, alog_f)
        ctx.meta = (chunk, dt_bias.dtype, A_log.dtype)
        return dtf, dacs

    @staticmethod
    def backward(ctx, ddtf, ddacs):
        dt2d, bias_f, alog_f = ctx.saved_tensors
        chunk, bdt, adt = ctx.meta
        ddt, dbias, dalog = _C.ssd_prep_bwd(
            ddtf.contiguous(), ddacs.contiguous(), dt2d, bias_f, alog_f,
            chunk)
        return ddt, dbias.to(bdt), dalog.to(adt), None


def ssd_prep(dt2d, dt_bias, A_log, chunk):
    return _SSDPrepFn.apply(dt2d, dt_bias, A_log, chunk)


class _SSDXdtFn(torch.autograd.Function):
    """x2d (b*l, H*P) strided bf16 -> (xdt, xdt_decayed) bf16 contiguous
    in H-MAJOR layout (b,nc,H,Q,P) — bmm-native for y_diag (no einsum
    permute copies); xdt = x*dtf, decayed by exp(dacs_end-dacs)."""

    @staticmethod
    def forward(ctx, x2d, dtf, dacs, H, P, Q, doc_start=None):
        ext = _require_ext("ssd_xdt")
        if doc_start is None:
            xdt, xdtd = ext.ssd_xdt_fwd(x2d, dtf, dacs, H, P, Q)
            ctx.save_for_backward(x2d, dtf, dacs)
        else:
            xdt, xdtd = ext.ssd_xdt_fwd_doc(x2d, dtf, dacs, H, P, Q,
                                            doc_start, doc_start.shape[-1])
            ctx.save_for_backward(x2d, dtf, dacs, doc_start)
        ctx.meta = (H, P, Q)
        return xdt, xdtd

    @staticmethod
    def backward(ctx, dxdt, dxdtd):
        x2d, dtf, dacs, *doc = ctx.saved_tensors
        H, P, Q = ctx.meta
        if doc:
            dx, ddtf, sdec = _C.ssd_xdt_bwd_doc(
                dxdt.contiguous(), dxdtd.contiguous(), x2d, dtf, dacs, H, P,
                Q, doc[0], doc[0].shape[-1])
        else:
            dx, ddtf, sdec = _C.ssd_xdt_bwd(
                dxdt.contiguous(), dxdtd.contiguous(), x2d, dtf, dacs, H, P,
                Q)
        # fold the decay-exponent grads: d/d dacs[q] = -sdec[q], and the
        # end column accumulates all q of its row
        ddacs = sdec.neg()
        ddacs[:, -1] += sdec.sum(-1)
        return dx, ddtf, ddacs, None, None, None, None


def ssd_xdt(x2d, dtf, dacs, H, P, Q, doc_mask=None):
    if not x2d.is_cuda:
        return reference.ssd_xdt(x2d, dtf, dacs, H, P, Q, doc_mask)
    return _SSDXdtFn.apply(x2d, dtf, dacs, H, P, Q,
                           *_doc_start_arg(doc_mask, x2d.shape[0], Q))


class _SSDScoresDecayFn(torch.autograd.Function):
    """sL[n,i,j] = scores[m,i,j] * exp(dacs[n,i]-dacs[n,j]) (j<=i), the
    decay matrix L never materialized. scores per GROUP (M=b*nc*G rows);
    backward returns per-head d_scores summed over each group's heads."""

    @staticmethod
    def forward(ctx, dacs, scores3d, H, G, doc_start=None):
        ext = _require_ext("ssd_sl")
        if doc_start is None:
            sL = ext.ssd_sl_fwd(dacs, scores3d, H, G)
            ctx.save_for_backward(dacs, scores3d)
        else:
            sL = ext.ssd_sl_fwd_doc(dacs, scores3d, H, G, doc_start,
                                    doc_start.shape[-1])
            ctx.save_for_backward(dacs, scores3d, doc_start)
        ctx.meta = (H, G)
        return sL

    @staticmethod
    def backward(ctx, g):
        dacs, scores3d, *doc = ctx.saved_tensors
        H, G = ctx.meta
        if doc:
            dsh, dcs = _C.ssd_sl_bwd_doc(g.contiguous(), scores3d, dacs, H,
                                         G, doc[0], doc[0].shape[-1])
        else:
            dsh, dcs = _C.ssd_sl_bwd(g.contiguous(), scores3d, dacs, H, G)
        rep = H // G
        M = scores3d.shape[0]
        Q = scores3d.shape[1]
        dscores = dsh.view(M // G, G, rep, Q, Q) \
            .sum(dim=2, dtype=torch.float32).to(scores3d.dtype).view(M, Q, Q)
        return dcs, dscores, None, None, None


def ssd_scores_decay(dacs, scores3d, H, G, doc_mask=None):
    if not dacs.is_cuda:
        return reference.ssd_scores_decay(dacs, scores3d, H, G, doc_mask)
    N, Q = dacs.shape
    return _SSDScoresDecayFn.apply(
        dacs, scores3d, H, G, *_doc_start_arg(doc_mask, N // H * Q, Q))


class _SSDYGateFn(torch.autograd.Function):
    """out = (ydiag + yoff*exp(dacs) + x*D) * silu(z), bf16 in one pass
    (y assembly + D residual + the gated epilogue)."""

    @staticmethod
    def forward(ctx, ydiag, yoff, dacs, x2d, D, z2d, H, G, P, Q,
                doc_start=None):
        ext = _require_ext("ssd_ygate")
        D_f = D.detach().float().contiguous()
        if doc_start is None:
            out = ext.ssd_ygate_fwd(ydiag, yoff, dacs, x2d, D_f, z2d, H, G,
                                    P, Q)
            ctx.save_for_backward(ydiag, yoff, dacs, x2d, D_f, z2d)
        else:
            out = ext.ssd_ygate_fwd_doc(ydiag, yoff, dacs, x2d, D_f, z2d, H,
                                        G, P, Q, doc_start,
                                        doc_start.shape[-1])
            ctx.save_for_backward(ydiag, yoff, dacs, x2d, D_f, z2d,
                                  doc_start)
        ctx.meta = (H, G, P, Q, D.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        ydiag, yoff, dacs, x2d, D_f, z2d, *doc = ctx.saved_tensors
        H, G, P, Q, ddt = ctx.meta
        if doc:
            dydiag, dyoff, ddacs, dx, dD_rows, dz = _C.ssd_ygate_bwd_doc(
                dout.contiguous(), ydiag, yoff, dacs, x2d, D_f, z2d, H, G, P,
                Q, doc[0], doc[0].shape[-1])
        else:
            dydiag, dyoff, ddacs, dx, dD_rows, dz = _C.ssd_ygate_bwd(
                dout.contiguous(), ydiag, yoff, dacs, x2d, D_f, z2d, H, G, P,
                Q)
        dD = dD_rows.sum(0)
        return (dydiag, dyoff, ddacs, dx, dD.to(ddt), dz, None, None, None,
                None, None)


def ssd_ygate(ydiag, yoff, dacs, x2d, D, z2d, H, G, P, Q, doc_mask=None):
    """ydiag h-major (b,nc,h,Q,p) flat; yoff in the y_off einsum's
    natural (b,nc,g,Q,rep,p) layout; out (b, l, H*P) row-major."""
    if not x2d.is_cuda:
        return reference.ssd_ygate(ydiag, yoff, dacs, x2d, D, z2d, H, G, P,
                                   Q, doc_mask)
    return _SSDYGateFn.apply(ydiag, yoff, dacs, x2d, D, z2d, H, G, P, Q,
                             *_doc_start_arg(doc_mask, x2d.shape[0], Q))


# --------------------------------------------------------------------------
# Fused AdamW on flat fp32 shards + multi-tensor sq-norm
# --------------------------------------------------------------------------
def fused_adamw(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay,
                grad_scale=None, p_bf16_out=None):
    """In-place AdamW on 1-D fp32 tensors. g may be fp32, bf16 or fp16;
    grad_scale (0-dim fp32 tensor) folds grad clipping (and fp16 loss
    unscaling) into the update; p_bf16_out receives the updated bf16 OR
    fp16 shard in the same pass."""
    if p.is_cuda:
        ext = _require_ext("adamw")
        ext.adamw(p, g.view(-1), m, v, float(step), lr, beta1, beta2, eps,
                  weight_decay, grad_scale,
                  p_bf16_out.view(-1) if p_bf16_out is not None else None)
        return True
    gf = g.float().view(-1)
    if grad_scale is not None:
        gf = gf * grad_scale
    reference.adamw_step(p, gf, m, v, step, lr, beta1, beta2, eps,
                         weight_decay)
    return False


def sq_norm(tensors):
    """Sum of squares over a list of tensors -> fp32 scalar tensor."""
    tensors = [t for t in tensors if t.numel() > 0]
    if tensors and tensors[0].is_cuda and _C is not None:
        out = torch.zeros((), device=tensors[0].device, dtype=torch.float32)
        for t in tensors:
            _C.sq_norm_accum(t.view(-1), out)
        return out
    return sum((t.float().pow(2).sum() for t in tensors),
               torch.zeros((), dtype=torch.float32,
                           device=tensors[0].device if tensors else "cpu"))
