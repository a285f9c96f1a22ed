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
# LayerNorm + scaled embedding add + GELU (the MLPSpeculator's head step)
# --------------------------------------------------------------------------
_SPECULATOR_MODES = ("torch", "fused")
_speculator_mode = None


def speculator_mode(mode=None):
    """Get/set the process-wide route of MLPSpeculator.forward: "torch"
    (default) is its chain of eager elementwise ops, "fused" runs the
    kernels of ops/hip/layernorm.hip where layernorm_act has one. None =
    query. Returns the previous mode; until it is set, FMS_AMD_SPECULATOR
    gives the mode."""
    global _speculator_mode
    prev = _speculator_mode
    if prev is None:
        prev = os.environ.get("FMS_AMD_SPECULATOR") or "torch"
        if prev not in _SPECULATOR_MODES:
            raise ValueError(f"FMS_AMD_SPECULATOR must be one of "
                             f"{_SPECULATOR_MODES}, got {prev!r}")
    if mode is not None:
        if mode not in _SPECULATOR_MODES:
            raise ValueError(f"speculator_mode: mode must be one of "
                             f"{_SPECULATOR_MODES}, got {mode!r}")
        _speculator_mode = mode
    return prev


class _LayerNormActFn(torch.autograd.Function):
    """ln_act_fwd_kernel / ln_act_bwd_kernel over x2d (T, H) and tok (T).
    Saves x, tok, mean and rstd; the backward recomputes the rest. The
    embedding grad is aten's scatter of dz."""

    @staticmethod
    def forward(ctx, x2d, w, b, emb, tok, eps, sx, se, gelu, out_scale):
        ext = _require_ext("layernorm_act")
        y, mean, rstd = ext.ln_act_fwd(x2d, emb, tok, w, b, sx, se, eps, gelu,
                                       out_scale)
        ctx.save_for_backward(x2d, w, b, emb, tok, mean, rstd)
        ctx.consts = (sx, se, gelu, out_scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, w, b, emb, tok, mean, rstd = ctx.saved_tensors
        dx, dz, dw, db = _C.ln_act_bwd(dy.contiguous(), x2d, emb, tok, w, b,
                                       mean, rstd, *ctx.consts)
        demb = None
        if emb is not None and ctx.needs_input_grad[3]:
            demb = torch.ops.aten.embedding_dense_backward(
                dz, tok, emb.shape[0], -1, False)
        return (dx, dw.to(w.dtype), db.to(b.dtype), demb) + (None,) * 6


def layernorm_act_has_kernel(x, w, b, emb=None, tok=None):
    """True where layernorm_act runs layernorm.hip: bf16 x (..., H), w, b
    and emb (V, H) contiguous and 16-byte aligned on one GPU, H a multiple
    of 8 up to 8192, integer tok of x's leading shape on that GPU."""
    if w is None or b is None or (emb is None) != (tok is None):
        return False
    ts = [x, w, b] if emb is None else [x, w, b, emb]
    if not x.is_cuda or x.dim() < 1 or any(
            t.dtype != torch.bfloat16 or t.device != x.device
            or not t.is_contiguous() or t.data_ptr() % 16 for t in ts):
        return False
    H = x.shape[-1]
    if H % 8 or not 8 <= H <= 8192 or x.numel() // H >= 2 ** 31 \
            or w.numel() != H or b.numel() != H:
        return False
    if emb is not None and (
            emb.dim() != 2 or emb.shape[1] != H
            or not 1 <= emb.shape[0] < 2 ** 31
            or tok.dtype not in (torch.int32, torch.int64)
            or tok.device != x.device or tok.shape != x.shape[:-1]):
        return False
    return True


def layernorm_act(x, w, b, eps, emb=None, tok=None, sx=1.0, se=0.0,
                  gelu=False, out_scale=1.0):
    """act(LN(x * sx + emb[tok] * se) * w + b) * out_scale over the last dim
    in x's dtype (reference.layernorm_act has the definition). One kernel
    forward and one backward where layernorm_act_has_kernel; CPU, fp32,
    fp16 and the other shapes run the torch expression in fp32."""
    if layernorm_act_has_kernel(x, w, b, emb, tok):
        H = x.shape[-1]
        tok1d = None if tok is None else tok.reshape(-1).contiguous()
        y = _LayerNormActFn.apply(x.view(-1, H), w, b, emb, tok1d, eps, sx,
                                  se, gelu, out_scale)
        return y.view(x.shape)
    return reference.layernorm_act(
        x.float(), w.float(), b.float(), eps,
        None if emb is None else emb.float(), tok, sx, se, gelu,
        out_scale).to(x.dtype)


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
#
# In the MLP two of those transposes re-read what swiglu's backward has
# just held in registers: dgu for the gate|up wgrad, and h, saved by the
# forward, for the down wgrad. swiglu_mlp (below, after swiglu) is the MLP
# as one autograd function whose backward gets dgu, dgu^T and h^T from one
# kernel (_C.swiglu_bwd_t) and hands the transposed operands to
# _C.wgrad_tn_pre: per layer two launches and 540 MB of traffic less, and
# h is no longer saved. It runs where both wgrads and both dgrads of the
# MLP take the TN routes above; elsewhere the MLP stays the composition
# of linear_flat and swiglu.
# --------------------------------------------------------------------------
_WGRAD_TN_MIN_TOKENS = 8192
_WGRAD_TN_MIN_WEIGHT = 4096 * 8192   # out * in
_DGRAD_TN_MIN_TOKENS = 8192
_DGRAD_TN_MIN_WEIGHT = 4096 * 8192   # out * in


def _transpose_reads(t):
    """What transpose.hip reads without a copy."""
    return not (t.stride(1) != 1 or t.stride(0) % 8
                or t.stride(0) < t.shape[1] or t.data_ptr() % 16)


def _wgrad_tn_shape(tokens, out, inn):
    """The part of _wgrad_mode's rule that the shape decides."""
    if _C is None or os.environ.get("FMS_AMD_WGRAD") == "nt":
        return False
    if tokens % 8 or out % 8 or inn % 8:
        return False
    return (tokens >= _WGRAD_TN_MIN_TOKENS
            and out * inn >= _WGRAD_TN_MIN_WEIGHT)


def _wgrad_mode(dy2, x2):
    """_C.wgrad_tn mode for this wgrad; 0 = plain addmm on the operands
    as they are."""
    if not (dy2.is_cuda and x2.is_cuda and dy2.dtype == torch.bfloat16
            and x2.dtype == torch.bfloat16):
        return 0
    if not _wgrad_tn_shape(dy2.shape[0], dy2.shape[1], x2.shape[1]):
        return 0
    if not (_transpose_reads(dy2) and _transpose_reads(x2)):
        return 0
    return 3


def _dgrad_tn_shape(tokens, out, inn):
    """The part of _dgrad_mode's rule that the shape decides."""
    if _C is None or os.environ.get("FMS_AMD_DGRAD") == "nn":
        return False
    if out % 8 or inn % 8:
        return False
    return (tokens >= _DGRAD_TN_MIN_TOKENS
            and out * inn >= _DGRAD_TN_MIN_WEIGHT)


def _dgrad_mode(dy2, w):
    """True where the dgrad dx = dy2 @ w goes through _C.dgrad_tn; False =
    the plain matmul on the operands as they are."""
    if not (dy2.is_cuda and w.is_cuda and dy2.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16 and dy2.dim() == 2 and w.dim() == 2):
        return False
    tokens, out = dy2.shape
    if out != w.shape[0] or not _dgrad_tn_shape(tokens, out, w.shape[1]):
        return False
    if dy2.stride(1) != 1 or dy2.stride(0) < out:   # the GEMM reads it as is
        return False
    return _transpose_reads(w)


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
      - s > 1 on a non-empty cache (verifying a speculator's n_predict
        proposals in one step, chunked prefill): the causal mask aligned
        bottom right. bf16/fp16 on a GPU with head_dim 64 or 128 and at
        most 64 heads per kv head run attn_decode_mq_kernel, one sweep of
        the cache for all s positions of a kv head; everything else the
        fp32 reference.
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
    if (qr.is_cuda and qr.dtype == torch.bfloat16
            and qr.shape[3] in (64, 128)
            and qr.shape[2] <= 64 * cache.k.shape[2]):
        ext = _require_ext("attention_cached")
        o, _ = ext.attn_decode_mq(qr.contiguous(), cache.k, cache.v, n, 0)
        return o
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
# The SwiGLU MLP, y = swiglu(x @ wg1^T) @ w2^T (+ residual), as one
# autograd function (see the comment block above _DirectWgradLinearFn)
# --------------------------------------------------------------------------
def _mlp_bwd_fused(x2, wg1, w2):
    """True where the backward of the MLP on x2 (tokens, emb) takes the
    fused route: both weights attached to a flat grad buffer, and both
    wgrads and both dgrads on their TN routes. The shapes decide for the
    operands the function makes itself (gu, dh, dgu: contiguous, from the
    allocator); dy is made contiguous in the backward if it is not."""
    if os.environ.get("FMS_AMD_MLP_BWD") == "split":
        return False
    if not (_direct_wgrad_on(wg1) and _direct_wgrad_on(w2)):
        return False
    if not (x2.is_cuda and all(t.dtype == torch.bfloat16 and t.dim() == 2
                               for t in (x2, wg1, w2))):
        return False
    tokens, emb = x2.shape
    hid2, hid = wg1.shape[0], w2.shape[1]
    if wg1.shape[1] != emb or w2.shape[0] != emb or hid2 != 2 * hid:
        return False
    if not (_wgrad_tn_shape(tokens, hid2, emb)
            and _wgrad_tn_shape(tokens, emb, hid)
            and _dgrad_tn_shape(tokens, hid2, emb)
            and _dgrad_tn_shape(tokens, emb, hid)):
        return False
    return all(_transpose_reads(t) for t in (x2, wg1, w2))


class _SwiGLUMLPFn(torch.autograd.Function):
    """The forward is linear_flat -> swiglu -> linear_flat call for call,
    but saves gu alone: the backward's one pass over dh and gu
    (_C.swiglu_bwd_t) recomputes h, and emits it and dgu transposed for the
    wgrads. The flat-grad protocol is _DirectWgradLinearFn's, per weight."""

    @staticmethod
    def forward(ctx, x, wg1, w2, residual):
        # attribute holders stashed at forward time: saved_tensors can
        # return attr-less re-wrapped tensors (e.g. under AC recompute)
        ctx.targets = [(w._flat_grad_view, w, getattr(w, "_wgrad_done", None))
                       for w in (wg1, w2)]
        ctx.res_shape = residual.shape if residual is not None else None
        x2 = x.reshape(-1, x.shape[-1])
        gu = x2 @ wg1.t()
        h = _C.swiglu_fwd(gu)
        if residual is not None:
            y = torch.addmm(residual.reshape(x2.shape[0], -1), h, w2.t())
        else:
            y = h @ w2.t()
        ctx.save_for_backward(x, gu, wg1, w2)
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def _wgrad(target, dy, x, dy_pre):
        """One weight's grad into its flat grad view: first touch since
        zero_grad overwrites, later touches accumulate."""
        gview, wobj, cb = target
        fresh = getattr(wobj, "_wgrad_fresh", False)
        _C.wgrad_tn_pre(dy, x, gview, not fresh, dy_pre, not dy_pre)
        if fresh:
            wobj._wgrad_fresh = False
        if cb is not None:
            cb()

    @staticmethod
    def backward(ctx, dy):
        x, gu, wg1, w2 = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if not _transpose_reads(dy2):
            dy2 = dy2.contiguous()
        dh = _C.dgrad_tn(dy2, w2)
        dgu, dguT, hT = _C.swiglu_bwd_t(dh, gu)
        del dh
        _SwiGLUMLPFn._wgrad(ctx.targets[1], dy2, hT, False)     # down
        del hT
        _SwiGLUMLPFn._wgrad(ctx.targets[0], dguT,               # gate|up
                            x.reshape(-1, x.shape[-1]), True)
        del dguT
        dx = (_C.dgrad_tn(dgu, wg1).view(x.shape)
              if ctx.needs_input_grad[0] else None)
        dres = dy.reshape(ctx.res_shape) if ctx.res_shape is not None else None
        return dx, None, None, dres


def swiglu_mlp(x, wg1, w2, residual=None):
    """swiglu(x @ wg1^T) @ w2^T (+ residual), wg1 the fused gate|up weight
    (2H, emb) and w2 the down weight (emb, H). Where _mlp_bwd_fused holds
    it is one autograd function with a fused backward; everywhere else
    (plain models, frozen weights, small shapes, CPU, FMS_AMD_WGRAD=nt,
    FMS_AMD_DGRAD=nn, FMS_AMD_MLP_BWD=split) the composition below."""
    if _mlp_bwd_fused(x.reshape(-1, x.shape[-1]), wg1, w2):
        return _SwiGLUMLPFn.apply(x, wg1, w2, residual)
    return linear_flat(swiglu(linear_flat(x, wg1)), w2, residual)


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


def _ssd_diag_gemm(C2d, B2d, dacs, xdt, H, G, P, N, Q, doc_mask):
    """y_diag in three launches: per-group scores (hipBLASLt), the fused
    scores*decay kernel, the bmm; sL (bc*H, Q, Q) goes through HBM."""
    bc = C2d.shape[0] // Q
    Cm = C2d.view(bc, Q, G, N)
    Bm = B2d.view(bc, Q, G, N)
    scores = torch.einsum("cqgn,ckgn->cgqk", Cm, Bm).contiguous()
    sL = ssd_scores_decay(dacs, scores.view(bc * G, Q, Q), H, G,
                          doc_mask=doc_mask)
    return torch.bmm(sL, xdt.view(bc * H, Q, P))


_SSD_DIAG_BWD_MODES = ("gemm", "fused")
_ssd_diag_bwd_mode = None


def ssd_diag_backward(mode=None):
    """Get/set the process-wide backward of the fused ssd_diag op: "gemm"
    (default) recomputes the three-launch route, "fused" runs the two-pass
    kernel of ops/hip/ssd_diag_bwd.hip. None = query. Returns the previous
    mode; until it is set, FMS_AMD_SSD_DIAG_BWD gives the mode."""
    global _ssd_diag_bwd_mode
    prev = _ssd_diag_bwd_mode
    if prev is None:
        prev = os.environ.get("FMS_AMD_SSD_DIAG_BWD") or "gemm"
        if prev not in _SSD_DIAG_BWD_MODES:
            raise ValueError(f"FMS_AMD_SSD_DIAG_BWD must be one of "
                             f"{_SSD_DIAG_BWD_MODES}, got {prev!r}")
    if mode is not None:
        if mode not in _SSD_DIAG_BWD_MODES:
            raise ValueError(f"ssd_diag_backward: mode must be one of "
                             f"{_SSD_DIAG_BWD_MODES}, got {mode!r}")
        _ssd_diag_bwd_mode = mode
    return prev


class _SSDDiagFn(torch.autograd.Function):
    """y_diag (bc*H, Q, P) from ops/hip/ssd_diag.hip: scores, decay and the
    second product in one kernel, sL never written. The backward depends on
    ssd_diag_backward(). "gemm" is the three-launch route's own: scores and
    sL are recomputed from the saved inputs, the bmm's two gradients are
    taken as autograd takes them, and dC / dB / ddacs come from that route's
    graph (ssd_sl_bwd, the group sum, the two score GEMMs). "fused" is
    ops/hip/ssd_diag_bwd.hip: nothing quadratic in Q reaches HBM, and dC /
    dB arrive as fp32 partials per head block that are summed here."""

    @staticmethod
    def forward(ctx, C2d, B2d, dacs, xdt, H, G, P, N, Q, doc_mask=None):
        ext = _require_ext("ssd_diag")
        doc = _doc_start_arg(doc_mask, C2d.shape[0], Q)
        if doc:
            y = ext.ssd_diag_fwd_doc(C2d, B2d, dacs, xdt, H, G, P, N, Q,
                                     doc[0], doc[0].shape[-1])
        else:
            y = ext.ssd_diag_fwd(C2d, B2d, dacs, xdt, H, G, P, N, Q)
        ctx.save_for_backward(C2d, B2d, dacs, xdt)
        ctx.meta = (H, G, P, N, Q, doc_mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        C2d, B2d, dacs, xdt = ctx.saved_tensors
        H, G, P, N, Q, doc_mask = ctx.meta
        bc = C2d.shape[0] // Q
        if ssd_diag_backward() == "fused":
            ext = _require_ext("ssd_diag_bwd")
            dy = dy.contiguous()
            doc = _doc_start_arg(doc_mask, C2d.shape[0], Q)
            if doc:
                dCp, dBp, dcs, dxdt = ext.ssd_diag_bwd_doc(
                    dy, C2d, B2d, dacs, xdt, H, G, P, N, Q, doc[0],
                    doc[0].shape[-1])
            else:
                dCp, dBp, dcs, dxdt = ext.ssd_diag_bwd(
                    dy, C2d, B2d, dacs, xdt, H, G, P, N, Q)
            return (dCp.sum(0).to(C2d.dtype), dBp.sum(0).to(B2d.dtype), dcs,
                    dxdt) + (None,) * 6
        with torch.enable_grad():
            Cd = C2d.detach().requires_grad_()
            Bd = B2d.detach().requires_grad_()
            cs = dacs.detach().requires_grad_()
            scores = torch.einsum(
                "cqgn,ckgn->cgqk", Cd.view(bc, Q, G, N),
                Bd.view(bc, Q, G, N)).contiguous()
            sL = ssd_scores_decay(cs, scores.view(bc * G, Q, Q), H, G,
                                  doc_mask=doc_mask)
        x3 = xdt.view(bc * H, Q, P)
        dsL = dy.bmm(x3.transpose(1, 2))
        dxdt = sL.detach().transpose(1, 2).bmm(dy)
        dC, dB, dcs = torch.autograd.grad(sL, (Cd, Bd, cs), dsL)
        return (dC, dB, dcs, dxdt.view_as(xdt)) + (None,) * 6


def _ssd_diag_view(t):
    """A (b*l, G*N) slice as the kernel reads it without a copy (the rule of
    _step_view): unit last stride, row stride a multiple of 8 elements,
    16-byte aligned base."""
    ok = (t.stride(1) == 1 and t.stride(0) >= t.shape[1]
          and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0)
    return t if ok else t.contiguous()


def ssd_diag(C2d, B2d, dacs, xdt, H, G, P, N, Q, doc_mask=None):
    """Intra-chunk term of the SSD, (b*l/Q*H, Q, P) h-major: y[n, i] =
    sum_{j<=i} (C_i . B_j) exp(dacs[n, i] - dacs[n, j]) xdt[n, j]
    (reference.ssd_diag has the definition). C2d/B2d (b*l, G*N) may be
    last-dim slices of the conv output; dacs (n, Q) fp32 from ssd_prep, xdt
    h-major bf16 from ssd_xdt. On the GPU the supported shapes (N and P
    with an instantiation, Q a multiple of 32 up to 256) run the fused
    kernel of ops/hip/ssd_diag.hip; every other shape, and every shape
    under FMS_AMD_SSD_DIAG=gemm, takes the three-launch route. The fused
    kernel's backward is chosen by ssd_diag_backward()."""
    if not dacs.is_cuda:
        return reference.ssd_diag(C2d, B2d, dacs, xdt, H, G, P, N, Q,
                                  doc_mask)
    ext = _require_ext("ssd_diag")
    if os.environ.get("FMS_AMD_SSD_DIAG") == "gemm" \
            or C2d.dtype != torch.bfloat16 \
            or not ext.ssd_diag_has_kernel(N, P, Q):
        return _ssd_diag_gemm(C2d, B2d, dacs, xdt, H, G, P, N, Q, doc_mask)
    return _SSDDiagFn.apply(_ssd_diag_view(C2d), _ssd_diag_view(B2d), dacs,
                            xdt.contiguous(), H, G, P, N, Q, doc_mask)


# --------------------------------------------------------------------------
# Inter-chunk state chain (ops/hip/ssd_state.hip): the chunk states as an
# MFMA kernel, the chunk-to-chunk recurrence as a sequential scan that
# starts from any state.
# --------------------------------------------------------------------------
_SSD_STATE_MODES = ("gemm", "fused")
_ssd_state_mode = None


def ssd_state_chain(mode=None):
    """Get/set the process-wide inter-chunk state chain of the fused scan
    (Mamba2Mixer._scan_fused): "gemm" (default) is the states einsum, the
    (nc x nc) decay matrix and the prev einsum; "fused" runs the kernels
    of ops/hip/ssd_state.hip. A scan from an initial state on the GPU takes
    the kernels whatever the mode. None = query. Returns the previous mode;
    until it is set, FMS_AMD_SSD_STATE gives the mode."""
    global _ssd_state_mode
    prev = _ssd_state_mode
    if prev is None:
        prev = os.environ.get("FMS_AMD_SSD_STATE") or "gemm"
        if prev not in _SSD_STATE_MODES:
            raise ValueError(f"FMS_AMD_SSD_STATE must be one of "
                             f"{_SSD_STATE_MODES}, got {prev!r}")
    if mode is not None:
        if mode not in _SSD_STATE_MODES:
            raise ValueError(f"ssd_state_chain: mode must be one of "
                             f"{_SSD_STATE_MODES}, got {mode!r}")
        _ssd_state_mode = mode
    return prev


def _ssd_chunk_state_gemm(B2d, xdtd, H, G, P, N, Q):
    bc = B2d.shape[0] // Q
    return torch.einsum(
        "ckgn,cgrkp->cgrnp", B2d.reshape(bc, Q, G, N),
        xdtd.reshape(bc, G, H // G, Q, P)).reshape(bc * H, N, P)


_SSD_STATE_BWD_MODES = ("gemm", "fused")
_ssd_state_bwd_mode = None


def ssd_chunk_state_backward(mode=None):
    """Get/set the process-wide backward of the chunk-state kernel: "gemm"
    (default) runs the two einsums autograd runs for the states einsum,
    "fused" runs the kernel of ops/hip/ssd_state_bwd.hip. None = query.
    Returns the previous mode; until it is set, FMS_AMD_SSD_STATE_BWD gives
    the mode."""
    global _ssd_state_bwd_mode
    prev = _ssd_state_bwd_mode
    if prev is None:
        prev = os.environ.get("FMS_AMD_SSD_STATE_BWD") or "gemm"
        if prev not in _SSD_STATE_BWD_MODES:
            raise ValueError(f"FMS_AMD_SSD_STATE_BWD must be one of "
                             f"{_SSD_STATE_BWD_MODES}, got {prev!r}")
    if mode is not None:
        if mode not in _SSD_STATE_BWD_MODES:
            raise ValueError(f"ssd_chunk_state_backward: mode must be one of "
                             f"{_SSD_STATE_BWD_MODES}, got {mode!r}")
        _ssd_state_bwd_mode = mode
    return prev


class _SSDChunkStateFn(torch.autograd.Function):
    """states (bc*H, N, P) from ssd_chunk_state_kernel. The backward depends
    on ssd_chunk_state_backward(). "gemm" is the pair of einsums autograd
    runs for the states einsum: dxdtd from B and dS, dB from xdtd and dS
    summed over the heads of a group. "fused" is ops/hip/ssd_state_bwd.hip:
    both gradients from one staging of a bf16 dS, dB as fp32 partials per
    head block that are summed here."""

    @staticmethod
    def forward(ctx, B2d, xdtd, H, G, P, N, Q):
        ext = _require_ext("ssd_chunk_state")
        S = ext.ssd_chunk_state(B2d, xdtd, H, G, P, N, Q)
        ctx.save_for_backward(B2d, xdtd)
        ctx.meta = (H, G, P, N, Q)
        return S

    @staticmethod
    def backward(ctx, dS):
        B2d, xdtd = ctx.saved_tensors
        H, G, P, N, Q = ctx.meta
        if ssd_chunk_state_backward() == "fused":
            ext = _require_ext("ssd_chunk_state_bwd")
            dBp, dxdtd = ext.ssd_chunk_state_bwd(
                dS.contiguous().to(torch.bfloat16), B2d, xdtd, H, G, P, N, Q)
            return (dBp.sum(0).to(B2d.dtype), dxdtd.view(xdtd.shape),
                    None, None, None, None, None)
        bc = B2d.shape[0] // Q
        rep = H // G
        dS5 = dS.reshape(bc, G, rep, N, P)
        dxdtd = torch.einsum("ckgn,cgrnp->cgrkp", B2d.reshape(bc, Q, G, N),
                             dS5)
        dB = torch.einsum("cgrkp,cgrnp->ckgn",
                          xdtd.view(bc, G, rep, Q, P), dS5)
        return (dB.reshape(bc * Q, G * N), dxdtd.reshape(xdtd.shape),
                None, None, None, None, None)


def ssd_chunk_state(B2d, xdtd, H, G, P, N, Q):
    """Chunk states (b*l/Q*H, N, P): S[m] = B_chunk^T xdtd[m]
    (reference.ssd_chunk_state has the definition). B2d (b*l, G*N) may be a
    last-dim slice of the conv output; xdtd h-major bf16 from ssd_xdt. On
    the GPU the bf16 shapes ssd_diag serves run ssd_chunk_state_kernel;
    CPU tensors, other dtypes and other shapes take the einsum."""
    if xdtd.is_cuda and xdtd.dtype == torch.bfloat16 \
            and B2d.dtype == torch.bfloat16 \
            and _require_ext("ssd_chunk_state").ssd_chunk_state_has_kernel(
                N, P, Q):
        return _SSDChunkStateFn.apply(_ssd_diag_view(B2d), xdtd.contiguous(),
                                      H, G, P, N, Q)
    return _ssd_chunk_state_gemm(B2d, xdtd, H, G, P, N, Q)


_SSD_YOFF_MODES = ("gemm", "fused")
_ssd_yoff_mode = None


def ssd_yoff_mode(mode=None):
    """Get/set the process-wide route of the y_off product of the fused scan
    (ssd_yoff): "gemm" (default) is the einsum on hipBLASLt, "fused" runs
    the kernels of ops/hip/ssd_yoff.hip, forward and backward. None = query.
    Returns the previous mode; until it is set, FMS_AMD_SSD_YOFF gives the
    mode."""
    global _ssd_yoff_mode
    prev = _ssd_yoff_mode
    if prev is None:
        prev = os.environ.get("FMS_AMD_SSD_YOFF") or "gemm"
        if prev not in _SSD_YOFF_MODES:
            raise ValueError(f"FMS_AMD_SSD_YOFF must be one of "
                             f"{_SSD_YOFF_MODES}, got {prev!r}")
    if mode is not None:
        if mode not in _SSD_YOFF_MODES:
            raise ValueError(f"ssd_yoff_mode: mode must be one of "
                             f"{_SSD_YOFF_MODES}, got {mode!r}")
        _ssd_yoff_mode = mode
    return prev


class _SSDYOffFn(torch.autograd.Function):
    """yoff (bc, G, Q, rep, P) from ssd_yoff_fwd_kernel; the backward is
    ssd_yoff_dprev_kernel and ssd_yoff_dC_kernel on a bf16 dyoff, dC as
    fp32 partials per head block that are summed here."""

    @staticmethod
    def forward(ctx, C2d, prev, H, G, P, N, Q):
        ext = _require_ext("ssd_yoff")
        yoff = ext.ssd_yoff_fwd(C2d, prev, H, G, P, N, Q)
        ctx.save_for_backward(C2d, prev)
        ctx.meta = (H, G, P, N, Q)
        return yoff

    @staticmethod
    def backward(ctx, dyoff):
        C2d, prev = ctx.saved_tensors
        need_dC, need_dprev = ctx.needs_input_grad[:2]
        ext = _require_ext("ssd_yoff")
        dCp, dprev = ext.ssd_yoff_bwd(
            dyoff.contiguous().to(torch.bfloat16), C2d, prev, *ctx.meta,
            need_dC=need_dC, need_dprev=need_dprev)
        return (dCp.sum(0).to(C2d.dtype) if need_dC else None,
                dprev.view(prev.shape) if need_dprev else None,
                None, None, None, None, None)


def ssd_yoff(C2d, prev, H, G, P, N, Q, b=1):
    """The y_off product of the SSD before its decay, (bc, G, Q, rep, P) on
    every route: yoff[bc, g, q, r] = C[bc*Q + q, g] . prev[bc*H + g*rep + r]
    (reference.ssd_yoff has the definition), the element order ssd_ygate
    reads as (b*l, H*P). C2d (b*l, G*N) may be a last-dim slice of the conv
    output; prev holds (b*l/Q*H, N, P) states in any shape with that element
    order. Under ssd_yoff_mode() "fused", bf16 GPU tensors of the shapes
    ssd_diag serves run the kernels of ops/hip/ssd_yoff.hip. Every other
    case is the einsum of the scan on views split into `b` sequences (so
    that it issues the same bmm whatever the caller's batch), with its two
    leading dimensions merged; like the einsum's own output the result is
    not necessarily contiguous."""
    if ssd_yoff_mode() == "fused" and prev.is_cuda \
            and prev.dtype == torch.bfloat16 \
            and C2d.dtype == torch.bfloat16 \
            and _require_ext("ssd_yoff").ssd_yoff_has_kernel(N, P, Q):
        return _SSDYOffFn.apply(_ssd_diag_view(C2d), prev.contiguous(),
                                H, G, P, N, Q)
    nc = C2d.shape[0] // (b * Q)
    return torch.einsum("bcqgn,bcgrnp->bcgqrp", C2d.reshape(b, nc, Q, G, N),
                        prev.view(b, nc, G, H // G, N, P)).flatten(0, 1)


_MOE_MODES = ("loop", "fused")
_moe_mode = None


def moe_mode(mode=None):
    """Get/set the process-wide route of the Mixtral MoE MLP: "loop"
    (default) is the per-expert loop of MoEMLP.forward, "fused" runs the
    inference kernels of ops/hip/moe.hip where moe_mlp applies. None = query.
    Returns the previous mode; until it is set, FMS_AMD_MOE gives the mode."""
    global _moe_mode
    prev = _moe_mode
    if prev is None:
        prev = os.environ.get("FMS_AMD_MOE") or "loop"
        if prev not in _MOE_MODES:
            raise ValueError(f"FMS_AMD_MOE must be one of {_MOE_MODES}, "
                             f"got {prev!r}")
    if mode is not None:
        if mode not in _MOE_MODES:
            raise ValueError(f"moe_mode: mode must be one of {_MOE_MODES}, "
                             f"got {mode!r}")
        _moe_mode = mode
    return prev


def moe_mlp(x2d, router_weight, wg1_list, w2_list, top_k):
    """The routed SwiGLU MoE forward of x2d (T, emb) on the kernels of
    ops/hip/moe.hip (reference.moe_mlp has the definition; the routing is
    the top_k of the fp32 softmax of the router logits, renormalised), or
    None where that path does not apply and the caller runs its loop. It
    applies under moe_mode() "fused" to contiguous bf16 GPU tensors with
    emb and H multiples of 64, at most 16 experts of one shape and
    top_k <= min(4, experts), when nothing needs a gradient: there is no
    backward. wg1_list[e] (2H, emb) and w2_list[e] (emb, H) are read in
    place."""
    if moe_mode() != "fused":
        return None
    ws = [router_weight, *wg1_list, *w2_list]
    if not x2d.is_cuda or any(t.dtype != torch.bfloat16 or
                              t.device != x2d.device for t in [x2d, *ws]):
        return None
    if torch.is_grad_enabled() and any(t.requires_grad for t in [x2d, *ws]):
        return None
    nE = len(wg1_list)
    if x2d.dim() != 2 or not 1 <= nE <= 16 or len(w2_list) != nE \
            or not 1 <= top_k <= min(4, nE):
        return None
    T, emb = x2d.shape
    H = w2_list[0].shape[-1]
    # the kernels address in 64 bits; rows and grid sizes are 32-bit counts
    if emb % 64 or H % 64 or T * top_k >= 2 ** 30 \
            or T * top_k * max(emb, H) >= 2 ** 43 \
            or any(w.shape != (2 * H, emb) for w in wg1_list) \
            or any(w.shape != (emb, H) for w in w2_list) \
            or any(not t.is_contiguous() or t.data_ptr() % 16
                   for t in [x2d, *wg1_list, *w2_list]):
        return None
    logits = torch.nn.functional.linear(x2d, router_weight).float()
    return _require_ext("moe_mlp").moe_mlp(x2d, logits, list(wg1_list),
                                           list(w2_list), top_k)


class _SSDStatePassFn(torch.autograd.Function):
    """prev (b*nc*H, N, P) bf16 and the fp32 final state from
    ssd_state_pass_fwd_kernel; the backward is the reverse scan of
    ssd_state_pass_bwd_kernel over the saved bf16 prev. Its per-block
    partials of dG_c are summed here and land in column Q-1 of ddacs."""

    @staticmethod
    def forward(ctx, states, dacs, initial_state, b, H, P, N, Q, want_final,
                doc_start=None):
        ext = _require_ext("ssd_state_pass")
        nc = states.shape[0] // (b * H)
        init = None if initial_state is None \
            else initial_state.detach().float().contiguous()
        if doc_start is None:
            out = ext.ssd_state_pass_fwd(states, dacs, b, nc, H, P, N, Q,
                                         init, want_final)
            ctx.save_for_backward(out[0], dacs)
        else:
            out = ext.ssd_state_pass_fwd_doc(
                states, dacs, b, nc, H, P, N, Q, init, want_final, doc_start,
                doc_start.shape[-1])
            ctx.save_for_backward(out[0], dacs, doc_start)
        ctx.meta = (b, nc, H, P, N, Q,
                    None if initial_state is None else initial_state.dtype)
        if not want_final:
            return out[0], None
        return out[0], out[1]

    @staticmethod
    def backward(ctx, dprev, dfinal):
        prev, dacs, *doc = ctx.saved_tensors
        b, nc, H, P, N, Q, idt = ctx.meta
        want_dinit = idt is not None and ctx.needs_input_grad[2]
        dprev = torch.zeros_like(prev) if dprev is None \
            else dprev.contiguous().to(prev.dtype)
        if dfinal is not None:
            dfinal = dfinal.float().contiguous()
        if doc:
            out = _C.ssd_state_pass_bwd_doc(
                dprev, dfinal, prev, dacs, b, nc, H, P, N, Q, want_dinit,
                doc[0], doc[0].shape[-1])
        else:
            out = _C.ssd_state_pass_bwd(dprev, dfinal, prev, dacs, b, nc, H,
                                        P, N, Q, want_dinit)
        ddacs = torch.zeros_like(dacs)
        ddacs[:, -1] = out[1].sum(0).reshape(-1)
        dinit = out[2].to(idt) if want_dinit else None
        return (out[0], ddacs, dinit) + (None,) * 7


def ssd_state_pass_has_kernel(N, P):
    """Whether the state-pass kernels serve (d_state, headdim): P a
    multiple of 8 and N*P of 512."""
    return _require_ext("ssd_state_pass").ssd_state_pass_has_kernel(N, P)


def ssd_state_pass(states, dacs, b, H, P, N, Q, doc_mask=None,
                   initial_state=None, return_final_state=False):
    """The inter-chunk recurrence over the chunk states (b*nc*H, N, P):
    prev[b, c, h] = the state in front of chunk c, Hc_c = keep_c
    exp(dacs[m, Q-1]) Hc_{c-1} + states[b, c, h], from initial_state
    (b, H, P, N) or zero (reference.ssd_state_pass has the definition).
    Returns prev, with return_final_state also the fp32 (b, H, P, N) state
    behind the last chunk. Gradients reach states, dacs and initial_state.
    initial_state and doc_mask do not combine. bf16 states on the GPU run
    the kernels of ops/hip/ssd_state.hip, and a shape they do not serve
    (ssd_state_pass_has_kernel) raises; CPU tensors and other dtypes run
    the oracle."""
    if doc_mask is not None and initial_state is not None:
        raise ValueError("ssd_state_pass: initial_state and doc_mask do not "
                         "combine")
    if not states.is_cuda or states.dtype != torch.bfloat16:
        return reference.ssd_state_pass(states, dacs, b, H, P, N, Q,
                                        doc_mask, initial_state,
                                        return_final_state)
    prev, final = _SSDStatePassFn.apply(
        states.contiguous(), dacs.contiguous(), initial_state, b, H, P, N, Q,
        return_final_state,
        *_doc_start_arg(doc_mask, states.shape[0] // H * Q, Q))
    return (prev, final) if return_final_state else prev


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
