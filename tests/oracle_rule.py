"""The one comparison rule of the non-attention kernel tests.

Every kernel judged with it is an elementwise chain or an fp32 reduction
that rounds to its output type once, so the allowed error follows from
the arithmetic instead of being tuned:

    |got - ref| <= R * |ref| + A * mag          for EVERY element

ref  the exact result, float64, computed from the same (already rounded)
     inputs the kernel received;
R    one rounding to the output type (2^-8 bf16, 2^-11 fp16, 0 fp32);
mag  float64 sum of the absolute values of the terms ref is a sum of
     (for a reduction: of its summands, scaled as the result is);
A    2^-16 where the output depends on a reduction, 2^-20 for short
     chains without one.

Where a kernel has a second, nameable fp32 effect (a bf16 intermediate,
__expf at a large argument), the caller widens `mag` for that output with
the derived term -- never R or A.

Plain module (not a conftest): the test files import it by name.
"""

import torch

A_REDUCE = 2.0 ** -16
A_CHAIN = 2.0 ** -20

_R = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11,
      torch.float32: 0.0}


def rounding(dtype):
    return _R[dtype]


def widen(mag, term, A=A_REDUCE):
    """mag widened so that A * mag grows by the derived absolute bound
    `term` (float64, same shape)."""
    return mag + term / A


def worst_ratio(got, ref, mag, A, R=None):
    """(ratio, flat index) of the worst err/tol; inf if got is not finite
    or an element with zero allowance is off."""
    assert ref.dtype == torch.float64 and mag.dtype == torch.float64
    R = rounding(got.dtype) if R is None else R
    g = got.detach().double()
    ref, mag = torch.broadcast_tensors(ref.detach(), mag.detach())
    assert g.shape == ref.shape, (tuple(g.shape), tuple(ref.shape))
    err = (g - ref).abs()
    tol = R * ref.abs() + A * mag
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(torch.isfinite(g), ratio,
                        torch.full_like(ratio, float("inf")))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    flat = ratio.reshape(-1)
    i = int(flat.argmax())
    return float(flat[i]), i


def check(name, got, ref, mag, A, R=None):
    """Assert the rule on every element of `got`; prints and returns the
    worst err/tol ratio (the figures in docs/kernels.md are these lines
    from a `pytest -s` run)."""
    ratio, i = worst_ratio(got, ref, mag, A, R)
    idx = tuple(int(v) for v in
                torch.unravel_index(torch.tensor(i), got.shape)) \
        if got.dim() else ()
    print(f"[rule] {name}: worst err/tol = {ratio:.4g} at {idx}")
    if not ratio <= 1.0:
        g = got.detach().double().reshape(-1)[i].item()
        r = torch.broadcast_to(ref, got.shape).reshape(-1)[i].item()
        m = torch.broadcast_to(mag, got.shape).reshape(-1)[i].item()
        raise AssertionError(
            f"{name}: worst err/tol = {ratio:.4g} at index {idx} "
            f"(got {g!r}, ref {r!r}, mag {m!r})")
    return ratio
