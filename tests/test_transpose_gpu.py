"""`_C.transpose_bf16` (transpose.hip) against `src.t().contiguous()`, bit
for bit. A transpose moves values and computes nothing, so equality is
the whole rule. Shapes: one 16-byte chunk; exactly one 64x64 tile; one
row and one chunk past a tile (rows % 8 != 0: the element-wise drain);
several row tiles with cols below a tile; more than one tile both ways
with both edges partial."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [(8, 8), (64, 64), (65, 72), (200, 24), (130, 264)]
SENTINEL = -777.0     # exact in bf16, never drawn by the inputs below


def ext():
    from fms_fsdp_amd import _C
    return _C


def src_of(rows, cols, pad):
    """(rows, cols) of distinct-ish values; with pad, a column slice of a
    (rows, cols + pad) buffer, 8 elements in."""
    torch.manual_seed(rows * 1000 + cols)
    wide = torch.randn(rows, cols + pad, device="cuda:0").to(BF)
    return wide[:, 8:8 + cols] if pad else wide


def transposed_into_sentinel(src):
    """Runs the op into a destination full of SENTINEL: an element the
    kernel leaves unwritten then differs from the reference."""
    rows, cols = src.shape
    out = torch.full((cols, rows), SENTINEL, device=src.device, dtype=BF)
    assert ext().transpose_bf16(src, out).data_ptr() == out.data_ptr()
    return out


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_transpose_contiguous(rows, cols):
    src = src_of(rows, cols, 0)
    out = transposed_into_sentinel(src)
    assert out.shape == (cols, rows) and out.is_contiguous()
    assert torch.equal(out, src.t().contiguous())


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_transpose_row_strided(rows, cols):
    src = src_of(rows, cols, 24)
    assert src.stride(0) == cols + 24 and not src.is_contiguous()
    out = transposed_into_sentinel(src)
    assert torch.equal(out, src.t().contiguous())


def test_transpose_rejects_what_it_cannot_read():
    x = torch.zeros(16, 16, device="cuda:0", dtype=BF)
    with pytest.raises(RuntimeError):
        ext().transpose_bf16(x[:, :12])          # cols % 8
    with pytest.raises(RuntimeError):
        ext().transpose_bf16(x[:, 4:12])         # 8-byte aligned only
    with pytest.raises(RuntimeError):
        ext().transpose_bf16(x.t())              # column stride
    with pytest.raises(RuntimeError):
        ext().transpose_bf16(x.float())
