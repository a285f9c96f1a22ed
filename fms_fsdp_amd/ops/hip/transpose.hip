// bf16 matrix transpose: dst (cols x rows, contiguous) = src^T, src
// (rows x cols) with a row stride >= cols. Feeds the wgrad GEMMs their
// operands token-contiguous and the dgrad GEMMs their weight transposed
// (ops/__init__.py, _DirectWgradLinearFn; _C.wgrad_tn and _C.dgrad_tn), so
// it has to run near copy speed: every global access is a 16-B access
// along a row, of the source on the way in and of the destination on the
// way out, and the 2-byte element shuffle happens in a 64x64 LDS tile.
//
// LDS image: row-major [64][64] bf16 (128-B rows = 8 chunks of 16 B), the
// chunk index XOR-ed with (row / 8) % 8.
//   fill  ds_write_b128, 8 consecutive lanes = one tile row: they cover
//         the row's 128 B whatever the chunk permutation, conflict-free.
//   drain 8 ds_read_u16 per lane (banked by dword mod 32, per 32-lane
//         half). A half holds 8 lanes per destination row, lane k reading
//         tile rows 8k..8k+7 at one column, and 4 destination rows
//         (columns c..c+3 of one chunk). Unswizzled, the 8 row groups sit
//         on the same 2 banks (rows are 32 dwords: 8-way); with the XOR
//         group k reads chunk (c/8)^k, 8 distinct 4-bank slots, and the 4
//         columns share 2 dwords of a slot: conflict-free.
// Per tile that is 8 ds_write_b128 + 64 ds_read_u16 wave-instructions,
// about 230 LDS cycles against the ~2200 clocks a CU's share of HBM needs
// for the tile's 16 KB.
#include "common.h"

#define TR_TILE 64
#define TR_CHUNKS (TR_TILE / 8)

// vec_dst: rows % 8 == 0, so every 8-element run of a destination row is
// 16-B aligned. Otherwise the drain stores element-wise (correct for any
// rows; neither route takes it: the wgrad's rows are the tokens, a
// multiple of 8 by its rule, the dgrad's are the weight's `out`, which
// _C.dgrad_tn checks).
template <bool vec_dst>
__global__ __launch_bounds__(256) void transpose_bf16_kernel(
    const short* __restrict__ src, short* __restrict__ dst, long long rows,
    long long cols, long long src_stride, long long tiles_c) {
  __shared__ bf16x8 tile[TR_TILE * TR_CHUNKS];
  const int t = threadIdx.x;
  const long long r0 = ((long long)blockIdx.x / tiles_c) * TR_TILE;
  const long long c0 = ((long long)blockIdx.x % tiles_c) * TR_TILE;
  const int sub = t % TR_CHUNKS;   // chunk on the way in, row group out
  const int line = t / TR_CHUNKS;  // 0..31

#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int lr = line + p * 32;
    const long long r = r0 + lr, c = c0 + sub * 8;
    bf16x8 v = {};
    if (r < rows && c < cols)   // cols % 8 == 0: a chunk is all in or out
      v = *(const bf16x8*)(src + r * src_stride + c);
    tile[lr * TR_CHUNKS + (sub ^ ((lr >> 3) & 7))] = v;
  }
  __syncthreads();

  const short* ts = (const short*)tile;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int lc = line + p * 32;            // tile column = dst row
    const long long c = c0 + lc, r = r0 + sub * 8;
    if (c >= cols || r >= rows) continue;
    const int col = ((((lc >> 3) ^ sub) & 7) << 3) + (lc & 7);
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o.v[i] = ts[(sub * 8 + i) * TR_TILE + col];
    short* d = dst + c * rows + r;
    if (vec_dst) {   // rows % 8 == 0 and r % 8 == 0: the run is all inside
      *(bf16x8*)d = o;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (r + i < rows) d[i] = o.v[i];
    }
  }
}

extern "C" {

// src, src_row_stride * 2 B and (when rows % 8 == 0) dst 16-B aligned;
// cols % 8 == 0; src_row_stride >= cols.
void launch_transpose_bf16(const void* src, void* dst, long long rows,
                           long long cols, long long src_row_stride,
                           hipStream_t stream) {
  if (rows <= 0 || cols <= 0) return;
  const long long tiles_c = (cols + TR_TILE - 1) / TR_TILE;
  const long long tiles_r = (rows + TR_TILE - 1) / TR_TILE;
  const unsigned grid = (unsigned)(tiles_r * tiles_c);
  if (rows % 8 == 0)
    transpose_bf16_kernel<true><<<grid, 256, 0, stream>>>(
        (const short*)src, (short*)dst, rows, cols, src_row_stride, tiles_c);
  else
    transpose_bf16_kernel<false><<<grid, 256, 0, stream>>>(
        (const short*)src, (short*)dst, rows, cols, src_row_stride, tiles_c);
  HIP_CHECK_LAUNCH();
}

}  // extern "C"
