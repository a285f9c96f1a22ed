// The 64x64 bf16 LDS tile of the transposing kernels (transpose.hip,
// swiglu.hip): filled with 16-B chunks along the source rows, drained
// with 16-B runs along the source columns.
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
//
// A 256-thread block covers the tile in two passes of 32 lines; thread t
// has sub = t % 8 (chunk on the way in, row group on the way out) and
// line = t / 8 (+ 32 in the second pass).
#pragma once

#include "common.h"

#define TR_TILE 64
#define TR_CHUNKS (TR_TILE / 8)

// chunk `chunk` (elements 8*chunk..8*chunk+7) of tile row `row`
__device__ __forceinline__ void tr_tile_put(bf16x8* tile, int row, int chunk,
                                            bf16x8 v) {
  tile[row * TR_CHUNKS + (chunk ^ ((row >> 3) & 7))] = v;
}

// tile rows 8*group..8*group+7 at tile column `col`: one 16-B run of
// destination row `col`
__device__ __forceinline__ bf16x8 tr_tile_take(const bf16x8* tile, int col,
                                               int group) {
  const short* ts = (const short*)tile;
  const int c = ((((col >> 3) ^ group) & 7) << 3) + (col & 7);
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o.v[i] = ts[(group * 8 + i) * TR_TILE + c];
  return o;
}
