// Tile plan of the routed MoE MLP (moe.hip).
//
// The sort places every expert's rows at a multiple of the GEMM row tile BM,
// so a row tile holds rows of one expert only. Two tiles are built:
//   BM = 32   decode: a handful of rows per expert, the op is a stream over
//             the active experts' weights and a wider tile would only pad;
//   BM = 128  prefill: the four waves of a workgroup take 32 rows each and
//             a weight tile is read once per 128 rows.
// The choice depends on T, top_k and the expert count alone (the mean number
// of rows per expert), never on the routing, so the chain reads nothing
// back from the device. MOE_PREFILL_ROWS is a tuning value: from 64 mean
// rows per expert on, two 32-row tiles per expert would stream every weight
// tile twice.
//
// Host-only and all-int64_t so the rule is checkable with a plain C++
// compiler.
#pragma once

#include <cstdint>

#define MOE_MAX_EXPERTS 16
#define MOE_MAX_TOPK 4
#define MOE_BM_DECODE 32
#define MOE_BM_PREFILL 128
#define MOE_PREFILL_ROWS 64

// row tile for T tokens routed to top_k of n_exp experts
inline int64_t moe_plan_bm(int64_t T, int64_t top_k, int64_t n_exp) {
  if (n_exp <= 0) return MOE_BM_DECODE;
  return T * top_k >= MOE_PREFILL_ROWS * n_exp ? MOE_BM_PREFILL
                                               : MOE_BM_DECODE;
}

// Static upper bound of the row tiles of `pairs` (token, slot) pairs: every
// expert's segment is rounded up to a whole tile, which adds less than one
// tile per expert. The GEMM grids are launched at this bound.
inline int64_t moe_plan_tiles(int64_t pairs, int64_t bm, int64_t n_exp) {
  return (pairs + bm - 1) / bm + n_exp;
}
