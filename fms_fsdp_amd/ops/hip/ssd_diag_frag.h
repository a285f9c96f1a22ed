// Pieces shared by the intra-chunk SSD kernels (ssd_diag.hip,
// ssd_diag_bwd.hip): the staged tile geometry, the split transpose reads and
// the clamped document start.
#pragma once

#include "common.h"
#include "attn_frag.h"

// immediate-offset transpose reads, issue and wait apart (attention.hip)
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void tr_issue4(unsigned base, U2x64& r0,
                                          U2x64& r1) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4 offset:%c5\n\t"
      "ds_read_b64_tr_b16 %1, %4 offset:%c6\n\t"
      "ds_read_b64_tr_b16 %2, %4 offset:%c7\n\t"
      "ds_read_b64_tr_b16 %3, %4 offset:%c8"
      : "=&v"(r0.u[0]), "=&v"(r0.u[1]), "=&v"(r1.u[0]), "=&v"(r1.u[1])
      : "v"(base), "i"(O0), "i"(O1), "i"(O2), "i"(O3)
      : "memory");
}

template <int CNT>
__device__ __forceinline__ void tr_wait(U2x64& r0, U2x64& r1) {
  asm volatile("s_waitcnt lgkmcnt(%c4)"
               : "+v"(r0.u[0]), "+v"(r0.u[1]), "+v"(r1.u[0]), "+v"(r1.u[1])
               : "i"(CNT)
               : "memory");
}

// start of chunk element q's document relative to its chunk (<= q), as in
// ssd.hip: clamped into [0, row position] before it is used
__device__ __forceinline__ int diag_rel_start(const int* __restrict__ start,
                                              long long bc, int q, int Q,
                                              int nc) {
  const int c0 = (int)((unsigned)bc % (unsigned)nc) * Q;
  const int s = start[bc * Q + q];
  return min(max(s, 0), c0 + q) - c0;
}

constexpr int DIAG_KT = 64;        // rows per staged tile
constexpr int DIAG_ROWS = 128;     // chunk rows per workgroup
