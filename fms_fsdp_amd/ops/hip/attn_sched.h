// Workgroup -> (causal tile, batch*head) mapping shared by the three causal
// attention kernels. The kernels launch a 1-D grid of ntile*nbh workgroups
// and call attn_sched_map() on the linear workgroup id. Host+device so the
// mapping is unit-testable with a plain C++ compiler.
//
// A causal workgroup's cost is linear in its tile index (fwd/dq: tile+1 KV
// sweeps; dkv: ntile-tile q sweeps), and the hardware is observed to deal
// workgroups to the 8 XCDs round-robin in linear-id order. Two orders:
//
//   ATTN_SCHED_BALANCED  rank = L / nbh, bh = L % nbh,
//                        tile = heavy_low ? rank : ntile-1-rank
//     every (b,h) copy of the heaviest tile is dispatched first, cost is
//     non-increasing in L, and when nbh % 8 == 0 the XCD group L % 8 equals
//     bh % 8: all 8 groups carry identical work and a (b,h)'s K/V is only
//     ever touched through one XCD's L2.
//   ATTN_SCHED_LEGACY    tile = L % ntile, bh = L / ntile
//     the assignment of the former dim3(ntile, nbh) grid (x fastest).
//
// Both are bijections [0, ntile*nbh) -> [0,ntile) x [0,nbh) for any
// ntile, nbh >= 1.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATTN_SCHED_HD __host__ __device__
#else
#define ATTN_SCHED_HD
#endif

enum { ATTN_SCHED_BALANCED = 0, ATTN_SCHED_LEGACY = 1 };

struct AttnWork {
  int tile;  // causal tile index (q tile for fwd/dq, key block for dkv)
  int bh;    // b * H + h
};

// heavy_low: tile 0 is the heaviest (dkv); otherwise the last tile is
// (fwd, dq). Unsigned arithmetic: one scalar divide per workgroup.
ATTN_SCHED_HD inline AttnWork attn_sched_map(unsigned L, unsigned ntile,
                                             unsigned nbh, int mode,
                                             bool heavy_low) {
  const bool legacy = mode == ATTN_SCHED_LEGACY;
  const unsigned div = legacy ? ntile : nbh;
  const unsigned quo = L / div;
  const unsigned rem = L - quo * div;
  AttnWork w;
  if (legacy) {
    w.tile = (int)rem;
    w.bh = (int)quo;
  } else {
    w.tile = (int)(heavy_low ? quo : ntile - 1 - quo);
    w.bh = (int)rem;
  }
  return w;
}
