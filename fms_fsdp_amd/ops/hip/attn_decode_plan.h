// Split-KV plan of the decode attention (attn_decode.hip).
//
// attn_decode_kernel runs one workgroup per (batch row, kv head, split);
// a split is a contiguous range of 32-key tiles. With b*kvh workgroups
// already covering the CUs (the speculator stage-2 shapes: b96 x kvh 8..32)
// splitting only adds the combine pass, so the plan is 1. A few long rows
// (b1, 16k keys) would otherwise leave most CUs idle: they get enough
// splits to put ATTN_DECODE_WG_PER_CU workgroups on every CU, as long as
// every split keeps at least ATTN_DECODE_MIN_TILES key tiles (below that
// the four waves of a workgroup have nothing to overlap their loads with).
// The two constants are tuning values; the table behind them is in
// docs/performance.md ("Decode attention"): one workgroup per CU was the
// fastest count at b1 kvh8 16k keys (32 splits) and at b8 kvh8 4k keys
// (4 splits), twice that already slower, and splitting the 10 tiles of a
// 320-key row only added time.
//
// Host-only and all-int64_t so the rule is unit-testable with a plain C++
// compiler (tests/test_kv_cache_cpu.py).
#pragma once

#include <cstdint>

#define ATTN_DECODE_KEY_TILE 32
#define ATTN_DECODE_WG_PER_CU 1
#define ATTN_DECODE_MIN_TILES 8

// number of key tiles of kv_len keys
inline int64_t attn_decode_tiles(int64_t kv_len) {
  return (kv_len + ATTN_DECODE_KEY_TILE - 1) / ATTN_DECODE_KEY_TILE;
}

// Split count for b*kvh (batch row, kv head) pairs of kv_len keys on a
// device with n_cu compute units: >= 1, never above the tile count,
// non-decreasing in kv_len.
inline int64_t attn_decode_plan(int64_t b, int64_t kvh, int64_t kv_len,
                                int64_t n_cu) {
  const int64_t units = b * kvh;
  const int64_t ntile = attn_decode_tiles(kv_len);
  if (units <= 0 || ntile <= 1 || n_cu <= 0) return 1;
  const int64_t want =
      (ATTN_DECODE_WG_PER_CU * n_cu + units - 1) / units;   // ceil
  const int64_t fit = ntile / ATTN_DECODE_MIN_TILES;
  int64_t splits = want < fit ? want : fit;
  if (splits < 1) splits = 1;
  return splits;
}

// a forced or planned count clamped so that no split is empty
inline int64_t attn_decode_clamp_splits(int64_t splits, int64_t kv_len) {
  const int64_t ntile = attn_decode_tiles(kv_len);
  if (splits < 1) return 1;
  return splits < ntile ? splits : ntile;
}
