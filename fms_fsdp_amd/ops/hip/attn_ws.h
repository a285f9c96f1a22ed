// Gate between the two causal-attention backward paths (attention.hip).
//
// The default backward has attn_bwd_dkv_kernel publish every dS tile to a
// bf16 workspace of shape (b*h, s, s) that attn_bwd_dq_kernel consumes:
// 5 gemm chains instead of 7, but memory quadratic in s (2 GiB at b2 h32
// s4096, 64 GiB at b1 h32 s32768). Above a byte limit the bindings pass
// no workspace and the launcher runs the O(s)-memory pair instead
// (non-publishing dkv + attn_bwd_dq_recompute_kernel).
//
// Host-only and all-int64_t so the decision is unit-testable with a plain
// C++ compiler: b*h*s*s*2 reaches 2^31 already at b2 h32 s4096.
#pragma once

#include <cstdint>

// default limit in MiB (4 GiB): the 7B benchmark shape's 2 GiB workspace
// stays on the workspace path
#define ATTN_BWD_WS_DEFAULT_MB 4096

// bytes of the (b*h, s, s) bf16 dS workspace
inline int64_t attn_bwd_ws_bytes(int64_t b, int64_t h, int64_t s) {
  return b * h * s * s * 2;
}

// true: allocate the workspace. The boundary is inclusive; limit 0 never
// uses the workspace.
inline bool attn_bwd_use_workspace(int64_t b, int64_t h, int64_t s,
                                   int64_t limit_bytes) {
  return attn_bwd_ws_bytes(b, h, s) <= limit_bytes;
}
