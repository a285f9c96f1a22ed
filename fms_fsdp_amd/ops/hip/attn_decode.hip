// KV-cache decode attention for CDNA4/gfx950: the fused cache append and
// single-query attention over a preallocated cache, with split-KV.
//
// Cache layout (bf16, contiguous): k and v (b, capacity, kvh, d); rows
// [0, kv_len) are valid, rows behind them are uninitialised memory.
//
//  kv_append_kernel<HAS_ROPE>   split + RoPE + append in one launch:
//      rotated q -> contiguous (b, s, h, d); rotated k and raw v -> cache
//      rows [pos, pos + s). Arithmetic is rope_kernel's (rope.hip).
//  attn_decode_kernel<D>        q (b, 1, h, d) against cache rows
//      [0, kv_len), one workgroup per (batch row, kv head, 32-head column
//      block, split).
//  attn_decode_combine_kernel   merges the splits' fp32 partials in split
//      order and rounds to bf16 once.
#include "common.h"
#include "attn_frag.h"
#include "attn_decode_plan.h"

// ---------------------------------------------------------------------
// Append. One thread moves 4 rotation pairs (two 8-byte loads, two 8-byte
// stores) of one head of one (b, s) row. The row's heads are numbered
// q heads | k heads | v heads; q/k/v are (b, s) row-strided views (slices
// of the fused qkv projection qualify), heads within a row contiguous.
// HAS_ROPE=false (learned positions) copies k and v and leaves q alone.
// ---------------------------------------------------------------------
template <bool HAS_ROPE>
__global__ void kv_append_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ qout,
    short* __restrict__ kcache, short* __restrict__ vcache,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, int s,
    int h, int kvh, int d, long long q_stride, long long k_stride,
    long long v_stride, long long capacity, long long pos,
    long long total4) {
  const int d2 = d / 2;
  const long long idx4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx4 >= total4) return;
  const int g_per_head = d2 / 4;
  const int nvh = (HAS_ROPE ? h : 0) + 2 * kvh;
  const long long head_idx = idx4 / g_per_head;
  const int g = (int)(idx4 % g_per_head);
  const long long row = head_idx / nvh;
  int vh = (int)(head_idx % nvh);
  if (!HAS_ROPE) vh += h;
  const int si = (int)(row % s);
  const long long bi = row / s;
  const long long crow = bi * capacity + pos + si;

  const short* src;
  short* dst;
  bool rot;
  if (vh < h) {
    src = q + row * q_stride + (long long)vh * d;
    dst = qout + (row * h + vh) * d;
    rot = true;
  } else if (vh < h + kvh) {
    src = k + row * k_stride + (long long)(vh - h) * d;
    dst = kcache + (crow * kvh + (vh - h)) * d;
    rot = HAS_ROPE;
  } else {
    src = v + row * v_stride + (long long)(vh - h - kvh) * d;
    dst = vcache + (crow * kvh + (vh - h - kvh)) * d;
    rot = false;
  }
  src += g * 4;
  dst += g * 4;
  const bf16x4 x1 = *(const bf16x4*)(src);
  const bf16x4 x2 = *(const bf16x4*)(src + d2);
  bf16x4 o1 = x1, o2 = x2;
  if (HAS_ROPE && rot) {
    const f32x4 c = *(const f32x4*)(cos_t + (size_t)si * d2 + g * 4);
    const f32x4 sn = *(const f32x4*)(sin_t + (size_t)si * d2 + g * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // rope_kernel's expression, so the bits match _C.rope_fwd
      const float a = bf2f(x1.v[j]);
      const float b = bf2f(x2.v[j]);
      const float sj = sn.v[j];
      o1.v[j] = f2bf(a * c.v[j] - b * sj);
      o2.v[j] = f2bf(b * c.v[j] + a * sj);
    }
  }
  *(bf16x4*)(dst) = o1;
  *(bf16x4*)(dst + d2) = o2;
}

// ---------------------------------------------------------------------
// Decode attention. Swapped layout S^T = K Q^T of the forward kernel: the
// 32 keys of a tile sit on the MFMA rows, the G = h/kvh query heads of
// one kv head on the 32 columns (zero beyond G; 32 < G <= 64 takes a
// second workgroup for heads 32..63), so every lane owns one query head
// and the online softmax is lane-local. The Q fragments stay in
// registers for the whole sweep.
//
// The 4 waves of a workgroup take the 32-key tiles of the split's range
// round-robin, each with its own (m, l, O); no barrier inside the sweep.
// K goes global -> registers (the S^T A-operand is 16 contiguous bytes of
// a key row per lane), V global -> registers -> a wave-private subtiled
// LDS image (attn_frag.h) that the PV A-operand reads transposed. The
// next tile's K and V loads are in flight during the current tile's
// softmax and PV.
//
// Keys >= kv_len: the cache rows behind kv_len are uninitialised and may
// hold NaN or inf. Their rows are never loaded (the row index is clamped
// to kv_len - 1, which also keeps every address inside the batch row),
// their scores are replaced by a select before the max, and their P is
// set to 0 by a select after the exponential, whatever the running max:
// they contribute exactly 0 to l and, with a finite V row in their
// place, exactly 0 to O.
//
// P is rounded to bf16 for the PV mfma only: l sums the fp32 values, so
// lse carries no bf16 rounding and o one of at most 2^-9 per term of its
// numerator. scale*log2e is applied in fp32 to the mfma result; q is not
// pre-scaled.
//
// After the sweep the waves agree on the column maxima through LDS,
// rescale, and add their O in the fixed order (w0 + w2) + (w1 + w3) in
// the LDS the V images occupied. splits == 1: o is normalised and written
// in bf16 with lse. splits > 1: the unnormalised fp32 O and (m, l) go to
// the workspace for attn_decode_combine_kernel.
// ---------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256, 2) void attn_decode_kernel(
    const short* __restrict__ qg, const short* __restrict__ kcg,
    const short* __restrict__ vcg, short* __restrict__ og,
    float* __restrict__ lseg, float* __restrict__ ws_o,
    float* __restrict__ ws_ml, int H, int KVH, int kv_len,
    long long capacity, int splits, int ncb, float scale) {
  constexpr int NC = D / 16;    // QK^T k-chunks = 16-byte V loads per lane
  constexpr int NT = D / 32;    // 32-wide output tiles
  constexpr int KT = ATTN_DECODE_KEY_TILE;
  constexpr int VIMG = KT * D * 2;          // bytes of one wave's V image
  constexpr int CPR = D / 8;                // 16-byte chunks per V row
  constexpr int RPI = 64 / CPR;             // V rows per load instruction
  static_assert(KT == 32 && NC * RPI == KT, "tile shape");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31;
  const int hb = lane >> 5;

  int bid = blockIdx.x;
  const int split = bid % splits;
  bid /= splits;
  const int cb = bid % ncb;
  bid /= ncb;
  const int kvh = bid % KVH;
  const long long b = bid / KVH;

  const int G = H / KVH;
  const int hc = cb * 32 + col;             // head within the group
  const bool valid = hc < G;
  const long long head = (long long)kvh * G + hc;
  const float scale2 = scale * 1.4426950408889634f;

  // Q -> B-fragments: B[k = d][j = head], k = hb*8 + e per 16-wide chunk
  bf16x8v qb[NC];
  {
    const short* qp = qg + (b * H + head) * D + hb * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bf16x8v qv = (bf16x8v)((__bf16)0.f);
      if (valid) qv = *(const bf16x8v*)(qp + c * 16);
      qb[c] = qv;
    }
  }

  // this split's tile range (never empty: splits <= ntile) and the wave's
  // share of it
  const int ntile = (kv_len + KT - 1) / KT;
  const int t_lo = (int)((long long)split * ntile / splits);
  const int t_hi = (int)((long long)(split + 1) * ntile / splits);

  const long long rs = (long long)KVH * D;  // cache row stride
  const long long cbase = (b * capacity * KVH + kvh) * D;
  const short* kbase = kcg + cbase + hb * 8;
  const int vrow0 = lane / CPR;
  const int vcol = (lane % CPR) * 8;
  const short* vbase = vcg + cbase + vcol;
  char* vimg = smem + wid * VIMG;
  int voff[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i)
    voff[i] = SUBT_OFF(i * RPI + vrow0, vcol, KT / 4);
  // transpose-read base of the PV A-operand (R4 = KT/4 = 8 row groups,
  // 1024 B per column block): row-group swizzle, in-subtile lane column,
  // the hb*8 key offset and the 16-lane column block
  const int pvswz = (((lane & 15) * 8) ^ (16 * hb)) + hb * 256 +
                    (col >> 4) * (KT / 4) * 128;

  bf16x8v kn[NC];
  f32x4v vn[NC];
  auto load_tile = [&](int t) {
    const int last = kv_len - 1;
    const long long krow = min(t * KT + col, last);
    const short* kp = kbase + krow * rs;
#pragma unroll
    for (int c = 0; c < NC; ++c) kn[c] = *(const bf16x8v*)(kp + c * 16);
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const long long vrow = min(t * KT + i * RPI + vrow0, last);
      vn[i] = *(const f32x4v*)(vbase + vrow * rs);
    }
  };

  f32x16 accO[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) accO[t] = (f32x16)(0.f);
  float m_run = -1e30f, l_run = 0.f;

  int tile = t_lo + wid;
  if (tile < t_hi) load_tile(tile);
  for (; tile < t_hi; tile += 4) {
    f32x16 accS = (f32x16)(0.f);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kn[c], qb[c], accS, 0,
                                                     0, 0);
    // DS ops of a wave complete in order: the previous tile's transposed
    // reads are done (waited for below), these writes land before the
    // reads that follow
#pragma unroll
    for (int i = 0; i < NC; ++i) *(f32x4v*)(vimg + voff[i]) = vn[i];
    if (tile + 4 < t_hi) load_tile(tile + 4);

    const int key0 = tile * KT;
    const bool partial = key0 + KT > kv_len;   // wave-uniform
    float p[16];
    float mt = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float sv = accS[r] * scale2;
      if (partial && key0 + DROW(r, hb) >= kv_len) sv = -1e30f;
      p[r] = sv;
      mt = fmaxf(mt, sv);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = fmaxf(m_run, mt);
    const float alpha = exp2f(m_run - m_new);
    m_run = m_new;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) accO[t][r] *= alpha;
    float s_own = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float e = exp2f(p[r] - m_run);
      // select, never multiply
      if (partial && key0 + DROW(r, hb) >= kv_len) e = 0.f;
      p[r] = e;
      s_own += e;
    }
    l_run = l_run * alpha + s_own + __shfl_xor(s_own, 32, 64);

    const bf16x8v pb0 = pack_pT_chunk(p);
    const bf16x8v pb1 = pack_pT_chunk(p + 8);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      // column blocks 2t, 2t+1; keys 0..15 then 16..31
      const int o = pvswz + t * 2 * (KT / 4) * 128;
      const TR4 fr = tr_read4(vimg, o, o + 128, o + 512, o + 640);
      accO[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr.a, pb0, accO[t],
                                                        0, 0, 0);
      accO[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr.b, pb1, accO[t],
                                                        0, 0, 0);
    }
  }

  // ---- merge the four waves ----
  float* sm_m = (float*)(smem + 4 * VIMG);    // [4][32]
  float* sm_l = sm_m + 128;                   // [4][32]
  if (hb == 0) {
    sm_m[wid * 32 + col] = m_run;
    sm_l[wid * 32 + col] = l_run;
  }
  __syncthreads();      // also: every wave is done with its V image
  float m_tot = -1e30f;
#pragma unroll
  for (int w = 0; w < 4; ++w) m_tot = fmaxf(m_tot, sm_m[w * 32 + col]);
  float l_tot = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w)     // a wave without tiles has l = 0
    l_tot += sm_l[w * 32 + col] * exp2f(sm_m[w * 32 + col] - m_tot);
  const float f = exp2f(m_run - m_tot);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) accO[t][r] *= f;

  // two buffers of NT*16 slots x 64 lanes fp32 = the four V images
  float* red = (float*)smem;
  constexpr int RED = NT * 16 * 64;
  if (wid >= 2) {
    float* dst = red + (wid - 2) * RED + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(t * 16 + r) * 64] = accO[t][r];
  }
  __syncthreads();
  if (wid < 2) {
    const float* src = red + wid * RED + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) accO[t][r] += src[(t * 16 + r) * 64];
  }
  __syncthreads();
  if (wid == 1) {
    float* dst = red + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(t * 16 + r) * 64] = accO[t][r];
  }
  __syncthreads();
  if (wid != 0 || !valid) return;
  {
    const float* src = red + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) accO[t][r] += src[(t * 16 + r) * 64];
  }

  // ---- epilogue: lane (col, hb), register r holds dv = 32t + DROW(r, hb)
  const long long bh = b * H + head;
  if (splits == 1) {
    const float inv_l = 1.f / l_tot;
    short* op = og + bh * D;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dv0 = t * 32 + 8 * g + 4 * hb;
        bf16x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          w.v[j] = f2bf(accO[t][g * 4 + j] * inv_l);
        *(bf16x4*)(op + dv0) = w;
      }
    }
    if (hb == 0)
      lseg[bh] = (m_tot + __log2f(l_tot)) * 0.6931471805599453f;
  } else {
    float* op = ws_o + (bh * splits + split) * D;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dv0 = t * 32 + 8 * g + 4 * hb;
        f32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w.v[j] = accO[t][g * 4 + j];
        *(f32x4*)(op + dv0) = w;
      }
    }
    if (hb == 0) {
      float* ml = ws_ml + (bh * splits + split) * 2;
      ml[0] = m_tot;
      ml[1] = l_tot;
    }
  }
}

// ---------------------------------------------------------------------
// Combine. One thread per (b, h) and 4 output columns: the splits'
// maxima, then l and O accumulated in split order 0..splits-1, one bf16
// rounding. No atomics: two calls give identical bits.
// ---------------------------------------------------------------------
__global__ void attn_decode_combine_kernel(
    const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
    short* __restrict__ og, float* __restrict__ lseg, int splits, int D,
    long long total4) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total4) return;
  const int d4n = D / 4;
  const long long bh = idx / d4n;
  const int d4 = (int)(idx % d4n);
  const float* ml = ws_ml + bh * splits * 2;
  float m = -1e30f;
  for (int s = 0; s < splits; ++s) m = fmaxf(m, ml[2 * s]);
  float l = 0.f;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* op = ws_o + bh * splits * D + d4 * 4;
  for (int s = 0; s < splits; ++s) {
    const float w = exp2f(ml[2 * s] - m);
    l += ml[2 * s + 1] * w;
    const f32x4 x = *(const f32x4*)(op + (long long)s * D);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += x.v[j] * w;
  }
  const float inv_l = 1.f / l;
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o.v[j] = f2bf(acc[j] * inv_l);
  *(bf16x4*)(og + bh * D + d4 * 4) = o;
  if (d4 == 0) lseg[bh] = (m + __log2f(l)) * 0.6931471805599453f;
}

extern "C" {

void launch_kv_append(const void* q, const void* k, const void* v, void* qout,
                      void* kcache, void* vcache, const float* cos_t,
                      const float* sin_t, int b, int s, int h, int kvh, int d,
                      long long q_stride, long long k_stride,
                      long long v_stride, long long capacity, long long pos,
                      hipStream_t stream) {
  const bool rope = cos_t != nullptr;
  const long long heads = (rope ? h : 0) + 2LL * kvh;
  const long long total4 = (long long)b * s * heads * (d / 2) / 4;
  if (total4 == 0) return;
  const int block = 256;
  const long long grid = (total4 + block - 1) / block;
  if (rope)
    kv_append_kernel<true><<<(int)grid, block, 0, stream>>>(
        (const short*)q, (const short*)k, (const short*)v, (short*)qout,
        (short*)kcache, (short*)vcache, cos_t, sin_t, s, h, kvh, d, q_stride,
        k_stride, v_stride, capacity, pos, total4);
  else
    kv_append_kernel<false><<<(int)grid, block, 0, stream>>>(
        (const short*)q, (const short*)k, (const short*)v, (short*)qout,
        (short*)kcache, (short*)vcache, cos_t, sin_t, s, h, kvh, d, q_stride,
        k_stride, v_stride, capacity, pos, total4);
}

// splits >= 1 and <= the tile count (the binding clamps); ws_o / ws_ml are
// the fp32 workspaces (b*h*splits*d and b*h*splits*2), unused at splits 1.
void launch_attn_decode(const void* q, const void* kcache, const void* vcache,
                        void* o, float* lse, float* ws_o, float* ws_ml, int b,
                        int h, int kvh, int d, int kv_len, long long capacity,
                        int splits, float scale, hipStream_t stream) {
  const int ncb = (h / kvh + 31) / 32;
  const int grid = b * kvh * ncb * splits;
  const size_t lds = (size_t)4 * ATTN_DECODE_KEY_TILE * d * 2 + 1024;
  if (d == 64)
    attn_decode_kernel<64><<<grid, 256, lds, stream>>>(
        (const short*)q, (const short*)kcache, (const short*)vcache,
        (short*)o, lse, ws_o, ws_ml, h, kvh, kv_len, capacity, splits, ncb,
        scale);
  else
    attn_decode_kernel<128><<<grid, 256, lds, stream>>>(
        (const short*)q, (const short*)kcache, (const short*)vcache,
        (short*)o, lse, ws_o, ws_ml, h, kvh, kv_len, capacity, splits, ncb,
        scale);
  if (splits > 1) {
    const long long total4 = (long long)b * h * d / 4;
    const int block = 256;
    attn_decode_combine_kernel<<<(int)((total4 + block - 1) / block), block,
                                 0, stream>>>(ws_o, ws_ml, (short*)o, lse,
                                              splits, d, total4);
  }
}

}  // extern "C"
