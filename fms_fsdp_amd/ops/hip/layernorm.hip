// LayerNorm with a fused prologue and epilogue, forward and backward: the
// MLPSpeculator's head step and its input norm in one read and one write
// (models/speculator.py). Per row t of x (T, H) bf16:
//   v  = x[t] * sx + (HAS_EMB ? emb[clamp(tok[t], 0, V-1)] * se : 0)
//   mu = mean(v);  rstd = rsqrt(mean((v - mu)^2) + eps)
//   n  = (v - mu) * rstd * w + b
//   y  = (ACT_GELU ? n * Phi(n) : n) * out_scale       Phi: exact erf form
// v lives in fp32 registers only and y is rounded to bf16 once.
//
// Ownership as in rmsnorm_bwd_fused_kernel: 256 threads, a thread always owns
// the column chunks threadIdx.x + k*256 (k < NC) of 8 bf16, so w, b and the
// backward's dw/db partials stay in registers while the block walks rows with
// a grid stride. H <= NC*2048, H % 8 == 0, threads past H/8 are masked. Every
// global access of a lane is 16 bytes; the embedding row is gathered by the
// same lanes. Rows and element offsets are 64-bit.
#include "common.h"

#define LN_THREADS 256
#define LN_WAVES (LN_THREADS / WAVE)
#define LN_RSQRT2 0.70710678118654752f
#define LN_RSQRT2PI 0.39894228040143268f

// Block sum over the 4 waves in a fixed order, valid on every thread. `s`
// is read after the barrier only; the caller alternates buffers so that the
// next reduction's writes cannot overtake a slow wave's reads.
__device__ __forceinline__ float ln_block_sum(float x, float* s) {
  x = wave_reduce_sum(x);
  if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = x;
  __syncthreads();
  return (s[0] + s[1]) + (s[2] + s[3]);
}

__device__ __forceinline__ long long ln_token(const void* tok, int tok64,
                                              long long row, int V) {
  const long long t = tok64 ? ((const long long*)tok)[row]
                            : (long long)((const int*)tok)[row];
  return t < 0 ? 0 : (t >= V ? V - 1 : t);
}

// The chunks of one row this thread owns: x and, with HAS_EMB, the token's
// embedding row.
template <int NC, bool HAS_EMB>
__device__ __forceinline__ void ln_load_row(
    const bf16x8* __restrict__ x, const bf16x8* __restrict__ emb,
    const void* __restrict__ tok, int tok64, long long row, int H8, int V,
    bf16x8* xv, bf16x8* ev) {
  const bf16x8* xr = x + row * H8;
  const bf16x8* er = nullptr;
  if (HAS_EMB) er = emb + ln_token(tok, tok64, row, V) * H8;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int i = threadIdx.x + k * LN_THREADS;
    if (i < H8) {
      xv[k] = xr[i];
      if (HAS_EMB) ev[k] = er[i];
    }
  }
}

// ---------------- forward ----------------
// y (T, H) bf16, mean (T), rstd (T) fp32. The variance is the mean of the
// squared centered values taken from registers (no E[v^2] - mu^2). The next
// row's chunks are requested before the current row's two reductions.
template <int NC, bool HAS_EMB, bool ACT_GELU>
__global__ __launch_bounds__(LN_THREADS) void ln_act_fwd_kernel(
    const bf16x8* __restrict__ x, const bf16x8* __restrict__ emb,
    const void* __restrict__ tok, int tok64, const bf16x8* __restrict__ w,
    const bf16x8* __restrict__ b, bf16x8* __restrict__ y,
    float* __restrict__ mean, float* __restrict__ rstd, int H8,
    long long rows, int V, float sx, float se, float eps, float out_scale) {
  __shared__ float red[2][LN_WAVES];
  const float invH = 1.f / (float)(H8 * 8);
  bf16x8 wv[NC], bv[NC], xn[NC], en[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int i = threadIdx.x + k * LN_THREADS;
    if (i < H8) {
      wv[k] = w[i];
      bv[k] = b[i];
    }
  }
  ln_load_row<NC, HAS_EMB>(x, emb, tok, tok64, blockIdx.x, H8, V, xn, en);
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    float v[NC][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const bool on = threadIdx.x + k * LN_THREADS < H8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = 0.f;
        if (on) {
          f = bf2f(xn[k].v[j]) * sx;
          if (HAS_EMB) f += bf2f(en[k].v[j]) * se;
        }
        v[k][j] = f;
        s += f;
      }
    }
    if (row + gridDim.x < rows)
      ln_load_row<NC, HAS_EMB>(x, emb, tok, tok64, row + gridDim.x, H8, V, xn,
                               en);
    const float mu = ln_block_sum(s, red[0]) * invH;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (threadIdx.x + k * LN_THREADS < H8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v[k][j] -= mu;
          q += v[k][j] * v[k][j];
        }
      }
    }
    const float rs = rsqrtf(ln_block_sum(q, red[1]) * invH + eps);
    if (threadIdx.x == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    bf16x8* yr = y + row * H8;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int i = threadIdx.x + k * LN_THREADS;
      if (i < H8) {
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float n = v[k][j] * rs * bf2f(wv[k].v[j]) + bf2f(bv[k].v[j]);
          if (ACT_GELU) n = n * 0.5f * (1.f + erff(n * LN_RSQRT2));
          o.v[j] = f2bf(n * out_scale);
        }
        yr[i] = o;
      }
    }
  }
}

// ---------------- backward ----------------
// Recomputes v, nh = (v - mu) * rstd and n from x, emb[tok], mean and rstd:
//   gn = dy * out_scale * (ACT_GELU ? Phi(n) + n * phi(n) : 1)
//   a  = gn * w
//   dv = rstd * (a - mean(a) - nh * mean(a * nh))     one reduction of a pair
//   dx = sx * dv,  dz = se * dv (HAS_EMB)
//   dw += gn * nh, db += gn        per thread, over the rows of the block
// The block then writes its partials to part[blockIdx.x][2][H] (dw row, db
// row); ln_act_bwd_finalize_kernel adds the blocks up. No atomics and no
// zero-fill: two calls give the same bits.
template <int NC, bool HAS_EMB, bool ACT_GELU>
__global__ __launch_bounds__(LN_THREADS) void ln_act_bwd_kernel(
    const bf16x8* __restrict__ dy, const bf16x8* __restrict__ x,
    const bf16x8* __restrict__ emb, const void* __restrict__ tok, int tok64,
    const bf16x8* __restrict__ w, const bf16x8* __restrict__ b,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    bf16x8* __restrict__ dx, bf16x8* __restrict__ dz,
    float* __restrict__ part, int H8, long long rows, int V, float sx,
    float se, float out_scale) {
  __shared__ float red[2][2][LN_WAVES];
  const int H = H8 * 8;
  const float invH = 1.f / (float)H;
  bf16x8 wv[NC], bv[NC];
  float pw[NC][8], pb[NC][8];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int i = threadIdx.x + k * LN_THREADS;
    if (i < H8) {
      wv[k] = w[i];
      bv[k] = b[i];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) pw[k][j] = pb[k][j] = 0.f;
  }
  int par = 0;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const float mu = mean[row], rs = rstd[row];
    const bf16x8* dyr = dy + row * H8;
    bf16x8 xv[NC], ev[NC];
    ln_load_row<NC, HAS_EMB>(x, emb, tok, tok64, row, H8, V, xv, ev);
    float a[NC][8], nh[NC][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int i = threadIdx.x + k * LN_THREADS;
      if (i < H8) {
        const bf16x8 d = dyr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = bf2f(xv[k].v[j]) * sx;
          if (HAS_EMB) v += bf2f(ev[k].v[j]) * se;
          const float h = (v - mu) * rs;
          const float wf = bf2f(wv[k].v[j]);
          float g = bf2f(d.v[j]) * out_scale;
          if (ACT_GELU) {
            const float n = h * wf + bf2f(bv[k].v[j]);
            g *= 0.5f * (1.f + erff(n * LN_RSQRT2)) +
                 n * LN_RSQRT2PI * __expf(-0.5f * n * n);
          }
          pw[k][j] += g * h;
          pb[k][j] += g;
          a[k][j] = g * wf;
          nh[k][j] = h;
          s1 += a[k][j];
          s2 += a[k][j] * h;
        }
      }
    }
    // both means behind one barrier
    s1 = wave_reduce_sum(s1);
    s2 = wave_reduce_sum(s2);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      red[par][0][threadIdx.x / WAVE] = s1;
      red[par][1][threadIdx.x / WAVE] = s2;
    }
    __syncthreads();
    const float* r1 = red[par][0];
    const float* r2 = red[par][1];
    const float m1 = ((r1[0] + r1[1]) + (r1[2] + r1[3])) * invH;
    const float m2 = ((r2[0] + r2[1]) + (r2[2] + r2[3])) * invH;
    par ^= 1;
    bf16x8* dxr = dx + row * H8;
    bf16x8* dzr = HAS_EMB ? dz + row * H8 : nullptr;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int i = threadIdx.x + k * LN_THREADS;
      if (i < H8) {
        bf16x8 ox, oz;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dv = rs * (a[k][j] - m1 - nh[k][j] * m2);
          ox.v[j] = f2bf(sx * dv);
          if (HAS_EMB) oz.v[j] = f2bf(se * dv);
        }
        dxr[i] = ox;
        if (HAS_EMB) dzr[i] = oz;
      }
    }
  }
  f32x4* prow = (f32x4*)(part + (size_t)blockIdx.x * 2 * H);
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int i = threadIdx.x + k * LN_THREADS;
    if (i < H8) {
      f32x4 lo, hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo.v[j] = pw[k][j];
        hi.v[j] = pw[k][4 + j];
      }
      prow[2 * i] = lo;
      prow[2 * i + 1] = hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo.v[j] = pb[k][j];
        hi.v[j] = pb[k][4 + j];
      }
      prow[2 * H8 + 2 * i] = lo;
      prow[2 * H8 + 2 * i + 1] = hi;
    }
  }
}

// out[c] = sum_g part[g][c] over the 2H columns of a partial row (dw, then
// db), g ascending within a slice, slices ascending: a fixed order. A block
// takes 32 columns x 32 row slices; a lane reads 16 bytes, 8 lanes a
// contiguous 128 bytes of a partial row. C4 = 2H / 4.
#define LN_FIN_LANES 8
#define LN_FIN_SLICES 32
__global__ __launch_bounds__(LN_THREADS) void ln_act_bwd_finalize_kernel(
    const f32x4* __restrict__ part, float* __restrict__ out, int C4,
    int nparts) {
  __shared__ float red[LN_FIN_SLICES][LN_FIN_LANES * 4];
  const int cl = threadIdx.x % LN_FIN_LANES;
  const int sl = threadIdx.x / LN_FIN_LANES;
  const int c = blockIdx.x * LN_FIN_LANES + cl;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < C4) {
#pragma unroll 4
    for (int g = sl; g < nparts; g += LN_FIN_SLICES) {
      const f32x4 p = part[(size_t)g * C4 + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += p.v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[sl][cl * 4 + j] = acc[j];
  __syncthreads();
  const int col = blockIdx.x * LN_FIN_LANES * 4 + threadIdx.x;
  if (threadIdx.x < LN_FIN_LANES * 4 && col < C4 * 4) {
    float sum = red[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < LN_FIN_SLICES; ++i) sum += red[i][threadIdx.x];
    out[col] = sum;
  }
}

// Blocks of both row kernels: rmsnorm_bwd's cap (docs/kernels.md).
#define LN_GRID_CAP 1024

#define LN_NC_SWITCH(CALL)   \
  if (H8 <= 256) {           \
    CALL(1);                 \
  } else if (H8 <= 512) {    \
    CALL(2);                 \
  } else {                   \
    CALL(4);                 \
  }

template <bool HAS_EMB, bool ACT_GELU>
static void ln_act_fwd_nc(const void* x, const void* emb, const void* tok,
                          int tok64, const void* w, const void* b, void* y,
                          float* mean, float* rstd, int rows, int H, int V,
                          float sx, float se, float eps, float out_scale,
                          hipStream_t stream) {
  const int H8 = H / 8;
  const int grid = min(rows, LN_GRID_CAP);
#define LN_FWD(NC)                                                          \
  ln_act_fwd_kernel<NC, HAS_EMB, ACT_GELU><<<grid, LN_THREADS, 0, stream>>>( \
      (const bf16x8*)x, (const bf16x8*)emb, tok, tok64, (const bf16x8*)w,   \
      (const bf16x8*)b, (bf16x8*)y, mean, rstd, H8, (long long)rows, V, sx, \
      se, eps, out_scale)
  LN_NC_SWITCH(LN_FWD)
#undef LN_FWD
}

template <bool HAS_EMB, bool ACT_GELU>
static void ln_act_bwd_nc(const void* dy, const void* x, const void* emb,
                          const void* tok, int tok64, const void* w,
                          const void* b, const float* mean, const float* rstd,
                          void* dx, void* dz, float* part, int nparts,
                          int rows, int H, int V, float sx, float se,
                          float out_scale, hipStream_t stream) {
  const int H8 = H / 8;
#define LN_BWD(NC)                                                            \
  ln_act_bwd_kernel<NC, HAS_EMB, ACT_GELU><<<nparts, LN_THREADS, 0, stream>>>( \
      (const bf16x8*)dy, (const bf16x8*)x, (const bf16x8*)emb, tok, tok64,    \
      (const bf16x8*)w, (const bf16x8*)b, mean, rstd, (bf16x8*)dx,            \
      (bf16x8*)dz, part, H8, (long long)rows, V, sx, se, out_scale)
  LN_NC_SWITCH(LN_BWD)
#undef LN_BWD
}

extern "C" {

// Rows of the [nparts, 2, H] fp32 workspace of the backward (= its grid).
int ln_act_bwd_nparts(int rows) { return min(rows, LN_GRID_CAP); }

// rows >= 1, 8 <= H <= 8192, H % 8 == 0. emb (V, H) and tok (rows; int64 if
// tok64 else int32) are both given or both null.
void launch_ln_act_fwd(const void* x, const void* emb, const void* tok,
                       int tok64, const void* w, const void* b, void* y,
                       float* mean, float* rstd, int rows, int H, int V,
                       float sx, float se, float eps, int gelu,
                       float out_scale, hipStream_t stream) {
#define LN_ARGS \
  x, emb, tok, tok64, w, b, y, mean, rstd, rows, H, V, sx, se, eps, \
      out_scale, stream
  if (emb != nullptr) {
    if (gelu)
      ln_act_fwd_nc<true, true>(LN_ARGS);
    else
      ln_act_fwd_nc<true, false>(LN_ARGS);
  } else {
    if (gelu)
      ln_act_fwd_nc<false, true>(LN_ARGS);
    else
      ln_act_fwd_nc<false, false>(LN_ARGS);
  }
#undef LN_ARGS
}

// part: [nparts, 2, H] fp32 with nparts = ln_act_bwd_nparts(rows); dwdb:
// [2, H] fp32 (dw, db). dz is written only where emb is given.
void launch_ln_act_bwd(const void* dy, const void* x, const void* emb,
                       const void* tok, int tok64, const void* w,
                       const void* b, const float* mean, const float* rstd,
                       void* dx, void* dz, float* part, int nparts,
                       float* dwdb, int rows, int H, int V, float sx,
                       float se, int gelu, float out_scale,
                       hipStream_t stream) {
#define LN_ARGS                                                            \
  dy, x, emb, tok, tok64, w, b, mean, rstd, dx, dz, part, nparts, rows, H, \
      V, sx, se, out_scale, stream
  if (emb != nullptr) {
    if (gelu)
      ln_act_bwd_nc<true, true>(LN_ARGS);
    else
      ln_act_bwd_nc<true, false>(LN_ARGS);
  } else {
    if (gelu)
      ln_act_bwd_nc<false, true>(LN_ARGS);
    else
      ln_act_bwd_nc<false, false>(LN_ARGS);
  }
#undef LN_ARGS
  const int C4 = 2 * H / 4;
  ln_act_bwd_finalize_kernel<<<(C4 + LN_FIN_LANES - 1) / LN_FIN_LANES,
                               LN_THREADS, 0, stream>>>(
      (const f32x4*)part, dwdb, C4, nparts);
}

}  // extern "C"
