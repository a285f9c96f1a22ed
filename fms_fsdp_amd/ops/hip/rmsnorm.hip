// RMSNorm forward/backward — one workgroup per row, wave64 reductions,
// bf16x8 vectorized loads (memory-bound: target HBM roofline).
// Replaces the reference's fms LayerNormParameterized call sites
// (SURVEY.md §2.3 kernel table: RMSNorm fwd/bwd).
#include "common.h"

// ---------------- forward ----------------
// x (N, H) bf16, w (H) bf16 -> y (N, H) bf16, rinv (N) f32
// H assumed % 8 == 0 (true for every llama dim); 256 threads/block.
__global__ void rmsnorm_fwd_kernel(const bf16x8* __restrict__ x,
                                   const bf16x8* __restrict__ w,
                                   bf16x8* __restrict__ y,
                                   float* __restrict__ rinv,
                                   int H8, float eps, int rows) {
  __shared__ float scratch[16];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const bf16x8* xr = x + (size_t)row * H8;
    bf16x8* yr = y + (size_t)row * H8;
    float ss = 0.f;
    for (int i = threadIdx.x; i < H8; i += blockDim.x) {
      bf16x8 v = xr[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf2f(v.v[j]);
        ss += f * f;
      }
    }
    ss = block_reduce_sum(ss, scratch);
    float r = rsqrtf(ss / (H8 * 8) + eps);
    if (threadIdx.x == 0) rinv[row] = r;
    for (int i = threadIdx.x; i < H8; i += blockDim.x) {
      bf16x8 v = xr[i];
      bf16x8 wv = w[i];
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o.v[j] = f2bf(bf2f(v.v[j]) * r * bf2f(wv.v[j]));
      yr[i] = o;
    }
    __syncthreads();  // scratch reuse across row iterations
  }
}

// ---------------- fused residual-add + RMSNorm forward ----------------
// s = x + res;  y = s / rms(s) * w.  Saves the separate elementwise-add
// HBM pass (SURVEY.md §2.3 "fused residual-add variant" / mamba
// fused_add_norm). Emits both y and s (the residual stream).
__global__ void add_rmsnorm_fwd_kernel(const bf16x8* __restrict__ x,
                                       const bf16x8* __restrict__ res,
                                       const bf16x8* __restrict__ w,
                                       bf16x8* __restrict__ y,
                                       bf16x8* __restrict__ s_out,
                                       float* __restrict__ rinv,
                                       int H8, float eps, int rows) {
  __shared__ float scratch[16];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const bf16x8* xr = x + (size_t)row * H8;
    const bf16x8* rr = res + (size_t)row * H8;
    bf16x8* yr = y + (size_t)row * H8;
    bf16x8* sr = s_out + (size_t)row * H8;
    float ss = 0.f;
    for (int i = threadIdx.x; i < H8; i += blockDim.x) {
      const bf16x8 xv = xr[i];
      const bf16x8 rv = rr[i];
      bf16x8 sv;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf2f(xv.v[j]) + bf2f(rv.v[j]);
        sv.v[j] = f2bf(f);
        const float fb = bf2f(sv.v[j]);  // rms of the bf16-rounded sum
        ss += fb * fb;
      }
      sr[i] = sv;
    }
    ss = block_reduce_sum(ss, scratch);
    const float r = rsqrtf(ss / (H8 * 8) + eps);
    if (threadIdx.x == 0) rinv[row] = r;
    for (int i = threadIdx.x; i < H8; i += blockDim.x) {
      const bf16x8 sv = sr[i];
      const bf16x8 wv = w[i];
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o.v[j] = f2bf(bf2f(sv.v[j]) * r * bf2f(wv.v[j]));
      yr[i] = o;
    }
    __syncthreads();
  }
}

// ---------------- backward ----------------
// dx_i = r*w_i*dy_i - (r^3/H) * x_i * sum_j(dy_j*w_j*x_j)
__global__ void rmsnorm_bwd_dx_kernel(const bf16x8* __restrict__ dy,
                                      const bf16x8* __restrict__ x,
                                      const bf16x8* __restrict__ w,
                                      const float* __restrict__ rinv,
                                      const bf16x8* __restrict__ dextra,
                                      bf16x8* __restrict__ dx,
                                      int H8, int rows) {
  __shared__ float scratch[16];
  const int H = H8 * 8;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const bf16x8* dyr = dy + (size_t)row * H8;
    const bf16x8* xr = x + (size_t)row * H8;
    bf16x8* dxr = dx + (size_t)row * H8;
    const float r = rinv[row];
    float s = 0.f;
    for (int i = threadIdx.x; i < H8; i += blockDim.x) {
      bf16x8 d = dyr[i], xv = xr[i], wv = w[i];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        s += bf2f(d.v[j]) * bf2f(wv.v[j]) * bf2f(xv.v[j]);
    }
    s = block_reduce_sum(s, scratch);
    const float c = r * r * r * s / H;
    for (int i = threadIdx.x; i < H8; i += blockDim.x) {
      bf16x8 d = dyr[i], xv = xr[i], wv = w[i];
      bf16x8 o;
      if (dextra != nullptr) {
        const bf16x8 de = dextra[(size_t)row * H8 + i];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o.v[j] = f2bf(r * bf2f(wv.v[j]) * bf2f(d.v[j]) - c * bf2f(xv.v[j])
                        + bf2f(de.v[j]));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o.v[j] = f2bf(r * bf2f(wv.v[j]) * bf2f(d.v[j]) - c * bf2f(xv.v[j]));
      }
      dxr[i] = o;
    }
    __syncthreads();
  }
}

// dw_j = sum_rows dy[i,j] * x[i,j] * rinv[i]; column-parallel with a
// row-chunk grid dim + fp32 atomics (few hundred K atomics total).
__global__ void rmsnorm_bwd_dw_kernel(const short* __restrict__ dy,
                                      const short* __restrict__ x,
                                      const float* __restrict__ rinv,
                                      float* __restrict__ dw,
                                      int H, int rows, int rows_per_chunk) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= H) return;
  const int r0 = blockIdx.y * rows_per_chunk;
  const int r1 = min(r0 + rows_per_chunk, rows);
  float acc = 0.f;
  for (int i = r0; i < r1; ++i) {
    size_t off = (size_t)i * H + col;
    acc += bf2f(dy[off]) * bf2f(x[off]) * rinv[i];
  }
  atomicAdd(&dw[col], acc);
}

// ---------------- fused backward: dx and dw in ONE pass ----------------
// Same dx as rmsnorm_bwd_dx_kernel. A thread always owns the same column
// chunks (threadIdx.x + k*256, k < NC), so dy and x stay in registers
// between the two loops and the thread sums dy*x*rinv for its columns over
// every row the block visits. The block then writes one fp32 row of
// partials to part[gridDim.x][H]; rmsnorm_bwd_dw_finalize_kernel adds the
// rows up. No atomics: two calls give the same bits. H <= NC*2048.
template <int NC>
__global__ __launch_bounds__(256) void rmsnorm_bwd_fused_kernel(
    const bf16x8* __restrict__ dy, const bf16x8* __restrict__ x,
    const bf16x8* __restrict__ w, const float* __restrict__ rinv,
    const bf16x8* __restrict__ dextra, bf16x8* __restrict__ dx,
    float* __restrict__ part, int H8, int rows) {
  __shared__ float scratch[16];
  const int H = H8 * 8;
  bf16x8 wv[NC];
  float pw[NC][8];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int i = threadIdx.x + k * 256;
    if (i < H8) wv[k] = w[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) pw[k][j] = 0.f;
  }
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const bf16x8* dyr = dy + (size_t)row * H8;
    const bf16x8* xr = x + (size_t)row * H8;
    bf16x8* dxr = dx + (size_t)row * H8;
    const float r = rinv[row];
    bf16x8 d[NC], xv[NC];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int i = threadIdx.x + k * 256;
      if (i < H8) {
        d[k] = dyr[i];
        xv[k] = xr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s += bf2f(d[k].v[j]) * bf2f(wv[k].v[j]) * bf2f(xv[k].v[j]);
      }
    }
    s = block_reduce_sum(s, scratch);
    const float c = r * r * r * s / H;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int i = threadIdx.x + k * 256;
      if (i < H8) {
        bf16x8 o;
        if (dextra != nullptr) {
          const bf16x8 de = dextra[(size_t)row * H8 + i];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            o.v[j] = f2bf(r * bf2f(wv[k].v[j]) * bf2f(d[k].v[j]) -
                          c * bf2f(xv[k].v[j]) + bf2f(de.v[j]));
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            o.v[j] = f2bf(r * bf2f(wv[k].v[j]) * bf2f(d[k].v[j]) -
                          c * bf2f(xv[k].v[j]));
        }
        dxr[i] = o;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          pw[k][j] += bf2f(d[k].v[j]) * bf2f(xv[k].v[j]) * r;
      }
    }
    __syncthreads();
  }
  f32x4* prow = (f32x4*)(part + (size_t)blockIdx.x * H);
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int i = threadIdx.x + k * 256;
    if (i < H8) {
      f32x4 lo, hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo.v[j] = pw[k][j];
        hi.v[j] = pw[k][4 + j];
      }
      prow[2 * i] = lo;
      prow[2 * i + 1] = hi;
    }
  }
}

// dw[c] = sum_g part[g][c], g ascending within a slice, slices ascending:
// a fixed order. 16 columns x 16 row slices per block (64 contiguous bytes
// per read of a partial row): H/16 blocks, enough to fill the GPU at
// H=4096. mode 0: fp32 dw_f32[c] = sum; mode 1: bf16 dw_bf[c] = sum;
// mode 2: bf16 dw_bf[c] += sum (one rounding).
#define RMS_FIN_COLS 16
#define RMS_FIN_SLICES 16
__global__ __launch_bounds__(256) void rmsnorm_bwd_dw_finalize_kernel(
    const float* __restrict__ part, float* __restrict__ dw_f32,
    short* __restrict__ dw_bf, int H, int nparts, int mode) {
  __shared__ float red[RMS_FIN_SLICES][RMS_FIN_COLS];
  const int cl = threadIdx.x % RMS_FIN_COLS;
  const int sl = threadIdx.x / RMS_FIN_COLS;
  const int col = blockIdx.x * RMS_FIN_COLS + cl;
  float acc = 0.f;
  if (col < H) {
#pragma unroll 8
    for (int g = sl; g < nparts; g += RMS_FIN_SLICES)
      acc += part[(size_t)g * H + col];
  }
  red[sl][cl] = acc;
  __syncthreads();
  if (sl == 0 && col < H) {
    float sum = red[0][cl];
#pragma unroll
    for (int i = 1; i < RMS_FIN_SLICES; ++i) sum += red[i][cl];
    if (mode == 0)
      dw_f32[col] = sum;
    else if (mode == 1)
      dw_bf[col] = f2bf(sum);
    else
      dw_bf[col] = f2bf(bf2f(dw_bf[col]) + sum);
  }
}

// Blocks of the fused backward at rows x H = 8192 x 4096 (the 7B shape);
// the [grid, H] fp32 partials cost grid*H*8 bytes of traffic against the
// occupancy of the memory-bound row pass (docs/kernels.md). A plain
// process-wide value without synchronisation: a tuning knob for the grid
// sweep of tools/bench_bwd_tail.py and the tests, not thread-safe and not
// meant to be changed while training runs.
static int g_rms_bwd_grid = 1024;

extern "C" {

// grid < 0: query only. Returns the grid cap in force before the call.
int rmsnorm_bwd_grid(int grid) {
  const int prev = g_rms_bwd_grid;
  if (grid > 0) g_rms_bwd_grid = grid;
  return prev;
}

// Rows of the fp32 partial workspace the fused backward needs, 0 where H
// exceeds what a thread holds in registers (the two-kernel fallback).
int rmsnorm_bwd_nparts(int rows, int H) {
  if (H > 8192 || rows <= 0) return 0;
  return min(rows, g_rms_bwd_grid);
}

// One-pass backward. part: [nparts, H] fp32 with nparts =
// rmsnorm_bwd_nparts(rows, H) > 0. mode as in the finalize kernel.
void launch_rmsnorm_bwd_fused(const void* dy, const void* x, const void* w,
                              const float* rinv, const void* dextra, void* dx,
                              float* part, int nparts, float* dw_f32,
                              void* dw_bf, int mode, int rows, int H,
                              hipStream_t stream) {
  const int H8 = H / 8;
#define RMS_FUSED(NC)                                                        \
  rmsnorm_bwd_fused_kernel<NC><<<nparts, 256, 0, stream>>>(                  \
      (const bf16x8*)dy, (const bf16x8*)x, (const bf16x8*)w, rinv,           \
      (const bf16x8*)dextra, (bf16x8*)dx, part, H8, rows)
  if (H8 <= 256)
    RMS_FUSED(1);
  else if (H8 <= 512)
    RMS_FUSED(2);
  else
    RMS_FUSED(4);
#undef RMS_FUSED
  rmsnorm_bwd_dw_finalize_kernel<<<(H + RMS_FIN_COLS - 1) / RMS_FIN_COLS, 256,
                                   0, stream>>>(part, dw_f32, (short*)dw_bf,
                                                H, nparts, mode);
}

// fp32 [H] -> bf16 destination (overwrite or accumulate): the tail of the
// two-kernel fallback when the caller wants dw in a bf16 view.
void launch_rmsnorm_dw_store(const float* dw_f32, void* dw_bf, int mode,
                             int H, hipStream_t stream) {
  rmsnorm_bwd_dw_finalize_kernel<<<(H + RMS_FIN_COLS - 1) / RMS_FIN_COLS, 256,
                                   0, stream>>>(dw_f32, nullptr,
                                                (short*)dw_bf, H, 1, mode);
}

void launch_rmsnorm_fwd(const void* x, const void* w, void* y, float* rinv,
                        int rows, int H, float eps, hipStream_t stream) {
  int grid = min(rows, 2048);
  rmsnorm_fwd_kernel<<<grid, 256, 0, stream>>>(
      (const bf16x8*)x, (const bf16x8*)w, (bf16x8*)y, rinv, H / 8, eps, rows);
}

void launch_add_rmsnorm_fwd(const void* x, const void* res, const void* w,
                            void* y, void* s_out, float* rinv, int rows,
                            int H, float eps, hipStream_t stream) {
  int grid = min(rows, 2048);
  add_rmsnorm_fwd_kernel<<<grid, 256, 0, stream>>>(
      (const bf16x8*)x, (const bf16x8*)res, (const bf16x8*)w, (bf16x8*)y,
      (bf16x8*)s_out, rinv, H / 8, eps, rows);
}

void launch_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                        const float* rinv, const void* dextra, void* dx,
                        float* dw, int rows, int H, hipStream_t stream) {
  int grid = min(rows, 2048);
  rmsnorm_bwd_dx_kernel<<<grid, 256, 0, stream>>>(
      (const bf16x8*)dy, (const bf16x8*)x, (const bf16x8*)w, rinv,
      (const bf16x8*)dextra, (bf16x8*)dx, H / 8, rows);
  int rows_per_chunk = max(1, (rows + 63) / 64);
  dim3 g2((H + 255) / 256, (rows + rows_per_chunk - 1) / rows_per_chunk);
  rmsnorm_bwd_dw_kernel<<<g2, 256, 0, stream>>>(
      (const short*)dy, (const short*)x, rinv, dw, H, rows, rows_per_chunk);
}

}  // extern "C"
