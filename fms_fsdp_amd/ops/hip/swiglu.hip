// SwiGLU epilogue: h = silu(g) * u over fused (N, 2H) gate|up layout,
// and its backward. Memory-bound; bf16x8 vectorized (guide G13).
// Replaces the torch.compile fusion the reference leans on
// (SwiGLU MLP epilogue).
#include "transpose_tile.h"

__global__ void swiglu_fwd_kernel(const bf16x8* __restrict__ gu,
                                  bf16x8* __restrict__ h,
                                  int H8, long long rows) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = rows * H8;
  if (i >= total) return;
  const long long row = i / H8;
  const int col = (int)(i % H8);
  const bf16x8 g = gu[row * 2 * H8 + col];
  const bf16x8 u = gu[row * 2 * H8 + H8 + col];
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float gf = bf2f(g.v[j]);
    const float s = 1.f / (1.f + __expf(-gf));
    o.v[j] = f2bf(gf * s * bf2f(u.v[j]));
  }
  h[i] = o;
}

// dg = dy * u * s * (1 + g*(1-s)),  du = dy * g * s,  s = sigmoid(g)
__global__ void swiglu_bwd_kernel(const bf16x8* __restrict__ dy,
                                  const bf16x8* __restrict__ gu,
                                  bf16x8* __restrict__ dgu,
                                  int H8, long long rows) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = rows * H8;
  if (i >= total) return;
  const long long row = i / H8;
  const int col = (int)(i % H8);
  const bf16x8 g = gu[row * 2 * H8 + col];
  const bf16x8 u = gu[row * 2 * H8 + H8 + col];
  const bf16x8 d = dy[i];
  bf16x8 og, ou;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float gf = bf2f(g.v[j]);
    const float uf = bf2f(u.v[j]);
    const float df = bf2f(d.v[j]);
    const float s = 1.f / (1.f + __expf(-gf));
    og.v[j] = f2bf(df * uf * s * (1.f + gf * (1.f - s)));
    ou.v[j] = f2bf(df * gf * s);
  }
  dgu[row * 2 * H8 + col] = og;
  dgu[row * 2 * H8 + H8 + col] = ou;
}

// The backward for the fused MLP backward (ops/__init__.py, _SwiGLUMLPFn):
// dgu as swiglu_bwd_kernel writes it, and in the same pass the operands
// the two wgrad GEMMs want token-contiguous, dguT (2H, rows) = dgu^T and
// hT (H, rows) = swiglu_fwd(gu)^T, so that neither dgu nor h is read back
// by a transpose. dg, du and h are the expressions of the two kernels
// above, in their order: every output has their bits.
// One block = a 64x64 tile of (rows, H), laid out as transpose.hip's:
// 16-B loads along the rows, dg|du stored row-major from registers, and
// dg, du, h each through an LDS tile of transpose_tile.h, drained with
// 16-B stores along the tokens. rows % 8 == 0 and H % 8 == 0.
__global__ __launch_bounds__(256) void swiglu_bwd_t_kernel(
    const short* __restrict__ dh, const short* __restrict__ gu,
    short* __restrict__ dgu, short* __restrict__ dguT,
    short* __restrict__ hT, long long rows, long long H, long long tiles_c) {
  __shared__ bf16x8 tile_g[TR_TILE * TR_CHUNKS];
  __shared__ bf16x8 tile_u[TR_TILE * TR_CHUNKS];
  __shared__ bf16x8 tile_h[TR_TILE * TR_CHUNKS];
  const int t = threadIdx.x;
  const long long r0 = ((long long)blockIdx.x / tiles_c) * TR_TILE;
  const long long c0 = ((long long)blockIdx.x % tiles_c) * TR_TILE;
  const int sub = t % TR_CHUNKS;   // chunk on the way in, row group out
  const int line = t / TR_CHUNKS;  // 0..31

#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int lr = line + p * 32;
    const long long r = r0 + lr, c = c0 + sub * 8;
    bf16x8 og = {}, ou = {}, oh = {};
    if (r < rows && c < H) {   // H % 8 == 0: a chunk is all in or out
      const bf16x8 g = *(const bf16x8*)(gu + r * 2 * H + c);
      const bf16x8 u = *(const bf16x8*)(gu + r * 2 * H + H + c);
      const bf16x8 d = *(const bf16x8*)(dh + r * H + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gf = bf2f(g.v[j]);
        const float uf = bf2f(u.v[j]);
        const float df = bf2f(d.v[j]);
        const float s = 1.f / (1.f + __expf(-gf));
        og.v[j] = f2bf(df * uf * s * (1.f + gf * (1.f - s)));
        ou.v[j] = f2bf(df * gf * s);
        oh.v[j] = f2bf(gf * s * uf);
      }
      *(bf16x8*)(dgu + r * 2 * H + c) = og;
      *(bf16x8*)(dgu + r * 2 * H + H + c) = ou;
    }
    tr_tile_put(tile_g, lr, sub, og);
    tr_tile_put(tile_u, lr, sub, ou);
    tr_tile_put(tile_h, lr, sub, oh);
  }
  __syncthreads();

#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int lc = line + p * 32;            // tile column = dst row
    const long long c = c0 + lc, r = r0 + sub * 8;
    if (c >= H || r >= rows) continue;   // rows % 8 == 0: a run is all in
    *(bf16x8*)(dguT + c * rows + r) = tr_tile_take(tile_g, lc, sub);
    *(bf16x8*)(dguT + (H + c) * rows + r) = tr_tile_take(tile_u, lc, sub);
    *(bf16x8*)(hT + c * rows + r) = tr_tile_take(tile_h, lc, sub);
  }
}

extern "C" {

void launch_swiglu_fwd(const void* gu, void* h, long long rows, int H,
                       hipStream_t stream) {
  long long total = rows * (H / 8);
  int block = 256;
  swiglu_fwd_kernel<<<(int)((total + block - 1) / block), block, 0, stream>>>(
      (const bf16x8*)gu, (bf16x8*)h, H / 8, rows);
}

void launch_swiglu_bwd(const void* dy, const void* gu, void* dgu,
                       long long rows, int H, hipStream_t stream) {
  long long total = rows * (H / 8);
  int block = 256;
  swiglu_bwd_kernel<<<(int)((total + block - 1) / block), block, 0, stream>>>(
      (const bf16x8*)dy, (const bf16x8*)gu, (bf16x8*)dgu, H / 8, rows);
}

// rows % 8 == 0, H % 8 == 0, every pointer 16-B aligned, all contiguous.
void launch_swiglu_bwd_t(const void* dh, const void* gu, void* dgu,
                         void* dguT, void* hT, long long rows, int H,
                         hipStream_t stream) {
  if (rows <= 0 || H <= 0) return;
  const long long tiles_c = (H + TR_TILE - 1) / TR_TILE;
  const long long tiles_r = (rows + TR_TILE - 1) / TR_TILE;
  swiglu_bwd_t_kernel<<<(unsigned)(tiles_r * tiles_c), 256, 0, stream>>>(
      (const short*)dh, (const short*)gu, (short*)dgu, (short*)dguT,
      (short*)hT, rows, H, tiles_c);
  HIP_CHECK_LAUNCH();
}

}  // extern "C"
