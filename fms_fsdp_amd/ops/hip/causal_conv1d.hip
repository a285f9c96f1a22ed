// Fused causal depthwise conv1d + silu (mamba xBC conv, width<=4) and its
// backward. Memory-bound; bf16x8 vectorized channel access (guide G13).
// Replaces mamba_ssm's causal-conv1d .cu kernel.
// x (b, l, C) bf16 row-major; weight (C, W) bf16; bias (C) fp32.
//
// STRIP kernels: one thread produces 8 consecutive timesteps for its
// 8-channel block, with the x (or g) rows entering a W-deep sliding
// register window — each row is loaded ONCE and the weights are
// unpacked once per strip. The per-(t,c) predecessor re-read every row
// W times and re-unpacked the weights per output; it measured ~1.9 TB/s
// effective (230-300 us per call, 12% of the mamba step across the four
// kernels).
//
// DOCMASK instantiations (packed rows, docs/kernels.md "Document mask"):
// tap x[r] of output t counts iff r >= start[t], the first position of
// t's document (unmasked: r >= 0). `dstart` / `dend` are the flat (b*L)
// int32 arrays of ops.DocMask. The strip kernels keep their ring
// buffers; the mask is a select to 0 where a tap is consumed, with row
// t's bound read once into a register and clamped (start into [0, t],
// end into [t+1, L]), so no array content moves an address or a loop
// bound. A masked tap adds +0 in the same order as an out-of-row tap, so
// the result equals the unmasked kernel run on the document's slice.
#include "common.h"

// per-thread 8-channel weight block: channels c0..c0+7, W taps each,
// stored row-major (c, wi) -> flat j*W+wi over 4 bf16x8 vectors
template <int W>
struct WBlock {
  bf16x8 v[(8 * W + 7) / 8];
  __device__ __forceinline__ void load(const short* w, int c0) {
#pragma unroll
    for (int k = 0; k < (8 * W + 7) / 8; ++k)
      v[k] = ((const bf16x8*)(w + (long long)c0 * W))[k];
  }
  __device__ __forceinline__ float at(int j, int wi) const {
    const int f = j * W + wi;
    return bf2f(v[f / 8].v[f % 8]);
  }
};

template <int W>
__device__ __forceinline__ void unpack_wb(const short* w, int c0,
                                          float wf[8][W]) {
  WBlock<W> wb;
  wb.load(w, c0);
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int wi = 0; wi < W; ++wi) wf[j][wi] = wb.at(j, wi);
}

__device__ __forceinline__ void load_row8(const short* p, float o[8]) {
  const bf16x8 v = *(const bf16x8*)p;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = bf2f(v.v[j]);
}

// strip index decode: i -> (b, ts, c0)
#define STRIP_DECODE()                                                     \
  const int C8 = C / 8;                                                    \
  const int LS = (L + 7) / 8;                                              \
  const int c0 = (int)(i % C8) * 8;                                        \
  long long r_ = i / C8;                                                   \
  const int ts = (int)(r_ % LS) * 8;                                       \
  const long long b_ = r_ / LS;

template <int W, bool DOCMASK>
__global__ void cconv_fwd_kernel(const short* __restrict__ x,
                                 const short* __restrict__ w,
                                 const float* __restrict__ bias,
                                 short* __restrict__ y,
                                 int L, int C, long long nstrip,
                                 const int* __restrict__ dstart) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nstrip) return;
  STRIP_DECODE();
  const short* xb = x + b_ * L * (long long)C + c0;
  short* yb = y + b_ * L * (long long)C + c0;
  float wf[8][W];
  unpack_wb<W>(w, c0, wf);
  const f32x4 bv0 = *(const f32x4*)(bias + c0);
  const f32x4 bv1 = *(const f32x4*)(bias + c0 + 4);
  float bb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bb[j] = j < 4 ? bv0.v[j] : bv1.v[j - 4];
  // ring[p] holds row ts + p - (W-1) at first; slot of row t is
  // (t - ts + W - 1) % W (constant-folded under the unrolled tt loop)
  float ring[W][8];
#pragma unroll
  for (int k = 0; k < W - 1; ++k) {
    const int ti = ts - (W - 1) + k;
    if (ti >= 0)
      load_row8(xb + (long long)ti * C, ring[k]);
    else
#pragma unroll
      for (int j = 0; j < 8; ++j) ring[k][j] = 0.f;
  }
#pragma unroll
  for (int tt = 0; tt < 8; ++tt) {
    const int t = ts + tt;
    if (t >= L) break;
    load_row8(xb + (long long)t * C, ring[(tt + W - 1) % W]);
    int st = 0;
    if (DOCMASK) st = min(max(dstart[b_ * L + t], 0), t);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float acc = bb[j];
#pragma unroll
      for (int wi = 0; wi < W; ++wi) { // row t-(W-1)+wi = slot (tt+wi)%W
        const float xv = (!DOCMASK || t - (W - 1) + wi >= st)
                             ? ring[(tt + wi) % W][j] : 0.f;
        acc += wf[j][wi] * xv;
      }
      const float s = 1.f / (1.f + __expf(-acc));
      o.v[j] = f2bf(acc * s);
    }
    *(bf16x8*)(yb + (long long)t * C) = o;
  }
}

// pass 1: g[t,c] = dy[t,c] * dsilu(z[t,c]) with z recomputed
template <int W, bool DOCMASK>
__global__ void cconv_bwd_g_kernel(const short* __restrict__ dy,
                                   const short* __restrict__ x,
                                   const short* __restrict__ w,
                                   const float* __restrict__ bias,
                                   short* __restrict__ g,
                                   int L, int C, long long nstrip,
                                   const int* __restrict__ dstart) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nstrip) return;
  STRIP_DECODE();
  const short* xb = x + b_ * L * (long long)C + c0;
  const short* dyb = dy + b_ * L * (long long)C + c0;
  short* gb = g + b_ * L * (long long)C + c0;
  float wf[8][W];
  unpack_wb<W>(w, c0, wf);
  const f32x4 bv0 = *(const f32x4*)(bias + c0);
  const f32x4 bv1 = *(const f32x4*)(bias + c0 + 4);
  float bb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bb[j] = j < 4 ? bv0.v[j] : bv1.v[j - 4];
  float ring[W][8];
#pragma unroll
  for (int k = 0; k < W - 1; ++k) {
    const int ti = ts - (W - 1) + k;
    if (ti >= 0)
      load_row8(xb + (long long)ti * C, ring[k]);
    else
#pragma unroll
      for (int j = 0; j < 8; ++j) ring[k][j] = 0.f;
  }
#pragma unroll
  for (int tt = 0; tt < 8; ++tt) {
    const int t = ts + tt;
    if (t >= L) break;
    load_row8(xb + (long long)t * C, ring[(tt + W - 1) % W]);
    const bf16x8 d = *(const bf16x8*)(dyb + (long long)t * C);
    int st = 0;
    if (DOCMASK) st = min(max(dstart[b_ * L + t], 0), t);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float z = bb[j];
#pragma unroll
      for (int wi = 0; wi < W; ++wi) {
        const float xv = (!DOCMASK || t - (W - 1) + wi >= st)
                             ? ring[(tt + wi) % W][j] : 0.f;
        z += wf[j][wi] * xv;
      }
      const float s = 1.f / (1.f + __expf(-z));
      o.v[j] = f2bf(bf2f(d.v[j]) * s * (1.f + z * (1.f - s)));
    }
    *(bf16x8*)(gb + (long long)t * C) = o;
  }
}

// pass 2: dx[t,c] = sum_wi g[t + (W-1) - wi, c] * w[c, wi]
// (future-looking window: rows t..t+W-1, slot of row r = (r - ts) % W)
// DOCMASK: row r counts iff r < end[t], the start of the next document.
template <int W, bool DOCMASK>
__global__ void cconv_bwd_dx_kernel(const short* __restrict__ g,
                                    const short* __restrict__ w,
                                    short* __restrict__ dx,
                                    int L, int C, long long nstrip,
                                    const int* __restrict__ dend) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nstrip) return;
  STRIP_DECODE();
  const short* gb = g + b_ * L * (long long)C + c0;
  short* dxb = dx + b_ * L * (long long)C + c0;
  float wf[8][W];
  unpack_wb<W>(w, c0, wf);
  float ring[W][8];
#pragma unroll
  for (int k = 0; k < W - 1; ++k) {   // rows ts..ts+W-2
    const int ti = ts + k;
    if (ti < L)
      load_row8(gb + (long long)ti * C, ring[k % W]);
    else
#pragma unroll
      for (int j = 0; j < 8; ++j) ring[k % W][j] = 0.f;
  }
#pragma unroll
  for (int tt = 0; tt < 8; ++tt) {
    const int t = ts + tt;
    if (t >= L) break;
    const int tin = t + W - 1;
    if (tin < L)
      load_row8(gb + (long long)tin * C, ring[(tt + W - 1) % W]);
    else
#pragma unroll
      for (int j = 0; j < 8; ++j) ring[(tt + W - 1) % W][j] = 0.f;
    int en = L;
    if (DOCMASK) en = min(max(dend[b_ * L + t], t + 1), L);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int wi = 0; wi < W; ++wi) { // row t+W-1-wi = slot (tt+W-1-wi)%W
        const float gv = (!DOCMASK || t + W - 1 - wi < en)
                             ? ring[(tt + W - 1 - wi) % W][j] : 0.f;
        acc += wf[j][wi] * gv;
      }
      o.v[j] = f2bf(acc);
    }
    *(bf16x8*)(dxb + (long long)t * C) = o;
  }
}

// pass 3: dw[c,wi] += sum_{b,t} g[t,c] x[t-W+1+wi,c]; db[c] += sum g
// 8-channel vector loads with the same sliding x window.
// DOCMASK: tap row ti counts iff ti >= start[t]; db is unchanged.
template <int W, bool DOCMASK>
__global__ void cconv_bwd_dwdb_kernel(const short* __restrict__ g,
                                      const short* __restrict__ x,
                                      float* __restrict__ dw,
                                      float* __restrict__ db,
                                      int L, int C,
                                      long long rows, int rows_per_chunk,
                                      const int* __restrict__ dstart) {
  const int c0 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c0 >= C) return;
  const long long r0 = (long long)blockIdx.y * rows_per_chunk;
  const long long r1 = min(r0 + rows_per_chunk, rows);
  float accw[W][8];
#pragma unroll
  for (int wi = 0; wi < W; ++wi)
#pragma unroll
    for (int j = 0; j < 8; ++j) accw[wi][j] = 0.f;
  float accb[8] = {0.f};
  float ring[W][8];
  int ring_t = -1 << 30;   // row index held in the newest slot
  for (long long bt = r0; bt < r1; ++bt) {
    const int t = (int)(bt % L);
    const long long row0 = bt - t;
    // (re)fill the window when the sequence or chunk boundary breaks it
    if (bt == r0 || t == 0 || ring_t != t - 1) {
#pragma unroll
      for (int k = 0; k < W - 1; ++k) {
        const int ti = t - (W - 1) + k;
        if (ti >= 0)
          load_row8(x + (row0 + ti) * C + c0, ring[(ti % W + W) % W]);
        else {
          const int slot = ((ti % W) + W) % W;
#pragma unroll
          for (int j = 0; j < 8; ++j) ring[slot][j] = 0.f;
        }
      }
    }
    load_row8(x + bt * C + c0, ring[t % W]);
    ring_t = t;
    float gv[8];
    load_row8(g + bt * C + c0, gv);
#pragma unroll
    for (int j = 0; j < 8; ++j) accb[j] += gv[j];
    int st = 0;
    if (DOCMASK) st = min(max(dstart[bt], 0), t);
#pragma unroll
    for (int wi = 0; wi < W; ++wi) {
      const int ti = t - (W - 1) + wi;
      const int slot = ((ti % W) + W) % W;
      if (ti >= st)
#pragma unroll
        for (int j = 0; j < 8; ++j) accw[wi][j] += gv[j] * ring[slot][j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int wi = 0; wi < W; ++wi)
      atomicAdd(&dw[(long long)(c0 + j) * W + wi], accw[wi][j]);
    atomicAdd(&db[c0 + j], accb[j]);
  }
}

// Recurrent decode: T new rows behind a carried conv state. state
// (b, W-1, C) holds the last W-1 RAW inputs of the sequence, oldest first
// (zeros for a fresh one); x (b, T, C) is row-strided (row b*T + t at
// that many times sx elements). Writes y = silu(conv + bias) over
// [state | x] and leaves the last W-1 rows of [state | x] in the state,
// for T < W-1 and T >= W-1 alike. One thread owns 8 channels for all T
// rows with the W-deep window in registers (shifted, so every index is
// static); channels are independent, so the in-place state update needs
// no synchronisation. The accumulation chain is cconv_fwd_kernel's (bias
// first, taps in wi order, the same silu): y equals cconv_fwd on the
// concatenated sequence bit for bit, a zero state row standing in for a
// tap in front of the row.
template <int W>
__global__ void cconv_update_kernel(short* __restrict__ state,
                                    const short* __restrict__ x,
                                    const short* __restrict__ w,
                                    const float* __restrict__ bias,
                                    short* __restrict__ y, int T, int C,
                                    long long sx, long long nthr) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nthr) return;
  const int C8 = C / 8;
  const int c0 = (int)(i % C8) * 8;
  const long long b_ = i / C8;
  short* sb = state + b_ * (W - 1) * (long long)C + c0;
  const short* xb = x + b_ * T * sx + c0;
  short* yb = y + b_ * T * (long long)C + c0;
  float wf[8][W];
  unpack_wb<W>(w, c0, wf);
  const f32x4 bv0 = *(const f32x4*)(bias + c0);
  const f32x4 bv1 = *(const f32x4*)(bias + c0 + 4);
  float bb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bb[j] = j < 4 ? bv0.v[j] : bv1.v[j - 4];
  // win[wi] is the tap of weight wi: rows t-(W-1) .. t of [state | x]
  float win[W][8];
#pragma unroll
  for (int k = 0; k < W - 1; ++k)
    load_row8(sb + (long long)k * C, win[k + 1]);
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int k = 0; k < W - 1; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) win[k][j] = win[k + 1][j];
    load_row8(xb + (long long)t * sx, win[W - 1]);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float acc = bb[j];
#pragma unroll
      for (int wi = 0; wi < W; ++wi) acc += wf[j][wi] * win[wi][j];
      const float s = 1.f / (1.f + __expf(-acc));
      o.v[j] = f2bf(acc * s);
    }
    *(bf16x8*)(yb + (long long)t * C) = o;
  }
#pragma unroll
  for (int k = 0; k < W - 1; ++k) {
    bf16x8 o;   // raw bf16 inputs: the float round trip is exact
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = f2bf(win[k + 1][j]);
    *(bf16x8*)(sb + (long long)k * C) = o;
  }
}

extern "C" {

void launch_cconv_update(void* state, const void* x, const void* w,
                         const float* bias, void* y, long long B, int T,
                         int C, int W, long long sx, hipStream_t stream) {
  const long long nthr = B * (C / 8);
  const int block = 256;
  const int grid = (int)((nthr + block - 1) / block);
#define CCONV_UPD(WV)                                                       \
  cconv_update_kernel<WV><<<grid, block, 0, stream>>>(                      \
      (short*)state, (const short*)x, (const short*)w, bias, (short*)y, T,  \
      C, sx, nthr)
  if (W == 4) CCONV_UPD(4);
  else if (W == 3) CCONV_UPD(3);
  else CCONV_UPD(2);
#undef CCONV_UPD
}

// dstart / dend (flat (b*L) int32, ops.DocMask) select the DOCMASK
// instantiations; nullptr is the unmasked kernel.
void launch_cconv_fwd(const void* x, const void* w, const float* bias,
                      void* y, int BL, int L, int C, int W,
                      const int* dstart, hipStream_t stream) {
  const int B = BL / L;
  const long long nstrip = (long long)B * ((L + 7) / 8) * (C / 8);
  const int block = 256;
  const int grid = (int)((nstrip + block - 1) / block);
#define CCONV_FWD(WV, DM)                                                   \
  cconv_fwd_kernel<WV, DM><<<grid, block, 0, stream>>>(                     \
      (const short*)x, (const short*)w, bias, (short*)y, L, C, nstrip,      \
      dstart)
  if (dstart) {
    if (W == 4) CCONV_FWD(4, true);
    else if (W == 3) CCONV_FWD(3, true);
    else CCONV_FWD(2, true);
  } else {
    if (W == 4) CCONV_FWD(4, false);
    else if (W == 3) CCONV_FWD(3, false);
    else CCONV_FWD(2, false);
  }
#undef CCONV_FWD
}

void launch_cconv_bwd(const void* dy, const void* x, const void* w,
                      const float* bias, void* g, void* dx, float* dw,
                      float* db, int BL, int L, int C, int W,
                      const int* dstart, const int* dend,
                      hipStream_t stream) {
  const int B = BL / L;
  const long long nstrip = (long long)B * ((L + 7) / 8) * (C / 8);
  const int block = 256;
  const int grid = (int)((nstrip + block - 1) / block);
  const int rpc = max(1, (int)((BL + 63) / 64));
  dim3 g2((C / 8 + 255) / 256, (BL + rpc - 1) / rpc);
#define CCONV_BWD(WV, DM)                                                   \
  do {                                                                      \
    cconv_bwd_g_kernel<WV, DM><<<grid, block, 0, stream>>>(                 \
        (const short*)dy, (const short*)x, (const short*)w, bias,           \
        (short*)g, L, C, nstrip, dstart);                                   \
    cconv_bwd_dx_kernel<WV, DM><<<grid, block, 0, stream>>>(                \
        (const short*)g, (const short*)w, (short*)dx, L, C, nstrip, dend);  \
    cconv_bwd_dwdb_kernel<WV, DM><<<g2, 256, 0, stream>>>(                  \
        (const short*)g, (const short*)x, dw, db, L, C, BL, rpc, dstart);   \
  } while (0)
  if (dstart) {
    if (W == 4) CCONV_BWD(4, true);
    else if (W == 3) CCONV_BWD(3, true);
    else CCONV_BWD(2, true);
  } else {
    if (W == 4) CCONV_BWD(4, false);
    else if (W == 3) CCONV_BWD(3, false);
    else CCONV_BWD(2, false);
  }
#undef CCONV_BWD
}

}  // extern "C"
