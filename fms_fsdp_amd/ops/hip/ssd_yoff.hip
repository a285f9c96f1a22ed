// The y_off term of the Mamba2 SSD and its backward (docs/kernels.md
// "ssd_yoff.hip"). m = bc*H + h, g = h / rep, r = h % rep, rep = H/G:
//   yoff[bc, g, q, r, p] = sum_k C[bc*Q + q, g*N + k] * prev[m, k, p]
//   dprev[m, k, p]       = sum_q C[bc*Q + q, g*N + k] * dyoff[bc, g, q, r, p]
//   dC[bc*Q + q, g*N+k]  = sum_{r, p} dyoff[bc, g, q, r, p] * prev[m, k, p]
// yoff / dyoff are (bc, G, Q, rep, P) bf16, the layout ssd_ygate reads: row
// q holds the group's rep*P features contiguously, so the heads of a block
// are adjacent in a row. prev / dprev are (bc*H, N, P) bf16 contiguous, C a
// (bc*Q, G*N) bf16 slice with row stride sC. The decay exp(dacs) and the
// document mask on this term live in ssd_ygate; nothing here is masked.
//
// ---- ssd_yoff_fwd_kernel<N, P> ------------------------------------------
// One workgroup of 4 waves per (bc, g, block of up to 128 rows q, head
// block), head block fastest in the grid. Wave w owns rows q0 + 32w .. +31
// with the own row on the MFMA column (ssd_diag's swapped layout):
//   Y^T[p][q] = prev^T[p][k] C^T[k][q]
// B operand = the lane's own C row (N/16 fragments from global, constant
// over the heads), A operand = transpose reads of the [N][P] subtiled image
// of prev[m]. The image is double-buffered across the heads: the next
// head's tile is fetched into registers before the current head's MFMAs
// and committed to the other image before the head's single barrier. The
// accumulators go through a wave-private LDS strip that holds the spans of
// two consecutive heads, so that a row leaves as 2*P contiguous elements
// (16-byte stores); an odd last head leaves as P. Waves past Q only stage.
//
// ---- ssd_yoff_dprev_kernel<N, P> ----------------------------------------
// The shape of ssd_chunk_state_kernel: one workgroup per (bc, g, head
// block), output tile NI x P per head (NI = max(N, 32)) split WK x WP over
// the waves, dprev^T[p][k] = dyoff^T[p][q] C[q][k] with both operands as
// transpose reads. The loop runs over the 64-row tiles of the chunk: a
// tile of C is staged once, the wave's C^T fragments of the tile stay in
// registers across the heads, and the tile of dyoff is staged as ONE
// [64][HB*P] slab (16-byte loads, consecutive threads along the row, runs
// of HB*P*2 bytes). In the column-block-major subtiled layout head j's
// image is the slab at byte offset j * 64*P*2, so the per-head images are
// cut out by offset. The accumulators of all HB heads persist over the
// tiles, which bounds HB: HB * NI * P <= 32768 (128 VGPRs).
//
// ---- ssd_yoff_dC_kernel<N, P> -------------------------------------------
// Grid and row ownership of the forward. dC^T[k][q] += prev[k][p]
// dyoff^T[p][q]: B operand = the lane's own dyoff[q, r, :] (P/16 fragments
// from global, issued before the head's first barrier), A operand = plain
// 16-byte reads of the prev[m] image with row k on lane & 31. The N/32 x 16
// accumulators persist over the head loop (the group sum happens in fp32
// registers) and go to partial hbk of a (nhb, bc*Q, G*N) fp32 buffer that
// the caller sums. No atomics anywhere: two calls give the same bits.
//
// N = 16: rows 16..31 of the prev image are never written and feed no
// output. The forward runs its one 16-row MFMA on rows 0..15; in dC they
// reach only rows 16..31 of the tile, which are never stored. dprev pads
// the C image with zero columns. No address or loop bound depends on array
// contents. 64-bit indexing.
#include <cstdio>
#include <cstdlib>

#include "ssd_diag_frag.h"

// lane terms of a transpose read of a 64-row subtiled image (ssd_diag's
// xtr): R4 = 16 row groups per 16-column block (2048 B)
__device__ __forceinline__ unsigned yoff_ltr(int lane) {
  const int hb = lane >> 5;
  return (unsigned)((((lane & 15) * 8) ^ (16 * hb)) + hb * 256 +
                    ((lane & 31) >> 4) * 2048);
}

template <int N, int P>
struct YFGeom {
  static constexpr int NCH = N / 16;            // 16-wide k chunks
  static constexpr int NKT = (N + 31) / 32;     // 32-row blocks of the image
  static constexpr int NT = P / 32;             // 32-feature tiles
  static constexpr int PCH = P / 16;
  static constexpr int IMG = DIAG_KT * P * 2;   // one 64-row tile
  static constexpr int NIMG = (N + DIAG_KT - 1) / DIAG_KT;
  static constexpr int PIMG = NIMG * IMG;       // one prev image
  static constexpr int NLD = (N * P / 8 + 255) / 256;   // 16-byte loads/thread
  static constexpr int ERS = 2 * P * 2 + 16;    // strip row: two heads' spans
  static constexpr int LDS_FWD = 2 * PIMG + 4 * 32 * ERS;
};

// prev[m] -> registers -> image, 16 bytes per thread and step
template <int N, int P>
__device__ __forceinline__ void yoff_fetch(
    const short* __restrict__ prev, long long m, int tid,
    f32x4v (&rg)[YFGeom<N, P>::NLD]) {
  const short* pb = prev + m * ((long long)N * P);
#pragma unroll
  for (int i = 0; i < YFGeom<N, P>::NLD; ++i) {
    const int s = tid + i * 256;
    if (s < N * P / 8) rg[i] = *(const f32x4v*)(pb + s * 8);
  }
}

template <int N, int P>
__device__ __forceinline__ void yoff_commit(
    char* img, int tid, const f32x4v (&rg)[YFGeom<N, P>::NLD]) {
#pragma unroll
  for (int i = 0; i < YFGeom<N, P>::NLD; ++i) {
    const int s = tid + i * 256;
    const int k = s / (P / 8), c8 = (s % (P / 8)) * 8;
    if (s < N * P / 8)
      *(f32x4v*)(img + (k / DIAG_KT) * YFGeom<N, P>::IMG +
                SUBT_OFF(k % DIAG_KT, c8, 16)) = rg[i];
  }
}

// (hblk, rb, g, bc) of a workgroup, head block fastest
__device__ __forceinline__ void yoff_decode(int nhb, int nrb, int G, int& hbk,
                                            int& rb, int& g, long long& bc) {
  unsigned rest = blockIdx.x;
  hbk = (int)(rest % (unsigned)nhb);
  rest /= (unsigned)nhb;
  rb = (int)(rest % (unsigned)nrb);
  rest /= (unsigned)nrb;
  g = (int)(rest % (unsigned)G);
  bc = rest / (unsigned)G;
}

template <int N, int P>
__global__ __launch_bounds__(256, 2) void ssd_yoff_fwd_kernel(
    const short* __restrict__ Cg, const short* __restrict__ prev,
    short* __restrict__ yoff, int H, int G, int Q, long long sC, int nrb,
    int HB, int nhb) {
  using Ge = YFGeom<N, P>;
  constexpr int NCH = Ge::NCH, NKT = Ge::NKT, NT = Ge::NT, ERS = Ge::ERS;
  static_assert(N % 16 == 0 && (N == 16 || N % 32 == 0) && P % 32 == 0,
                "tile shape");
  __shared__ __attribute__((aligned(128))) char smem[Ge::LDS_FWD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;             // own row inside the wave's 32
  const int hb = lane >> 5;
  char* ep = smem + 2 * Ge::PIMG + wid * (32 * ERS);

  int hbk, rb, g;
  long long bc;
  yoff_decode(nhb, nrb, G, hbk, rb, g, bc);
  const int rep = H / G;
  const int r_lo = hbk * HB;
  const int r_hi = min(rep, r_lo + HB);

  const int qw = rb * DIAG_ROWS + wid * 32;          // wave's first own row
  const bool live = qw < Q;                          // wave-uniform
  const int my_q = qw + col;

  // the lane's own C row as B-operand fragments, constant over the heads
  bf16x8v cf[NCH];
  if (live) {
    const short* cp = Cg + (bc * Q + my_q) * sC + (long long)g * N + hb * 8;
#pragma unroll
    for (int c = 0; c < NCH; ++c) cf[c] = *(const bf16x8v*)(cp + c * 16);
  }

  const unsigned str = (unsigned)(unsigned long long)smem + yoff_ltr(lane);
  const long long rowlen = (long long)rep * P;       // one yoff row
  short* yw = yoff + ((bc * G + g) * Q + qw) * rowlen;

  f32x4v rg[Ge::NLD];
  long long m = bc * H + (long long)g * rep + r_lo;
  yoff_fetch<N, P>(prev, m, tid, rg);
  yoff_commit<N, P>(smem, tid, rg);
  __syncthreads();

  for (int r = r_lo, i = 0; r < r_hi; ++r, ++i, ++m) {
    const bool more = r + 1 < r_hi;
    const int odd = i & 1;
    if (more) yoff_fetch<N, P>(prev, m + 1, tid, rg);
    if (live) {
      f32x16 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = (f32x16)(0.f);
      const unsigned cur = str + odd * Ge::PIMG;
#pragma unroll
      for (int kk = 0; kk < NKT; ++kk) {
        const unsigned base = cur + (kk >> 1) * Ge::IMG + (kk & 1) * 1024;
        U2x64 fr[2][2];
        tr_issue4<0, 128, 512, 640>(base, fr[0][0], fr[0][1]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int pp = t & 1;
          if (t + 1 < NT) {
            tr_issue4<0, 128, 512, 640>(base + (t + 1) * 4096, fr[pp ^ 1][0],
                                        fr[pp ^ 1][1]);
            tr_wait<4>(fr[pp][0], fr[pp][1]);
          } else {
            tr_wait<0>(fr[pp][0], fr[pp][1]);
          }
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              fr[pp][0].v, cf[N >= 32 ? 2 * kk : 0], acc[t], 0, 0, 0);
          if constexpr (N >= 32)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                fr[pp][1].v, cf[2 * kk + 1], acc[t], 0, 0, 0);
        }
      }
      // acc is [p][q]: into the wave's strip as [q][head of the pair][p].
      // The strip is wave-private and a wave's DS operations execute in
      // order: no workgroup barrier between its writes and reads.
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          bf16x4 w;
#pragma unroll
          for (int e = 0; e < 4; ++e) w.v[e] = f2bf(acc[t][q4 * 4 + e]);
          *(bf16x4*)(ep + col * ERS +
                     (odd * P + t * 32 + 8 * q4 + 4 * hb) * 2) = w;
        }
      __builtin_amdgcn_wave_barrier();
      if (odd || !more) {
        // one or two heads' spans of the wave's 32 rows
        const int w8 = (odd + 1) * (P / 8);
        short* yb = yw + (long long)(r - odd) * P;
        for (int s = lane; s < 32 * w8; s += 64) {
          const int row = s / w8, c8 = (s % w8) * 8;
          *(f32x4*)(yb + row * rowlen + c8) =
              *(const f32x4*)(ep + row * ERS + c8 * 2);
        }
      }
    }
    if (more) yoff_commit<N, P>(smem + (odd ^ 1) * Ge::PIMG, tid, rg);
    __syncthreads();     // the other image is complete, this one is free
  }
}

template <int N, int P>
struct YDGeom {
  static constexpr int NI = N < 32 ? 32 : N;          // C image columns
  static constexpr int WK = NI / 32 < 4 ? NI / 32 : 4;
  static constexpr int WP = (4 / WK) < (P / 32) ? (4 / WK) : (P / 32);
  static constexpr int TP = P / 32 / WP;              // 32-feature tiles/wave
  static constexpr int PW = TP * 32;                  // features per wave
  static constexpr int ERS = PW * 2 + 16;             // epilogue row stride
  static constexpr int HBMAX =                        // heads per workgroup
      32768 / (NI * P) < 8 ? 32768 / (NI * P) : 8;
  static constexpr int CIMG = DIAG_KT * NI * 2;       // one tile of C
  static constexpr int XT = DIAG_KT * P * 2;          // one head of the slab
  static constexpr int EPI = 4 * 32 * ERS;
  static constexpr int SLAB = HBMAX * XT > EPI ? HBMAX * XT : EPI;
  static constexpr int LDS = CIMG + SLAB;
};

template <int N, int P>
__global__ __launch_bounds__(256, 2) void ssd_yoff_dprev_kernel(
    const short* __restrict__ dyoff, const short* __restrict__ Cg,
    short* __restrict__ dprev, int H, int G, int Q, long long sC, int HB,
    int nhb) {
  using Ge = YDGeom<N, P>;
  constexpr int TP = Ge::TP, PW = Ge::PW, ERS = Ge::ERS, XT = Ge::XT;
  constexpr int HBMAX = Ge::HBMAX;
  static_assert(N % 16 == 0 && P % 32 == 0 && Ge::NI <= 128 && HBMAX >= 1,
                "tile shape");
  __shared__ __attribute__((aligned(128))) char smem[Ge::LDS];
  char* cimg = smem;
  char* slab = smem + Ge::CIMG;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;
  const int hb = lane >> 5;
  const bool live = wid < Ge::WK * Ge::WP;            // wave-uniform
  const int kb = wid % Ge::WK;                        // block of 32 state rows
  const int pb = wid / Ge::WK;                        // block of PW features

  const int rep = H / G;
  long long w = blockIdx.x;
  const int hblk = (int)(w % nhb);
  w /= nhb;
  const int g = (int)(w % G);
  const long long bc = w / G;
  const int r0 = hblk * HB;
  const int nh = min(rep, r0 + HB) - r0;              // 1 .. HBMAX heads
  const int rw8 = nh * (P / 8);                       // 16-byte pieces per row

  const short* cbase = Cg + bc * Q * sC + (long long)g * N;
  const long long rowlen = (long long)rep * P;
  const short* dbase = dyoff + (bc * G + g) * Q * rowlen + (long long)r0 * P;

  if constexpr (N < Ge::NI) {     // zero the pad columns once
    for (int s = tid; s < Ge::CIMG / 16; s += 256)
      *(f32x4*)(cimg + s * 16) = f32x4{{0.f, 0.f, 0.f, 0.f}};
  }

  const unsigned ltr = yoff_ltr(lane);
  const unsigned ctr = (unsigned)(unsigned long long)cimg + ltr + kb * 4096;
  const unsigned xtr =
      (unsigned)(unsigned long long)slab + ltr + pb * TP * 4096;

  f32x16 acc[HBMAX][TP];
#pragma unroll
  for (int j = 0; j < HBMAX; ++j)
#pragma unroll
    for (int t = 0; t < TP; ++t) acc[j][t] = (f32x16)(0.f);

  for (int kv0 = 0; kv0 < Q; kv0 += DIAG_KT) {
    __syncthreads();     // the previous tile's reads are done
#pragma unroll
    for (int s = tid; s < DIAG_KT * N / 8; s += 256) {
      const int key = s / (N / 8), c8 = (s % (N / 8)) * 8;
      if (kv0 + key < Q)
        *(f32x4*)(cimg + SUBT_OFF(key, c8, 16)) =
            *(const f32x4*)(cbase + (long long)(kv0 + key) * sC + c8);
    }
    // the dyoff tile of all heads of the block as one [64][nh*P] slab
    for (int s = tid; s < DIAG_KT * rw8; s += 256) {
      const int key = s / rw8, c8 = (s % rw8) * 8;
      if (kv0 + key < Q)
        *(f32x4*)(slab + SUBT_OFF(key, c8, 16)) =
            *(const f32x4*)(dbase + (kv0 + key) * rowlen + c8);
    }
    __syncthreads();
    if (!live) continue;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if (kv0 + kt * 32 < Q) {
        U2x64 c0, c1;              // the wave's C^T fragments of these 32 rows
        tr_issue4<0, 128, 512, 640>(ctr + kt * 1024, c0, c1);
        tr_wait<0>(c0, c1);
#pragma unroll
        for (int j = 0; j < HBMAX; ++j) {
          if (j < nh) {
            const unsigned xb = xtr + j * XT + kt * 1024;
            U2x64 fr[TP][2];
#pragma unroll
            for (int t = 0; t < TP; ++t)
              tr_issue4<0, 128, 512, 640>(xb + t * 4096, fr[t][0], fr[t][1]);
#pragma unroll
            for (int t = 0; t < TP; ++t) {
              if (t == 0) {
#pragma unroll
                for (int u = 0; u < TP; ++u) tr_wait<0>(fr[u][0], fr[u][1]);
              }
              acc[j][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  fr[t][0].v, c0.v, acc[j][t], 0, 0, 0);
              acc[j][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  fr[t][1].v, c1.v, acc[j][t], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  __syncthreads();       // the slab becomes the waves' epilogue regions
  if (!live) return;

  // acc[j] is [p][k]: lane = state row k, registers = features. Through the
  // wave-private region (DS operations of a wave execute in order) into
  // 16-byte stores of dprev[m].
  char* ep = slab + wid * (32 * ERS);
#pragma unroll
  for (int j = 0; j < HBMAX; ++j) {
    if (j < nh) {
      const long long m = bc * H + (long long)g * rep + r0 + j;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < TP; ++t)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          bf16x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v.v[e] = f2bf(acc[j][t][q4 * 4 + e]);
          *(bf16x4*)(ep + col * ERS + (t * 32 + 8 * q4 + 4 * hb) * 2) = v;
        }
      __builtin_amdgcn_wave_barrier();
      short* sw = dprev + (m * N + kb * 32) * (long long)P + pb * PW;
#pragma unroll
      for (int s = lane; s < 32 * PW / 8; s += 64) {
        const int row = s / (PW / 8), c8 = (s % (PW / 8)) * 8;
        if (kb * 32 + row < N)
          *(f32x4*)(sw + (long long)row * P + c8) =
              *(const f32x4*)(ep + row * ERS + c8 * 2);
      }
    }
  }
}

// part (nhb, rows, G*N) fp32 with rows = bc*Q
template <int N, int P>
__global__ __launch_bounds__(256, 2) void ssd_yoff_dC_kernel(
    const short* __restrict__ dyoff, const short* __restrict__ prev,
    float* __restrict__ part, int H, int G, int Q, long long rows, int nrb,
    int nhb) {
  using Ge = YFGeom<N, P>;
  constexpr int NKT = Ge::NKT, PCH = Ge::PCH;
  static_assert(N % 16 == 0 && (N == 16 || N % 32 == 0) && P % 32 == 0,
                "tile shape");
  __shared__ __attribute__((aligned(128))) char simg[Ge::PIMG];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;             // own row inside the wave's 32
  const int hb = lane >> 5;

  int hbk, rb, g;
  long long bc;
  yoff_decode(nhb, nrb, G, hbk, rb, g, bc);
  const int rep = H / G;
  const int r_lo = hbk * rep / nhb;                  // uneven splits allowed
  const int r_hi = (hbk + 1) * rep / nhb;

  const int qw = rb * DIAG_ROWS + wid * 32;
  const bool live = qw < Q;                          // wave-uniform
  const int my_q = qw + col;

  f32x16 acc[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) acc[t] = (f32x16)(0.f);

  // the lane's own dyoff row: the heads' P features side by side
  const short* dp =
      dyoff + ((bc * G + g) * Q + my_q) * ((long long)rep * P) + hb * 8;
  f32x4v rg[Ge::NLD];
  for (int r = r_lo; r < r_hi; ++r) {
    const long long m = bc * H + (long long)g * rep + r;
    bf16x8v df[PCH];
    if (live) {
#pragma unroll
      for (int c = 0; c < PCH; ++c)
        df[c] = *(const bf16x8v*)(dp + (long long)r * P + c * 16);
    }
    yoff_fetch<N, P>(prev, m, tid, rg);
    __syncthreads();     // the previous head's image reads are done
    yoff_commit<N, P>(simg, tid, rg);
    __syncthreads();
    if (!live) continue;
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const char* ib = simg + (t >> 1) * Ge::IMG;
#pragma unroll
      for (int c = 0; c < PCH; ++c) {
        const bf16x8v a = *(const bf16x8v*)(
            ib + SUBT_OFF((t & 1) * 32 + col, c * 16 + hb * 8, 16));
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, df[c], acc[t], 0,
                                                         0, 0);
      }
    }
  }
  if (!live) return;

  // acc is [k][q]: four registers = four consecutive k of the lane's own
  // row, one 16-byte store each
  const long long prow = (long long)hbk * rows + bc * Q + my_q;
  float* pw = part + prow * ((long long)G * N) + (long long)g * N;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int k = t * 32 + 8 * q4 + 4 * hb;
      if (k < N) {
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w.v[e] = acc[t][q4 * 4 + e];
        *(f32x4*)(pw + k) = w;
      }
    }
}

template <int N, int P>
static void launch_yf(const void* C, const void* prev, void* yoff,
                      long long bc, int H, int G, int Q, long long sC, int HB,
                      int nhb, hipStream_t stream) {
  const int nrb = (Q + DIAG_ROWS - 1) / DIAG_ROWS;
  const unsigned grid = (unsigned)(bc * G * nrb * nhb);
  ssd_yoff_fwd_kernel<N, P><<<grid, 256, 0, stream>>>(
      (const short*)C, (const short*)prev, (short*)yoff, H, G, Q, sC, nrb, HB,
      nhb);
}

template <int N, int P>
static void launch_yd(const void* dyoff, const void* C, void* dprev,
                      long long bc, int H, int G, int Q, long long sC, int HB,
                      int nhb, hipStream_t stream) {
  const unsigned grid = (unsigned)(bc * G * nhb);
  ssd_yoff_dprev_kernel<N, P><<<grid, 256, 0, stream>>>(
      (const short*)dyoff, (const short*)C, (short*)dprev, H, G, Q, sC, HB,
      nhb);
}

template <int N, int P>
static void launch_yc(const void* dyoff, const void* prev, float* part,
                      long long bc, int H, int G, int Q, int nhb,
                      hipStream_t stream) {
  const int nrb = (Q + DIAG_ROWS - 1) / DIAG_ROWS;
  const unsigned grid = (unsigned)(bc * G * nrb * nhb);
  ssd_yoff_dC_kernel<N, P><<<grid, 256, 0, stream>>>(
      (const short*)dyoff, (const short*)prev, part, H, G, Q, bc * Q, nrb,
      nhb);
}

extern "C" {

// Heads per workgroup: `cap`, halved while the grid stays under `wgs`
// workgroups (two per compute unit of the device). `base` = workgroups per
// head block. Returns the number of head blocks per group and stores the
// block size.
int ssd_yoff_plan(long long base, int rep, int cap, int wgs, int* HB) {
  int hb = rep < cap ? rep : cap;
  while (hb > 1 && base * ((rep + hb - 1) / hb) < wgs) hb = (hb + 1) / 2;
  *HB = hb;
  return (rep + hb - 1) / hb;
}

// most heads a dprev workgroup holds: its accumulators persist over the
// chunk's tiles
int ssd_yoff_dprev_cap(int N, int P) {
  const int ni = N < 32 ? 32 : N;
  const int c = 32768 / (ni * P);
  return c < 8 ? c : 8;
}

#define YOFF_CASES(CALL) \
  CALL(16, 32);          \
  CALL(16, 64);          \
  CALL(32, 64);          \
  CALL(64, 64);          \
  CALL(128, 32);         \
  CALL(128, 64)

// ssd_diag_supported() and the lists below disagree: the output would stay
// uninitialised
static void yoff_no_kernel(const char* what, int N, int P) {
  fprintf(stderr, "%s: no kernel for N = %d, P = %d\n", what, N, P);
  abort();
}

// (N, P) as ssd_diag_supported; shapes are checked by the binding.
void launch_ssd_yoff_fwd(const void* C, const void* prev, void* yoff,
                         long long bc, int H, int G, int P, int N, int Q,
                         long long sC, int HB, int nhb, hipStream_t stream) {
#define YF_CASE(NN, PP)       \
  if (N == NN && P == PP)     \
  return launch_yf<NN, PP>(C, prev, yoff, bc, H, G, Q, sC, HB, nhb, stream)
  YOFF_CASES(YF_CASE);
#undef YF_CASE
  yoff_no_kernel("launch_ssd_yoff_fwd", N, P);
}

// HB <= ssd_yoff_dprev_cap(N, P)
void launch_ssd_yoff_dprev(const void* dyoff, const void* C, void* dprev,
                           long long bc, int H, int G, int P, int N, int Q,
                           long long sC, int HB, int nhb,
                           hipStream_t stream) {
#define YD_CASE(NN, PP)       \
  if (N == NN && P == PP)     \
  return launch_yd<NN, PP>(dyoff, C, dprev, bc, H, G, Q, sC, HB, nhb, stream)
  YOFF_CASES(YD_CASE);
#undef YD_CASE
  yoff_no_kernel("launch_ssd_yoff_dprev", N, P);
}

// part (nhb, bc*Q, G*N) fp32, 1 <= nhb <= H/G
void launch_ssd_yoff_dC(const void* dyoff, const void* prev, float* part,
                        long long bc, int H, int G, int P, int N, int Q,
                        int nhb, hipStream_t stream) {
#define YC_CASE(NN, PP)       \
  if (N == NN && P == PP)     \
  return launch_yc<NN, PP>(dyoff, prev, part, bc, H, G, Q, nhb, stream)
  YOFF_CASES(YC_CASE);
#undef YC_CASE
  yoff_no_kernel("launch_ssd_yoff_dC", N, P);
}
#undef YOFF_CASES

}  // extern "C"
