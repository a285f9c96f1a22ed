// Backward of the chunk states (docs/kernels.md "ssd_state_bwd.hip"): both
// gradients of
//   S[m, k, p] = sum_q B[bc*Q + q, g*N + k] * xdtd[m, q, p]
// (m = bc*H + h, g = h / (H/G)) from one staging of dS[m]:
//   dxdtd[m, q, p]        = sum_k B[bc*Q + q, g*N + k] * dS[m, k, p]
//   dB[bc*Q + q, g*N + k] = sum_{h in g} sum_p xdtd[m, q, p] * dS[m, k, p]
//
// One workgroup of 4 waves per (bc, g, block of up to 128 chunk rows q, head
// block), head block fastest in the grid so that the workgroups of a (bc, g)
// find B in L2. Wave w owns rows q0 + 32w .. +31 and the lane column is the
// own row q, as on ssd_diag_bwd's key side: the lane's B row (N/16
// fragments, constant over the heads) and its xdtd row of the head (P/16
// fragments) come straight from global as B-operand fragments. Waves past Q
// only help to stage.
//
// Per head dS[m] is staged once as an [N][P] subtiled image (64-row tiles,
// coalesced 16-byte loads) and serves both chains:
//   chain 1  dxdtd^T[p][q] = dS^T[p][k] B^T[k][q]   A = transpose reads
//   chain 2  dB^T[k][q]   += dS[k][p] xdtd^T[p][q]  A = plain 16-byte reads
// The dB^T accumulators persist across the head loop: the group sum happens
// in fp32 registers, and a workgroup stores its tile into the partial of
// its head block (the caller sums the nhb partials; no atomics). dxdtd^T is
// transposed through a wave-private LDS region beside the image, so that a
// head's 32 rows leave as one contiguous span of 16-byte stores; the span
// is written out behind the next head's first barrier, which makes two
// barriers per head instead of three.
//
// N = 16: the image's rows 16..31 are zeroed once, chain 1 runs its one
// 16-row MFMA, and rows 16..31 of chain 2's tile are never stored.
// No address or loop bound depends on array contents. 64-bit indexing.
#include <cstdio>
#include <cstdlib>

#include "ssd_diag_frag.h"

// acc[t] += A(t) * (b0 | b1): A fragments of 32-feature block t are
// transpose reads of the image at `base`, one block ahead of the MFMAs.
// BOTH = false (N = 16) uses only the first 16 image rows.
template <int NTT, bool BOTH>
__device__ __forceinline__ void csb_chain(f32x16 (&acc)[NTT], unsigned base,
                                          bf16x8v b0, bf16x8v b1) {
  U2x64 fr[2][2];
  tr_issue4<0, 128, 512, 640>(base, fr[0][0], fr[0][1]);
#pragma unroll
  for (int t = 0; t < NTT; ++t) {
    const int pp = t & 1;
    if (t + 1 < NTT) {
      tr_issue4<0, 128, 512, 640>(base + (t + 1) * 4096, fr[pp ^ 1][0],
                                  fr[pp ^ 1][1]);
      tr_wait<4>(fr[pp][0], fr[pp][1]);
    } else {
      tr_wait<0>(fr[pp][0], fr[pp][1]);
    }
    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][0].v, b0, acc[t],
                                                     0, 0, 0);
    if constexpr (BOTH)
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][1].v, b1,
                                                       acc[t], 0, 0, 0);
  }
}

// part (nhb, rows, G*N) fp32 with rows = bc*Q; dxdtd bf16 in xdtd's layout
template <int N, int P>
__global__ __launch_bounds__(256, 2) void ssd_chunk_state_bwd_kernel(
    const short* __restrict__ dS, const short* __restrict__ Bg,
    const short* __restrict__ xdtd, float* __restrict__ part,
    short* __restrict__ dxdtd, int H, int G, int Q, long long sB,
    long long rows, int nrb, int nhb) {
  constexpr int NCH = N / 16;            // k-chunks of chain 1
  constexpr int PCH = P / 16;            // k-chunks of chain 2
  constexpr int NKT = (N + 31) / 32;     // 32-row tiles of dB^T
  constexpr int NT = P / 32;             // 32-feature tiles of dxdtd^T
  constexpr int IMG = DIAG_KT * P * 2;   // one 64-row tile of the dS image
  constexpr int NIMG = (N + DIAG_KT - 1) / DIAG_KT;
  constexpr int ERS = P * 2 + 16;        // epilogue row stride
  static_assert(N % 16 == 0 && (N == 16 || N % 32 == 0) && P % 32 == 0,
                "tile shape");
  __shared__ __attribute__((aligned(128))) char smem[NIMG * IMG +
                                                     4 * 32 * ERS];
  char* simg = smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;             // own row inside the wave's 32
  const int hb = lane >> 5;
  char* ep = smem + NIMG * IMG + wid * (32 * ERS);

  unsigned rest = blockIdx.x;
  const int hbk = (int)(rest % (unsigned)nhb);
  rest /= (unsigned)nhb;
  const int rb = (int)(rest % (unsigned)nrb);
  rest /= (unsigned)nrb;
  const int g = (int)(rest % (unsigned)G);
  const long long bc = rest / (unsigned)G;
  const int rep = H / G;
  const int h_lo = g * rep + hbk * rep / nhb;        // uneven splits allowed
  const int h_hi = g * rep + (hbk + 1) * rep / nhb;

  const int qw = rb * DIAG_ROWS + wid * 32;          // wave's first own row
  const bool live = qw < Q;                          // wave-uniform
  const int my_q = qw + col;

  // the lane's own B row as B-operand fragments, constant over the heads
  bf16x8v bf[NCH];
  if (live) {
    const short* bp =
        Bg + (bc * Q + my_q) * sB + (long long)g * N + hb * 8;
#pragma unroll
    for (int c = 0; c < NCH; ++c) bf[c] = *(const bf16x8v*)(bp + c * 16);
  }
  if constexpr (N < 32) {          // rows N..31: read by chain 2, not staged
    for (int s = tid; s < (32 - N) * (P / 8); s += 256) {
      const int k = N + s / (P / 8), c8 = (s % (P / 8)) * 8;
      *(f32x4*)(simg + SUBT_OFF(k, c8, 16)) = f32x4{{0.f, 0.f, 0.f, 0.f}};
    }
  }

  f32x16 accB[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) accB[t] = (f32x16)(0.f);

  // transpose-read base (ssd_diag.hip): R4 = 16 row groups per 16-column
  // block (2048 B)
  const unsigned str = (unsigned)(unsigned long long)simg +
                       (unsigned)((((lane & 15) * 8) ^ (16 * hb)) + hb * 256 +
                                  (col >> 4) * 2048);

  // the wave's 32 rows of dxdtd[m] from its epilogue region
  auto flush = [&](long long m) {
    short* xw = dxdtd + (m * Q + qw) * (long long)P;
#pragma unroll
    for (int s = lane; s < 32 * P / 8; s += 64) {
      const int row = s / (P / 8), c8 = (s % (P / 8)) * 8;
      *(f32x4*)(xw + (long long)s * 8) =
          *(const f32x4*)(ep + row * ERS + c8 * 2);
    }
  };

  for (int h = h_lo; h < h_hi; ++h) {
    const long long m = bc * H + h;
    // the lane's own xdtd row of the head as B-operand fragments
    bf16x8v xf[PCH];
    if (live) {
      const short* xp = xdtd + (m * Q + my_q) * (long long)P + hb * 8;
#pragma unroll
      for (int c = 0; c < PCH; ++c) xf[c] = *(const bf16x8v*)(xp + c * 16);
    }
    __syncthreads();     // the previous head's image reads are done
    if (live && h > h_lo) flush(m - 1);
    const short* sbase = dS + m * ((long long)N * P);
#pragma unroll
    for (int s = tid; s < N * P / 8; s += 256) {
      const int k = s / (P / 8), c8 = (s % (P / 8)) * 8;
      *(f32x4*)(simg + (k / DIAG_KT) * IMG + SUBT_OFF(k % DIAG_KT, c8, 16)) =
          *(const f32x4*)(sbase + s * 8);
    }
    __syncthreads();
    if (!live) continue;

    // chain 1: dxdtd^T[p][q] over the 32-row blocks of the image
    f32x16 accX[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) accX[t] = (f32x16)(0.f);
#pragma unroll
    for (int kk = 0; kk < NKT; ++kk)
      csb_chain<NT, (N >= 32)>(accX, str + (kk >> 1) * IMG + (kk & 1) * 1024,
                               bf[N >= 32 ? 2 * kk : 0],
                               bf[N >= 32 ? 2 * kk + 1 : 0]);

    // chain 2: dB^T[k][q] += dS[k][p] xdtd^T[p][q], image row k on the lane
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const char* ib = simg + (t >> 1) * IMG;
#pragma unroll
      for (int c = 0; c < PCH; ++c) {
        const bf16x8v a = *(const bf16x8v*)(
            ib + SUBT_OFF((t & 1) * 32 + col, c * 16 + hb * 8, 16));
        accB[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xf[c], accB[t],
                                                          0, 0, 0);
      }
    }

    // accX is [p][q]: into the wave's epilogue region as [q][p]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        bf16x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w.v[e] = f2bf(accX[t][q4 * 4 + e]);
        *(bf16x4*)(ep + col * ERS + (t * 32 + 8 * q4 + 4 * hb) * 2) = w;
      }
  }
  __syncthreads();
  if (!live) return;
  flush(bc * H + h_hi - 1);

  // accB is [k][q]: four registers = four consecutive k of the lane's own
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
        for (int e = 0; e < 4; ++e) w.v[e] = accB[t][q4 * 4 + e];
        *(f32x4*)(pw + k) = w;
      }
    }
}

template <int N, int P>
static void launch_csb(const void* dS, const void* B, const void* xdtd,
                       float* part, void* dxdtd, long long bc, int H, int G,
                       int Q, long long sB, int nhb, hipStream_t stream) {
  const int nrb = (Q + DIAG_ROWS - 1) / DIAG_ROWS;
  const unsigned grid = (unsigned)(bc * G * nrb * nhb);
  ssd_chunk_state_bwd_kernel<N, P><<<grid, 256, 0, stream>>>(
      (const short*)dS, (const short*)B, (const short*)xdtd, part,
      (short*)dxdtd, H, G, Q, sB, bc * Q, nrb, nhb);
}

extern "C" {

// (N, P) as ssd_diag_supported; shapes are checked by the binding. dS
// (bc*H, N, P) and xdtd (bc*H, Q, P) bf16 contiguous, B (bc*Q, G*N) bf16 with
// row stride sB; part (nhb, bc*Q, G*N) fp32, 1 <= nhb <= H/G.
void launch_ssd_chunk_state_bwd(const void* dS, const void* B,
                                const void* xdtd, float* part, void* dxdtd,
                                long long bc, int H, int G, int P, int N,
                                int Q, long long sB, int nhb,
                                hipStream_t stream) {
#define CSB_CASE(NN, PP)                                                     \
  if (N == NN && P == PP)                                                    \
    return launch_csb<NN, PP>(dS, B, xdtd, part, dxdtd, bc, H, G, Q, sB,     \
                              nhb, stream)
  CSB_CASE(16, 32);
  CSB_CASE(16, 64);
  CSB_CASE(32, 64);
  CSB_CASE(64, 64);
  CSB_CASE(128, 32);
  CSB_CASE(128, 64);
#undef CSB_CASE
  // ssd_diag_supported() and the list above disagree: the outputs would
  // stay uninitialised
  fprintf(stderr, "launch_ssd_chunk_state_bwd: no kernel for N = %d, P = %d\n",
          N, P);
  abort();
}

}  // extern "C"
