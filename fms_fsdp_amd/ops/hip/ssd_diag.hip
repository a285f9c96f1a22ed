// Fused intra-chunk term of the Mamba2 SSD (docs/kernels.md "SSD diag"):
//   y[n,i,p] = sum_{j<=i} (sum_k C[bc,i,g,k] B[bc,j,g,k])
//                         * exp(cs[n,i] - cs[n,j]) * xdt[n,j,p]
// n = bc*H + h, g = h / (H/G). Causal linear attention without a softmax:
// scores, decay and the second product stay in registers, so neither the
// (bc*G, Q, Q) scores nor the (n, Q, Q) sL tensor of the three-launch
// route (hipBLASLt einsum, ssd_sl_fwd_kernel, hipBLASLt bmm) reach HBM.
//
// One workgroup of 4 waves per (n, block of up to 128 chunk rows); wave w
// owns rows i0 + 32w .. +31, one row per lane column (lane&31), in the
// swapped layout of attention.hip:
//   S^T[j][i] = B C^T   A = B image rows (plain LDS reads), B operand = the
//                       lane's C row, N/16 fragments held for the sweep
//   p[r]      = S^T * exp2((cs_i - cs_j) log2e), select to 0 where masked
//   Y^T[p][i] += xdt^T[p][j] sL^T[j][i]   A = xdt image (transpose reads),
//                       B operand = pack_pT_chunk(p), no LDS round trip;
//                       p enters as bf16 high part + bf16 remainder
// Register r of a 32x32 D tile is key DROW(r, hb): four runs of four
// consecutive keys, so the cs_j of a lane's 16 registers are four
// ds_read_b128 of the staged dacs row.
//
// Keys arrive in 64-row tiles: B [64][N] and xdt [64][P] as the subtiled
// images of attn_frag.h, staged with coalesced 16-byte loads (a row of
// either operand is contiguous). A 32-key subtile wholly above the wave's
// rows, or (DOCMASK) wholly in front of its first document, is skipped
// wave-uniformly; the select runs only in subtiles that cross the
// diagonal or a document start of the wave.
//
// Masked entries are a SELECT to exact 0 after the exponential: above the
// diagonal cs_i - cs_j > 0 and exp2 may be inf. DOCMASK keeps (i, j) iff
// rel_start(i) <= j <= i, rel_start clamped where it is read, so no
// content of `start` moves an address or a loop bound.
#include "ssd_diag_frag.h"

template <int N, int P>
constexpr int diag_lds_bytes() {
  const int img = DIAG_KT * (N + P) * 2 + 256 * 4;       // images + cs row
  const int epi = 4 * 32 * (P * 2 + 16);                 // output transpose
  return img > epi ? img : epi;
}

template <int N, int P, bool DOCMASK>
__global__ __launch_bounds__(256, 2) void ssd_diag_fwd_kernel(
    const short* __restrict__ Cg, const short* __restrict__ Bg,
    const float* __restrict__ dacs, const short* __restrict__ xdt,
    short* __restrict__ y, int H, int G, int Q, long long sC, long long sB,
    int nrb, const int* __restrict__ start, int nc) {
  constexpr int NCH = N / 16;      // S^T k-chunks
  constexpr int NT = P / 32;       // 32-feature output tiles
  constexpr int BIMG = DIAG_KT * N * 2;
  constexpr int XIMG = DIAG_KT * P * 2;
  constexpr int ERS = P * 2 + 16;  // epilogue row stride: spreads the banks
  constexpr float LOG2E = 1.4426950408889634f;
  __shared__ __attribute__((aligned(128))) char smem[diag_lds_bytes<N, P>()];
  char* bimg = smem;
  char* ximg = smem + BIMG;
  float* csl = (float*)(smem + BIMG + XIMG);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;       // row owner inside the wave's 32 rows
  const int hb = lane >> 5;

  const long long n = blockIdx.x / nrb;            // bc*H + h
  const int rb = (int)(blockIdx.x % nrb);
  const long long bc = n / H;
  const int g = (int)(n % H) / (H / G);
  const int i0 = rb * DIAG_ROWS;
  const int qw = i0 + wid * 32;                    // wave's first row
  const bool live = qw < Q;                        // wave-uniform (Q % 32 == 0)
  const int my_i = qw + col;
  const int iend = min(Q, i0 + DIAG_ROWS);         // rows of this block
  const int ntiles = (iend + DIAG_KT - 1) / DIAG_KT;

  const short* cbase = Cg + bc * Q * sC + (long long)g * N;
  const short* bbase = Bg + bc * Q * sB + (long long)g * N;
  const short* xbase = xdt + n * Q * (long long)P;
  const float* csrow = dacs + n * Q;

  if (tid < Q) csl[tid] = csrow[tid];

  // the lane's C row as B-operand fragments, its cs and its document start
  bf16x8v cf[NCH];
  float ci = 0.f;
  int my_js = 0, w_lo = 0, w_hi = 0;
  if (live) {
    const short* cp = cbase + (long long)my_i * sC + hb * 8;
#pragma unroll
    for (int c = 0; c < NCH; ++c) cf[c] = *(const bf16x8v*)(cp + c * 16);
    ci = csrow[my_i];
    if constexpr (DOCMASK) {
      my_js = diag_rel_start(start, bc, my_i, Q, nc);
      w_lo = __builtin_amdgcn_readfirstlane(__shfl(my_js, 0, 64));
      w_hi = __builtin_amdgcn_readfirstlane(__shfl(my_js, 31, 64));
    }
  }

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x16)(0.f);

  // transpose-read base inside an xdt image: R4 = 16 row groups per column
  // block (2048 B), lane terms as attention.hip's tr_base
  const unsigned xtr = (unsigned)(unsigned long long)ximg +
                       (unsigned)((((lane & 15) * 8) ^ (16 * hb)) + hb * 256 +
                                  (col >> 4) * 2048);

  for (int tile = 0; tile < ntiles; ++tile) {
    const int kv0 = tile * DIAG_KT;
    __syncthreads();               // the previous tile's reads are done
    // ---- stage: 16-byte segments, consecutive threads along a row ----
#pragma unroll
    for (int s = tid; s < DIAG_KT * N / 8; s += 256) {
      const int key = s / (N / 8), c8 = (s % (N / 8)) * 8;
      if (kv0 + key < Q)
        *(f32x4*)(bimg + SUBT_OFF(key, c8, 16)) =
            *(const f32x4*)(bbase + (long long)(kv0 + key) * sB + c8);
    }
#pragma unroll
    for (int s = tid; s < DIAG_KT * P / 8; s += 256) {
      const int key = s / (P / 8), c8 = (s % (P / 8)) * 8;
      if (kv0 + key < Q)
        *(f32x4*)(ximg + SUBT_OFF(key, c8, 16)) =
            *(const f32x4*)(xbase + (long long)(kv0 + key) * P + c8);
    }
    __syncthreads();
    if (!live) continue;

#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int kv32 = kv0 + kt * 32;
      // wave-uniform skip: above the diagonal / in front of every document
      if (kv32 > qw + 31) break;
      if (DOCMASK && kv32 + 31 < w_lo) continue;

      f32x16 s = (f32x16)(0.f);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const bf16x8v a = *(const bf16x8v*)(
            bimg + SUBT_OFF(kt * 32 + col, c * 16 + hb * 8, 16));
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, cf[c], s, 0, 0, 0);
      }
      // the xdt fragments stream from LDS behind the decay arithmetic
      const unsigned xb = xtr + kt * 1024;
      U2x64 fr[NT][2];
#pragma unroll
      for (int t = 0; t < NT; ++t)
        tr_issue4<0, 128, 512, 640>(xb + t * 4096, fr[t][0], fr[t][1]);

      const bool partial = kv32 + 31 > qw || (DOCMASK && kv32 < w_hi);
      float p[16];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 cj = *(const f32x4*)(csl + kv32 + 8 * q4 + 4 * hb);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = q4 * 4 + e;
          const int j = kv32 + 8 * q4 + 4 * hb + e;      // = DROW(r, hb)
          float v = s[r] * exp2f((ci - cj.v[e]) * LOG2E);
          if (partial && (j > my_i || (DOCMASK && j < my_js))) v = 0.f;
          p[r] = v;
        }
      }
      const bf16x8v pb0 = pack_pT_chunk(p);
      const bf16x8v pb1 = pack_pT_chunk(p + 8);
      // One bf16 rounding is up to 2^-8 of a term, which a row of few terms
      // shows in y. The remainder p - bf16(p) goes through the same MFMA as
      // a second bf16 operand, so a term enters the sum to about 2^-16.
      // (A term that rounds to inf keeps remainder 0: y is inf, not NaN.)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float hi = bf2f(f2bf(p[r]));
        p[r] = fabsf(hi) < __builtin_inff() ? p[r] - hi : 0.f;
      }
      const bf16x8v pl0 = pack_pT_chunk(p);
      const bf16x8v pl1 = pack_pT_chunk(p + 8);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t == 0) {
#pragma unroll
          for (int u = 0; u < NT; ++u) tr_wait<0>(fr[u][0], fr[u][1]);
        }
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[t][0].v, pb0,
                                                         acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[t][1].v, pb1,
                                                         acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[t][0].v, pl0,
                                                         acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[t][1].v, pl1,
                                                         acc[t], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: acc is [p][i]; transpose through the now free LDS so
  // that the wave's 32 rows (one contiguous 32*P span of y) leave in
  // 16-byte stores ----
  __syncthreads();
  char* ep = smem + wid * (32 * ERS);
  if (live) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        bf16x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w.v[e] = f2bf(acc[t][q4 * 4 + e]);
        *(bf16x4*)(ep + col * ERS + (t * 32 + 8 * q4 + 4 * hb) * 2) = w;
      }
  }
  __syncthreads();
  if (live) {
    short* yw = y + (n * Q + qw) * (long long)P;
#pragma unroll
    for (int s = lane; s < 32 * P / 8; s += 64) {
      const int row = s / (P / 8), c8 = (s % (P / 8)) * 8;
      *(f32x4*)(yw + (long long)s * 8) =
          *(const f32x4*)(ep + row * ERS + c8 * 2);
    }
  }
}

template <int N, int P>
static void launch_diag(const void* C, const void* B, const float* dacs,
                        const void* xdt, void* y, long long nrows, int H,
                        int G, int Q, long long sC, long long sB,
                        const int* start, int nc, hipStream_t stream) {
  const int nrb = (Q + DIAG_ROWS - 1) / DIAG_ROWS;
  const unsigned grid = (unsigned)(nrows * nrb);
  if (start)
    ssd_diag_fwd_kernel<N, P, true><<<grid, 256, 0, stream>>>(
        (const short*)C, (const short*)B, dacs, (const short*)xdt, (short*)y,
        H, G, Q, sC, sB, nrb, start, nc);
  else
    ssd_diag_fwd_kernel<N, P, false><<<grid, 256, 0, stream>>>(
        (const short*)C, (const short*)B, dacs, (const short*)xdt, (short*)y,
        H, G, Q, sC, sB, nrb, nullptr, 1);
}

extern "C" {

// 1 if (N, P) has an instantiation below
int ssd_diag_supported(int N, int P) {
  return ((N == 16 || N == 128) && (P == 32 || P == 64)) ||
         ((N == 32 || N == 64) && P == 64);
}

// nrows = bc*H rows of dacs; C/B row strides in elements; `start` (flat
// (b*l) int32 document starts) selects the DOCMASK kernel, nc = chunks per
// row (read only when masked). Shapes are checked by the binding.
void launch_ssd_diag_fwd(const void* C, const void* B, const float* dacs,
                         const void* xdt, void* y, long long nrows, int H,
                         int G, int P, int N, int Q, long long sC,
                         long long sB, const int* start, int nc,
                         hipStream_t stream) {
#define DIAG_CASE(NN, PP)                                                   \
  if (N == NN && P == PP)                                                   \
    return launch_diag<NN, PP>(C, B, dacs, xdt, y, nrows, H, G, Q, sC, sB,  \
                               start, nc, stream)
  DIAG_CASE(16, 32);
  DIAG_CASE(16, 64);
  DIAG_CASE(32, 64);
  DIAG_CASE(64, 64);
  DIAG_CASE(128, 32);
  DIAG_CASE(128, 64);
#undef DIAG_CASE
}

}  // extern "C"
