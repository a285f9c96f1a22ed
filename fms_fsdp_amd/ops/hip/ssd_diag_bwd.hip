// Fused backward of the intra-chunk SSD term (docs/kernels.md
// "ssd_diag_bwd.hip — fused backward of the intra-chunk term"). With S = C B^T per group, L[i,j] = exp(cs_i - cs_j) kept iff
// rel_start(i) <= j <= i, M = S∘L, Y = M X (X = xdt):
//   dM = dY X^T      dX = M^T dY      dS_h = dM∘L      Gm = dM∘M
//   dcs[i] = sum_j Gm[i,j] - sum_i' Gm[i',i]
//   dC = sum_{h in g} dS_h B        dB = sum_{h in g} dS_h^T C
// None of S, L, M, dM, dS, Gm reaches HBM: one kernel body, launched twice.
//
//                 row side (KEYSIDE = false)    key side (KEYSIDE = true)
//   lane owns     chunk row i (ssd_diag.hip)    key j (attention's keylane)
//   own operands  C row, dY row                 B row, X row
//   swept images  B [64][N], X [64][P]          C [64][N], dY [64][P]
//   sweep         j = 0 .. block's last row     i = block's first key .. Q
//   chain 1       S^T[j][i]                     S[i][j]
//   chain 2       dM^T[j][i] = X dY^T           dM[i][j] = dY X^T
//   chain 3       dC^T[k][i] += B^T dS^T        dB^T[k][j] += C^T dS
//   chain 4       -                             dX^T[p][j] += dY^T M
//   sum of Gm     over j -> drow[n,i]           over i -> ddacs = drow - sum
// In both, register r of a D tile is the swept index DROW(r, hb) and the
// lane column is the own index, so chains 1/2 take plain image rows as A
// and the lane's own fragments as B operand, and chains 3/4 take transpose
// reads of the same images as A and pack_pT_chunk of the lane's registers
// as B operand. Both sides recompute S and dM (7 MFMA chains, not 5).
//
// One workgroup of 4 waves per (bc, group, block of up to 128 own rows, head
// block); the head block is the fastest grid index, so the workgroups of a
// group run together and share C/B in L2. A workgroup loops over its heads
// (outer loop) and the swept 64-row tiles (inner loop, the forward's
// staging). The dC^T / dB^T accumulators persist across the head loop: the
// group sum happens in registers, each head's dS rounded to bf16 once. A
// workgroup writes its fp32 tile to the partial of its head block; the
// caller sums the nhb partials, so there are no atomics.
//
// The decay is exp2 of the difference on the fp32 accumulators, then a
// SELECT to exact 0 where masked (on the masked side the exponent is
// positive and may be inf). rel_start is clamped where it is read; no
// content of `start` moves an address or a loop bound, it only skips
// arithmetic (document starts do not decrease along a row).
#include <cstdio>
#include <cstdlib>

#include "ssd_diag_frag.h"

template <int N, int P, bool KEYSIDE>
constexpr int diag_bwd_tile_bytes() {
  const int img = DIAG_KT * (N + P) * 2;
  const int epi = KEYSIDE ? 4 * 32 * (P * 2 + 16) : 0;   // dX transpose
  return img > epi ? img : epi;
}

// acc[t] += A(t) * (b0 | b1): A fragments of 32-feature block t stream from
// a subtiled image by transpose reads, one block ahead of the MFMAs
template <int NTT>
__device__ __forceinline__ void diag_bwd_chain(f32x16 (&acc)[NTT],
                                               unsigned base, bf16x8v b0,
                                               bf16x8v b1) {
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
    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][1].v, b1, acc[t],
                                                     0, 0, 0);
  }
}

// part: this side's partials (nhb, rows, G*N) fp32, dC on the row side, dB
// on the key side. ddacs (bc*H, Q): the row side writes the row sums of Gm
// into it, the key side (launched second) replaces them by the result.
template <int N, int P, bool KEYSIDE, bool DOCMASK>
__global__ __launch_bounds__(256, 2) void ssd_diag_bwd_kernel(
    const short* __restrict__ dy, const short* __restrict__ Cg,
    const short* __restrict__ Bg, const float* __restrict__ dacs,
    const short* __restrict__ xdt, float* __restrict__ part,
    float* __restrict__ ddacs, short* __restrict__ dxdt, int H, int G, int Q,
    long long sC, long long sB, long long rows, int nrb, int nhb,
    const int* __restrict__ start, int nc) {
  constexpr int NCH = N / 16;            // k-chunks of chain 1
  constexpr int PCH = P / 16;            // k-chunks of chain 2
  constexpr int NGT = (N + 31) / 32;     // 32-feature tiles of dC^T / dB^T
  constexpr int NT = P / 32;             // 32-feature tiles of dX^T
  constexpr int GIMG = DIAG_KT * N * 2;
  constexpr int TILEB = diag_bwd_tile_bytes<N, P, KEYSIDE>();
  constexpr int ERS = P * 2 + 16;        // epilogue row stride
  constexpr float LOG2E = 1.4426950408889634f;
  // The key side at N = 128 does not fit 256 registers with the own B row
  // in them (64 dB + 32 dX accumulators): its fragments then come from a
  // wave-private image with plain 16-byte reads.
  constexpr bool OWN_LDS = KEYSIDE && N == 128;
  constexpr int OIMG = OWN_LDS ? 32 * N * 2 : 0;
  __shared__ __attribute__((aligned(128))) char smem[TILEB + 2048 + 4 * OIMG];
  char* gimg = smem;                     // group image: B (row) / C (key)
  char* himg = smem + GIMG;              // head image: X (row) / dY (key)
  float* csl = (float*)(smem + TILEB);   // the head's cs row
  int* stl = (int*)(smem + TILEB + 1024);   // relative starts (key side)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;             // own index inside the wave's 32
  const int hb = lane >> 5;

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

  const int i0 = rb * DIAG_ROWS;
  const int qw = i0 + wid * 32;                      // wave's first own index
  const bool live = qw < Q;                          // wave-uniform
  const int my_o = qw + col;
  const int iend = min(Q, i0 + DIAG_ROWS);
  const int t_begin = KEYSIDE ? i0 / DIAG_KT : 0;
  const int t_end = ((KEYSIDE ? Q : iend) + DIAG_KT - 1) / DIAG_KT;

  const long long sO = KEYSIDE ? sB : sC, sS = KEYSIDE ? sC : sB;
  const short* ownbase = (KEYSIDE ? Bg : Cg) + bc * Q * sO + (long long)g * N;
  const short* swpbase = (KEYSIDE ? Cg : Bg) + bc * Q * sS + (long long)g * N;

  // the lane's own group row as B-operand fragments, constant over the heads
  // (or the wave's 32 own rows as a subtiled image, R4 = 8)
  bf16x8v of[OWN_LDS ? 1 : NCH];
  char* oimg = smem + TILEB + 2048 + (tid >> 6) * OIMG;
  int my_js = 0, w_lo = 0, w_hi = 0;
  if (live) {
    if constexpr (OWN_LDS) {
      for (int s = lane; s < 32 * N / 8; s += 64) {
        const int row = s / (N / 8), c8 = (s % (N / 8)) * 8;
        *(f32x4*)(oimg + SUBT_OFF(row, c8, 8)) =
            *(const f32x4*)(ownbase + (long long)(qw + row) * sO + c8);
      }
    } else {
      const short* op = ownbase + (long long)my_o * sO + hb * 8;
#pragma unroll
      for (int c = 0; c < NCH; ++c) of[c] = *(const bf16x8v*)(op + c * 16);
    }
    if constexpr (DOCMASK && !KEYSIDE) {
      my_js = diag_rel_start(start, bc, my_o, Q, nc);
      w_lo = __builtin_amdgcn_readfirstlane(__shfl(my_js, 0, 64));
      w_hi = __builtin_amdgcn_readfirstlane(__shfl(my_js, 31, 64));
    }
  }
  if constexpr (DOCMASK && KEYSIDE) {
    if (tid < Q) stl[tid] = diag_rel_start(start, bc, tid, Q, nc);
  }

  f32x16 accG[NGT];
#pragma unroll
  for (int t = 0; t < NGT; ++t) accG[t] = (f32x16)(0.f);

  // transpose-read bases (ssd_diag.hip): R4 = 16 row groups per column
  // block (2048 B). N = 16 has one column block: both lane halves read it
  // and D rows 16..31 of chain 3 are never stored.
  const unsigned trl = (unsigned)((((lane & 15) * 8) ^ (16 * hb)) + hb * 256);
  const unsigned gtr = (unsigned)(unsigned long long)gimg + trl +
                       (N >= 32 ? (col >> 4) * 2048 : 0);
  const unsigned htr =
      (unsigned)(unsigned long long)himg + trl + (col >> 4) * 2048;

  for (int h = h_lo; h < h_hi; ++h) {
    const long long n = bc * H + h;
    const short* hown = (KEYSIDE ? xdt : dy) + n * Q * (long long)P;
    const short* hswp = (KEYSIDE ? dy : xdt) + n * Q * (long long)P;
    const float* csrow = dacs + n * Q;

    // the lane's own head row (dY / X) as B-operand fragments, and its cs
    bf16x8v hf[PCH];
    float co = 0.f;
    if (live) {
      const short* hp = hown + (long long)my_o * P + hb * 8;
#pragma unroll
      for (int c = 0; c < PCH; ++c) hf[c] = *(const bf16x8v*)(hp + c * 16);
      co = csrow[my_o];
    }
    f32x16 accX[KEYSIDE ? NT : 1];
    if constexpr (KEYSIDE) {
#pragma unroll
      for (int t = 0; t < NT; ++t) accX[t] = (f32x16)(0.f);
    }
    float gsum = 0.f;

    for (int tile = t_begin; tile < t_end; ++tile) {
      const int s0 = tile * DIAG_KT;
      __syncthreads();             // the previous tile's reads are done
      // the head's cs row rides along with every tile (1 KB, between the
      // same barriers): no first tile to tell apart
      if (tid < Q) csl[tid] = csrow[tid];
      // uniform 64-bit tile bases, 32-bit offsets per thread
      const short* gsrc = swpbase + (long long)s0 * sS;
      const short* hsrc = hswp + (long long)s0 * P;
#pragma unroll
      for (int s = tid; s < DIAG_KT * N / 8; s += 256) {
        const int row = s / (N / 8), c8 = (s % (N / 8)) * 8;
        if (s0 + row < Q)
          *(f32x4*)(gimg + SUBT_OFF(row, c8, 16)) =
              *(const f32x4*)(gsrc + (row * (int)sS + c8));
      }
#pragma unroll
      for (int s = tid; s < DIAG_KT * P / 8; s += 256) {
        const int row = s / (P / 8), c8 = (s % (P / 8)) * 8;
        if (s0 + row < Q)
          *(f32x4*)(himg + SUBT_OFF(row, c8, 16)) =
              *(const f32x4*)(hsrc + (row * P + c8));
      }
      __syncthreads();
      if (!live) continue;

#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const int s32 = s0 + kt * 32;
        // wave-uniform skips: the dead side of the diagonal, or no row of
        // the subtile shares a document with a key of the wave
        bool partial;
        if constexpr (KEYSIDE) {
          if (s32 >= Q) break;
          if (s32 + 31 < qw) continue;
          partial = s32 < qw + 31;
          if constexpr (DOCMASK) {
            if (__builtin_amdgcn_readfirstlane(stl[s32]) > qw + 31) continue;
            partial |= __builtin_amdgcn_readfirstlane(stl[s32 + 31]) > qw;
          }
        } else {
          if (s32 > qw + 31) break;
          if (DOCMASK && s32 + 31 < w_lo) continue;
          partial = s32 + 31 > qw || (DOCMASK && s32 < w_hi);
        }

        f32x16 sc = (f32x16)(0.f), dm = (f32x16)(0.f);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const bf16x8v a = *(const bf16x8v*)(
              gimg + SUBT_OFF(kt * 32 + col, c * 16 + hb * 8, 16));
          const bf16x8v o =
              OWN_LDS ? *(const bf16x8v*)(oimg +
                                          SUBT_OFF(col, c * 16 + hb * 8, 8))
                      : of[OWN_LDS ? 0 : c];
          sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, o, sc, 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < PCH; ++c) {
          const bf16x8v a = *(const bf16x8v*)(
              himg + SUBT_OFF(kt * 32 + col, c * 16 + hb * 8, 16));
          dm = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hf[c], dm, 0, 0, 0);
        }

        float ds[16], mm[KEYSIDE ? 16 : 1];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int sw4 = s32 + 8 * q4 + 4 * hb;         // = DROW(4 q4, hb)
          const f32x4 cw = *(const f32x4*)(csl + sw4);
          int st4[4] = {0, 0, 0, 0};
          if constexpr (DOCMASK && KEYSIDE) {
            const int4 v = *(const int4*)(stl + sw4);
            st4[0] = v.x, st4[1] = v.y, st4[2] = v.z, st4[3] = v.w;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = q4 * 4 + e;
            const int sw = sw4 + e;
            const float d = KEYSIDE ? cw.v[e] - co : co - cw.v[e];
            const float L = exp2f(d * LOG2E);
            float dsv = dm[r] * L, mv = sc[r] * L;
            const bool dead =
                KEYSIDE ? (my_o > sw || (DOCMASK && my_o < st4[e]))
                        : (sw > my_o || (DOCMASK && sw < my_js));
            if (partial && dead) dsv = 0.f, mv = 0.f;
            ds[r] = dsv;
            gsum += dm[r] * mv;
            if constexpr (KEYSIDE) mm[r] = mv;
          }
        }
        const unsigned sub = kt * 1024;
        diag_bwd_chain<NGT>(accG, gtr + sub, pack_pT_chunk(ds),
                            pack_pT_chunk(ds + 8));
        if constexpr (KEYSIDE)
          diag_bwd_chain<NT>(accX, htr + sub, pack_pT_chunk(mm),
                             pack_pT_chunk(mm + 8));
      }
    }

    // ---- the head's outputs ----
    if (live) {
      const float tot = gsum + __shfl_xor(gsum, 32, 64);
      float* dp = ddacs + n * Q + my_o;
      if (hb == 0) *dp = KEYSIDE ? *dp - tot : tot;
    }
    if constexpr (KEYSIDE) {
      // accX is [p][j]: transpose through the now free LDS so that the
      // wave's 32 rows of dxdt leave in 16-byte stores (ssd_diag.hip)
      __syncthreads();
      char* ep = smem + wid * (32 * ERS);
      if (live) {
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
      if (live) {
        short* xw = dxdt + (n * Q + qw) * (long long)P;
#pragma unroll
        for (int s = lane; s < 32 * P / 8; s += 64) {
          const int row = s / (P / 8), c8 = (s % (P / 8)) * 8;
          *(f32x4*)(xw + (long long)s * 8) =
              *(const f32x4*)(ep + row * ERS + c8 * 2);
        }
      }
    }
  }

  // ---- the group tile: accG is [k][own], four registers = four
  // consecutive k of the lane's own row, one 16-byte store each ----
  if (live) {
    const long long prow = (long long)hbk * rows + bc * Q + my_o;
    float* pw = part + prow * ((long long)G * N) + (long long)g * N;
#pragma unroll
    for (int t = 0; t < NGT; ++t)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int k = t * 32 + 8 * q4 + 4 * hb;
        if (k < N) {
          f32x4 w;
#pragma unroll
          for (int e = 0; e < 4; ++e) w.v[e] = accG[t][q4 * 4 + e];
          *(f32x4*)(pw + k) = w;
        }
      }
  }
}

template <int N, int P>
static void launch_diag_bwd(const void* dy, const void* C, const void* B,
                            const float* dacs, const void* xdt, float* dCp,
                            float* dBp, float* ddacs, void* dxdt,
                            long long rows, int H, int G, int Q, long long sC,
                            long long sB, int nhb, const int* start, int nc,
                            hipStream_t stream) {
  const int nrb = (Q + DIAG_ROWS - 1) / DIAG_ROWS;
  const unsigned grid = (unsigned)(rows / Q * G * nrb * nhb);
#define DIAG_BWD_LAUNCH(KS, DM, PART)                                        \
  ssd_diag_bwd_kernel<N, P, KS, DM><<<grid, 256, 0, stream>>>(               \
      (const short*)dy, (const short*)C, (const short*)B, dacs,              \
      (const short*)xdt, PART, ddacs, (short*)dxdt, H, G, Q, sC, sB, rows,   \
      nrb, nhb, start, nc)
  // the row side first: the key side reads its row sums from ddacs
  if (start) {
    DIAG_BWD_LAUNCH(false, true, dCp);
    DIAG_BWD_LAUNCH(true, true, dBp);
  } else {
    DIAG_BWD_LAUNCH(false, false, dCp);
    DIAG_BWD_LAUNCH(true, false, dBp);
  }
#undef DIAG_BWD_LAUNCH
}

extern "C" {

// Head blocks per group for head_blocks = 0: the smallest nhb <= rep whose
// grid of `base` * nhb workgroups reaches `per_cu` workgroups per CU
// (docs/performance.md has the measurement behind per_cu).
int ssd_diag_bwd_plan(long long base, int rep, int cus, int per_cu) {
  for (int nhb = 1; nhb < rep; ++nhb)
    if (base * nhb >= (long long)per_cu * cus) return nhb;
  return rep;
}

// rows = b*l rows of C / B; the shapes are those of launch_ssd_diag_fwd and
// are checked by the binding (row strides below 2^24 elements: a staged
// tile's rows are offset in 32 bits). dCp / dBp (nhb, rows, G*N) fp32, ddacs
// (rows/Q*H, Q) fp32, dxdt bf16 in xdt's layout.
void launch_ssd_diag_bwd(const void* dy, const void* C, const void* B,
                         const float* dacs, const void* xdt, float* dCp,
                         float* dBp, float* ddacs, void* dxdt, long long rows,
                         int H, int G, int P, int N, int Q, long long sC,
                         long long sB, int nhb, const int* start, int nc,
                         hipStream_t stream) {
#define DIAG_CASE(NN, PP)                                                    \
  if (N == NN && P == PP)                                                    \
    return launch_diag_bwd<NN, PP>(dy, C, B, dacs, xdt, dCp, dBp, ddacs,     \
                                   dxdt, rows, H, G, Q, sC, sB, nhb, start,  \
                                   nc, stream)
  DIAG_CASE(16, 32);
  DIAG_CASE(16, 64);
  DIAG_CASE(32, 64);
  DIAG_CASE(64, 64);
  DIAG_CASE(128, 32);
  DIAG_CASE(128, 64);
#undef DIAG_CASE
  // ssd_diag_supported() and the list above disagree: the outputs would
  // stay uninitialised
  fprintf(stderr, "launch_ssd_diag_bwd: no kernel for N = %d, P = %d\n", N,
          P);
  abort();
}

}  // extern "C"
