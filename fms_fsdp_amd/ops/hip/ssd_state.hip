// Inter-chunk state chain of the Mamba2 SSD (docs/kernels.md
// "ssd_state.hip"): the chunk states as an MFMA kernel and the chunk-to-
// chunk recurrence as a sequential scan that starts from any state.
// m = bc*H + h with bc = b*nc + c, g = h / (H/G), G_c = dacs[m, Q-1].
//
// ---- ssd_chunk_state_kernel<N, P> --------------------------------------
//   S[m, k, p] = sum_{q < Q} B[bc*Q + q, g*N + k] * xdtd[m, q, p]
// Both operands are row-major with the contraction index q on the rows,
// so both MFMA operands are transpose reads (ds_read_b64_tr_b16) of the
// subtiled images ssd_diag_fwd_kernel stages; the A and B lane maps of
// 32x32x16 hold the same registers for such a fragment. The product is
// taken as S^T[p][k] (A = xdtd^T, B operand = B^T): a lane then owns one
// state row k and four runs of four consecutive p, which the epilogue
// turns into 16-byte stores through LDS as ssd_diag does.
//
// One workgroup of 4 waves per (bc, g, block of HB heads), head block
// fastest in the grid so that the blocks of a (bc, g) find B in L2. The
// output tile is NI x P (NI = max(N, 32): N = 16 pads the B image with
// zero columns); the waves split it into WK = min(4, NI/32) column blocks
// of 32 state rows times WP = min(4/WK, P/32) blocks of P/WP features;
// waves beyond WK*WP only help to stage. B is staged once per workgroup
// in 64-row tiles and the wave's B^T fragments (Q/16 of them, 4 VGPRs
// each) stay in registers across the heads of the block. Per head the
// whole xdtd chunk [Q][P] is staged as Q/64 images with coalesced 16-byte
// loads and every live wave runs Q/16 * TP MFMAs on it.
//
// ---- ssd_state_pass_fwd_kernel / ssd_state_pass_bwd_kernel --------------
//   Hc_{-1} = initial (or 0);  prev[b,c,h] = bf16(Hc_{c-1})
//   Hc_c = keep_c a_c Hc_{c-1} + S[b,c,h];  final = Hc_{nc-1}
// a_c = __expf(G_c); keep_c (document mask) = the document of the chunk's
// last token began before the chunk, a select to exact 0. A thread owns 8
// consecutive (k, p) elements of one (b, h) and keeps the fp32 carry in
// registers over the chunk loop; S and prev move as 16-byte accesses and
// the next chunk's loads are issued before the current arithmetic. The
// initial / final state is fp32 (b, H, P, N): the transposition against
// the (k, p) carry is eight strided scalar accesses per thread, once per
// call. The backward is the same loop in reverse:
//   gH_{nc-1} = dfinal (or 0); dS_c = bf16(gH_c)
//   dG_c = keep_c a_c sum_{k,p} gH_c prev_c
//   gH_{c-1} = dprev_c + keep_c a_c gH_c;  dinitial = gH_{-1}
// with the (k, p) sum reduced per workgroup (shuffles, then the waves'
// sums in a fixed order) into one fp32 partial per (block, b, c, h). No
// atomics: two calls give the same bits. No address or loop bound depends
// on array contents (`start` is clamped where it is read). 64-bit indexing.
#include <cstdio>
#include <cstdlib>

#include "ssd_diag_frag.h"

constexpr int CS_MAXQ = 256;       // largest chunk
constexpr int CS_MAXF = CS_MAXQ / 16;

template <int N, int P>
struct CSGeom {
  static constexpr int NI = N < 32 ? 32 : N;          // B image columns
  static constexpr int WK = NI / 32 < 4 ? NI / 32 : 4;
  static constexpr int WP = (4 / WK) < (P / 32) ? (4 / WK) : (P / 32);
  static constexpr int TP = P / 32 / WP;              // 32-feature tiles/wave
  static constexpr int PW = TP * 32;                  // features per wave
  static constexpr int ERS = PW * 2 + 16;             // epilogue row stride
  static constexpr int BIMG = DIAG_KT * NI * 2;
  static constexpr int EPI = 4 * 32 * ERS;
  static constexpr int R0 = BIMG > EPI ? BIMG : EPI;  // B image, then epilogue
  static constexpr int XT = DIAG_KT * P * 2;          // one xdtd image
  static constexpr int LDS = R0 + (CS_MAXQ / DIAG_KT) * XT;
};

template <int N, int P>
__global__ __launch_bounds__(256, 2) void ssd_chunk_state_kernel(
    const short* __restrict__ Bg, const short* __restrict__ xdtd,
    short* __restrict__ S, int H, int G, int Q, long long sB, int HB,
    int nhb) {
  using Ge = CSGeom<N, P>;
  constexpr int TP = Ge::TP, PW = Ge::PW, ERS = Ge::ERS, XT = Ge::XT;
  static_assert(N % 16 == 0 && P % 32 == 0 && Ge::NI <= 128, "tile shape");
  __shared__ __attribute__((aligned(128))) char smem[Ge::LDS];
  char* bimg = smem;
  char* ximg = smem + Ge::R0;

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
  const int r1 = min(rep, r0 + HB);

  const short* bbase = Bg + bc * Q * sB + (long long)g * N;
  const int ntiles = (Q + DIAG_KT - 1) / DIAG_KT;

  // lane terms of a transpose read (ssd_diag's xtr): R4 = 16 row groups
  // per 16-column block (2048 B)
  const unsigned ltr = (unsigned)((((lane & 15) * 8) ^ (16 * hb)) + hb * 256 +
                                  (col >> 4) * 2048);

  if constexpr (N < Ge::NI) {     // zero the pad columns once
    for (int s = tid; s < Ge::BIMG / 16; s += 256)
      *(f32x4*)(bimg + s * 16) = f32x4{{0.f, 0.f, 0.f, 0.f}};
  }

  // ---- B: staged tile by tile, the wave's B^T fragments stay ----
  bf16x8v bfr[CS_MAXF];
#pragma unroll
  for (int f = 0; f < CS_MAXF; ++f) bfr[f] = (bf16x8v)(0);
  const unsigned btr = (unsigned)(unsigned long long)bimg + ltr + kb * 4096;
#pragma unroll
  for (int tile = 0; tile < CS_MAXQ / DIAG_KT; ++tile) {
    if (tile < ntiles) {
      const int kv0 = tile * DIAG_KT;
      __syncthreads();
#pragma unroll
      for (int s = tid; s < DIAG_KT * N / 8; s += 256) {
        const int key = s / (N / 8), c8 = (s % (N / 8)) * 8;
        if (kv0 + key < Q)
          *(f32x4*)(bimg + SUBT_OFF(key, c8, 16)) =
              *(const f32x4*)(bbase + (long long)(kv0 + key) * sB + c8);
      }
      __syncthreads();
      if (live) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          if (kv0 + kt * 32 < Q) {
            U2x64 f0, f1;
            tr_issue4<0, 128, 512, 640>(btr + kt * 1024, f0, f1);
            tr_wait<0>(f0, f1);
            bfr[tile * 4 + kt * 2] = f0.v;
            bfr[tile * 4 + kt * 2 + 1] = f1.v;
          }
        }
      }
    }
  }

  const unsigned xtr = (unsigned)(unsigned long long)ximg + ltr;
  char* ep = smem + wid * (32 * ERS);

  for (int r = r0; r < r1; ++r) {
    const long long m = bc * H + (long long)g * rep + r;
    const short* xbase = xdtd + m * Q * (long long)P;
    __syncthreads();     // B fragments / the previous head's reads are done
    for (int s = tid; s < Q * (P / 8); s += 256) {
      const int q = s / (P / 8), c8 = (s % (P / 8)) * 8;
      *(f32x4*)(ximg + (q / DIAG_KT) * XT + SUBT_OFF(q % DIAG_KT, c8, 16)) =
          *(const f32x4*)(xbase + (long long)s * 8);
    }
    __syncthreads();

    f32x16 acc[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) acc[t] = (f32x16)(0.f);
    if (live) {
#pragma unroll
      for (int k32 = 0; k32 < CS_MAXQ / 32; ++k32) {
        if (k32 * 32 < Q) {
          const unsigned xb = xtr + (k32 >> 1) * XT + (k32 & 1) * 1024;
          U2x64 fr[TP][2];
#pragma unroll
          for (int t = 0; t < TP; ++t)
            tr_issue4<0, 128, 512, 640>(xb + (pb * TP + t) * 4096, fr[t][0],
                                        fr[t][1]);
#pragma unroll
          for (int t = 0; t < TP; ++t) {
            if (t == 0) {
#pragma unroll
              for (int u = 0; u < TP; ++u) tr_wait<0>(fr[u][0], fr[u][1]);
            }
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                fr[t][0].v, bfr[k32 * 2], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                fr[t][1].v, bfr[k32 * 2 + 1], acc[t], 0, 0, 0);
          }
        }
      }
      // acc is [p][k]: lane = state row k, registers = features
#pragma unroll
      for (int t = 0; t < TP; ++t)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          bf16x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v.v[e] = f2bf(acc[t][q4 * 4 + e]);
          *(bf16x4*)(ep + col * ERS + (t * 32 + 8 * q4 + 4 * hb) * 2) = v;
        }
    }
    __syncthreads();
    if (live) {
      short* sw = S + (m * N + kb * 32) * (long long)P + pb * PW;
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

// keep_c of the document mask: the (clamped) document start of the chunk's
// last token lies before the chunk
__device__ __forceinline__ bool pass_keep(const int* __restrict__ start,
                                          long long b, int c, int Q, int nc) {
  const int last = (c + 1) * Q - 1;
  const int s = start[(b * nc + c) * (long long)Q + Q - 1];
  return min(max(s, 0), last) <= c * Q - 1;
}

// (b, H, P, N) fp32 element of carry slot (k, p0 + e)
#define PASS_ST(bh, k, p) (((bh) * (long long)P + (p)) * N + (k))

__global__ __launch_bounds__(256) void ssd_state_pass_fwd_kernel(
    const short* __restrict__ S, const float* __restrict__ dacs,
    const float* __restrict__ init, short* __restrict__ prev,
    float* __restrict__ fin, const int* __restrict__ start, int nc, int H,
    int P, int N, int Q, int nblk) {
  const long long bh = blockIdx.x / nblk;
  const int j = (int)(blockIdx.x % nblk) * blockDim.x + threadIdx.x;
  const long long b = bh / H;
  const int h = (int)(bh % H);
  const int e0 = j * 8;                 // first of 8 consecutive (k, p)
  const int k = e0 / P, p0 = e0 % P;
  const long long NP = (long long)N * P;

  float carry[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
    carry[e] = init ? init[PASS_ST(bh, k, p0 + e)] : 0.f;

  long long m = (b * nc) * H + h;       // row of chunk 0
  bf16x8 sn = *(const bf16x8*)(S + m * NP + e0);
  float gn = dacs[m * Q + Q - 1];
  for (int c = 0; c < nc; ++c) {
    const bf16x8 sc = sn;
    const float gc = gn;
    const long long mn = c + 1 < nc ? m + H : m;
    sn = *(const bf16x8*)(S + mn * NP + e0);
    gn = dacs[mn * Q + Q - 1];
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = f2bf(carry[e]);
    *(bf16x8*)(prev + m * NP + e0) = o;
    const bool keep = start ? pass_keep(start, b, c, Q, nc) : true;
    const float a = __expf(gc);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float s = bf2f(sc.v[e]);
      carry[e] = keep ? fmaf(a, carry[e], s) : s;
    }
    m = mn;
  }
  if (fin) {
#pragma unroll
    for (int e = 0; e < 8; ++e) fin[PASS_ST(bh, k, p0 + e)] = carry[e];
  }
}

__global__ __launch_bounds__(256) void ssd_state_pass_bwd_kernel(
    const short* __restrict__ dprev, const float* __restrict__ dfin,
    const short* __restrict__ prev, const float* __restrict__ dacs,
    short* __restrict__ dS, float* __restrict__ dGp, float* __restrict__ dinit,
    const int* __restrict__ start, long long nb, int nc, int H, int P, int N,
    int Q, int nblk) {
  __shared__ float red[2][4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  const long long bh = blockIdx.x / nblk;
  const int blk = (int)(blockIdx.x % nblk);
  const int j = blk * blockDim.x + threadIdx.x;
  const long long b = bh / H;
  const int h = (int)(bh % H);
  const int e0 = j * 8;
  const int k = e0 / P, p0 = e0 % P;
  const long long NP = (long long)N * P;

  float gH[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
    gH[e] = dfin ? dfin[PASS_ST(bh, k, p0 + e)] : 0.f;

  long long m = (b * nc + (nc - 1)) * H + h;       // row of the last chunk
  bf16x8 dn = *(const bf16x8*)(dprev + m * NP + e0);
  bf16x8 pn = *(const bf16x8*)(prev + m * NP + e0);
  float gn = dacs[m * Q + Q - 1];
  for (int c = nc - 1; c >= 0; --c) {
    const bf16x8 dc = dn, pc = pn;
    const float gc = gn;
    const long long mn = c > 0 ? m - H : m;
    dn = *(const bf16x8*)(dprev + mn * NP + e0);
    pn = *(const bf16x8*)(prev + mn * NP + e0);
    gn = dacs[mn * Q + Q - 1];
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = f2bf(gH[e]);
    *(bf16x8*)(dS + m * NP + e0) = o;
    const bool keep = start ? pass_keep(start, b, c, Q, nc) : true;
    const float a = __expf(gc);
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      dot = fmaf(gH[e], bf2f(pc.v[e]), dot);
      const float d = bf2f(dc.v[e]);
      gH[e] = keep ? fmaf(a, gH[e], d) : d;
    }
    dot = wave_reduce_sum(dot);
    if (lane == 0) red[c & 1][wid] = dot;
    __syncthreads();                  // buffers alternate: one barrier a chunk
    if (threadIdx.x == 0) {
      float t = red[c & 1][0];
      for (int i = 1; i < nw; ++i) t += red[c & 1][i];
      dGp[((blk * nb + b) * nc + c) * H + h] = keep ? a * t : 0.f;
    }
    m = mn;
  }
  if (dinit) {
#pragma unroll
    for (int e = 0; e < 8; ++e) dinit[PASS_ST(bh, k, p0 + e)] = gH[e];
  }
}
#undef PASS_ST

template <int N, int P>
static void launch_cs(const void* B, const void* xdtd, void* S, long long bc,
                      int H, int G, int Q, long long sB, int HB, int nhb,
                      hipStream_t stream) {
  const unsigned grid = (unsigned)(bc * G * nhb);
  ssd_chunk_state_kernel<N, P><<<grid, 256, 0, stream>>>(
      (const short*)B, (const short*)xdtd, (short*)S, H, G, Q, sB, HB, nhb);
}

extern "C" {

// Heads per workgroup: 8, halved while the grid stays under 512 workgroups
// (two per compute unit), so that a short batch still fills the chip.
// Returns the number of head blocks per group and stores the block size.
int ssd_chunk_state_plan(long long bcg, int rep, int* HB) {
  int hb = rep < 8 ? rep : 8;
  while (hb > 1 && bcg * ((rep + hb - 1) / hb) < 512) hb = (hb + 1) / 2;
  *HB = hb;
  return (rep + hb - 1) / hb;
}

// (N, P) as ssd_diag_supported; shapes are checked by the binding.
void launch_ssd_chunk_state(const void* B, const void* xdtd, void* S,
                            long long bc, int H, int G, int P, int N, int Q,
                            long long sB, int HB, int nhb,
                            hipStream_t stream) {
#define CS_CASE(NN, PP)                                                      \
  if (N == NN && P == PP)                                                    \
    return launch_cs<NN, PP>(B, xdtd, S, bc, H, G, Q, sB, HB, nhb, stream)
  CS_CASE(16, 32);
  CS_CASE(16, 64);
  CS_CASE(32, 64);
  CS_CASE(64, 64);
  CS_CASE(128, 32);
  CS_CASE(128, 64);
#undef CS_CASE
  // ssd_diag_supported() and the list above disagree: the output would
  // stay uninitialised
  fprintf(stderr, "launch_ssd_chunk_state: no kernel for N = %d, P = %d\n", N,
          P);
  abort();
}

// threads per workgroup of the state pass: N*P/8 threads serve one (b, h)
int ssd_state_pass_block(int N, int P) {
  const int ept = N * P / 8;
  return ept % 256 == 0 ? 256 : 64;
}

void launch_ssd_state_pass_fwd(const void* S, const float* dacs,
                               const float* init, void* prev, float* fin,
                               const int* start, long long b, int nc, int H,
                               int P, int N, int Q, hipStream_t stream) {
  const int tb = ssd_state_pass_block(N, P);
  const int nblk = N * P / 8 / tb;
  ssd_state_pass_fwd_kernel<<<(unsigned)(b * H * nblk), tb, 0, stream>>>(
      (const short*)S, dacs, init, (short*)prev, fin, start, nc, H, P, N, Q,
      nblk);
}

// dGp: (N*P/8/block, b, nc, H) fp32 partials
void launch_ssd_state_pass_bwd(const void* dprev, const float* dfin,
                               const void* prev, const float* dacs, void* dS,
                               float* dGp, float* dinit, const int* start,
                               long long b, int nc, int H, int P, int N, int Q,
                               hipStream_t stream) {
  const int tb = ssd_state_pass_block(N, P);
  const int nblk = N * P / 8 / tb;
  ssd_state_pass_bwd_kernel<<<(unsigned)(b * H * nblk), tb, 0, stream>>>(
      (const short*)dprev, dfin, (const short*)prev, dacs, (short*)dS, dGp,
      dinit, start, b, nc, H, P, N, Q, nblk);
}

}  // extern "C"
