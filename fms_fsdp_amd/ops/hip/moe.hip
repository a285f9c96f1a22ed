// Inference forward of the routed SwiGLU MoE MLP (docs/kernels.md
// "moe.hip"): routing, a stable counting sort of the (token, slot) pairs by
// expert, two grouped GEMMs over the sorted rows and the slot sum. No host
// sync, no per-expert launch, no atomics: two calls give the same bits.
//
//   ids, wts (T, k)      top-k of the fp32 softmax, renormalised to sum 1
//   row_pair (P_pad)     sorted position -> pair t*k + j, -1 = padding
//   tile_expert (tiles)  expert of a row tile of BM positions, -1 = unused
//   h (P_pad, H) bf16    silu(x[tok] wg[e]^T) * (x[tok] wu[e]^T), sorted rows
//   ys (T*k, emb) fp32   wts[pair] * (h[p] w2[e]^T) at row pair
//   out (T, emb) bf16    sum over the k slots of a token, rounded once
//
// ---- moe_route_kernel -----------------------------------------------------
// One thread per token, the nE <= 16 probabilities in registers. Top-k by
// repeated argmax with a strict compare: on equal values the lower expert
// index wins. An id is always a valid, not yet chosen expert, whatever the
// logits hold.
//
// ---- moe_hist_kernel / moe_scan_kernel / moe_scatter_kernel ---------------
// A workgroup owns 256 consecutive pairs, a wave 64 of them. Counts come
// from wave ballots: hist[block][e]. One workgroup turns them into each
// block's first position per expert, with every expert's segment starting
// at a multiple of BM, and writes tile_expert and the -1 of every padding
// position. The scatter repeats the ballots: position = the block's first
// position + the earlier waves' counts + the number of lower lanes of the
// wave with the same expert. Every term is a count, so the order inside an
// expert is the pair order (stable) and no result depends on timing. An id
// outside [0, nE) is clamped by both kernels alike.
//
// ---- moe_gemm_kernel<BM, GU> ----------------------------------------------
// D^T[n][p] = W[n][:] . act[p][:] with weight rows on the MFMA A operand and
// sorted rows on B (the attention forward's swapped layout): lane & 31 is
// the row p, a register quad of D holds 4 consecutive output columns. Both
// operands are contiguous along the reduction, which runs in BK = 64 steps:
// the step's act tile [BM][64] and weight tile [WR][64] are subtiled LDS
// images read with plain 16-byte fragment reads. Two image pairs alternate;
// the next step's tiles are fetched into registers before the current
// step's MFMAs and committed to the other pair before the step's single
// barrier. A -1 row, and a weight row past the matrix, stage zeros.
//   BM = 128: WR = 128, wave w owns rows 32w..32w+31 and all four 32-row
//             weight blocks (64 accumulator registers);
//   BM = 32:  WR = 256, the waves share the 32 rows, wave w owns two weight
//             blocks (32 accumulator registers).
//   GU  = true:  gate_up. act = x gathered by row_pair[p] / k. The first
//             half of the weight image holds gate rows n0.., the second up
//             rows H + n0.. (BN = WR/2 columns per workgroup); a wave's
//             blocks pair up, so g and u of a column meet in one register.
//             h = silu(g) * u in fp32 (swiglu_fwd_kernel's expression),
//             rounded once, 8-byte stores.
//   GU  = false: down. act = h, BN = WR rows of w2[e]; the epilogue scales
//             by wts[pair] and stores fp32 quads at row pair of ys.
// The expert base pointers arrive by value in the kernel arguments. A
// workgroup whose tile_expert is not an expert exits at once. row_pair
// entries are range-checked before they address anything. 64-bit addressing
// throughout.
//
// ---- moe_combine_kernel ---------------------------------------------------
// One thread per 8 output columns: the k slot rows summed in slot order in
// fp32, one rounding, 16-byte loads and stores.
#include <cstdio>
#include <cstdlib>

#include "attn_frag.h"
#include "moe_plan.h"

struct MoePtrs {
  const short* p[MOE_MAX_EXPERTS];
};

__global__ __launch_bounds__(256) void moe_route_kernel(
    const float* __restrict__ logits, int* __restrict__ ids,
    float* __restrict__ wts, long long T, int nE, int k) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const float* lg = logits + t * nE;
  float v[MOE_MAX_EXPERTS];
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < MOE_MAX_EXPERTS; ++e) {
    v[e] = e < nE ? lg[e] : -INFINITY;
    mx = fmaxf(mx, v[e]);
  }
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < MOE_MAX_EXPERTS; ++e) {
    v[e] = e < nE ? expf(v[e] - mx) : 0.f;
    sum += v[e];
  }
#pragma unroll
  for (int e = 0; e < MOE_MAX_EXPERTS; ++e) v[e] = v[e] / sum;

  unsigned taken = 0;
  int id[MOE_MAX_TOPK];
  float w[MOE_MAX_TOPK];
  float wsum = 0.f;
#pragma unroll
  for (int j = 0; j < MOE_MAX_TOPK; ++j) {
    if (j < k) {
      int best = -1;
      float bv = 0.f;
#pragma unroll
      for (int e = 0; e < MOE_MAX_EXPERTS; ++e)
        if (e < nE && !((taken >> e) & 1u) && (best < 0 || v[e] > bv)) {
          best = e;
          bv = v[e];
        }
      taken |= 1u << best;
      id[j] = best;
      w[j] = bv;
      wsum += bv;
    }
  }
#pragma unroll
  for (int j = 0; j < MOE_MAX_TOPK; ++j)
    if (j < k) {
      ids[t * k + j] = id[j];
      wts[t * k + j] = w[j] / wsum;
    }
}

// the pair's expert, clamped into [0, nE); -1 past the last pair
__device__ __forceinline__ int moe_pair_expert(const int* __restrict__ ids,
                                               long long p, long long npairs,
                                               int nE) {
  if (p >= npairs) return -1;
  return min(max(ids[p], 0), nE - 1);
}

// hist (nb, 16): pairs of block b routed to expert e
__global__ __launch_bounds__(256) void moe_hist_kernel(
    const int* __restrict__ ids, int* __restrict__ hist, long long npairs,
    int nE) {
  __shared__ int wc[4][MOE_MAX_EXPERTS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int id =
      moe_pair_expert(ids, (long long)blockIdx.x * 256 + tid, npairs, nE);
#pragma unroll
  for (int e = 0; e < MOE_MAX_EXPERTS; ++e) {
    const unsigned long long m = __ballot(id == e);
    if (lane == 0) wc[wid][e] = __popcll(m);
  }
  __syncthreads();
  if (tid < MOE_MAX_EXPERTS)
    hist[(long long)blockIdx.x * MOE_MAX_EXPERTS + tid] =
        wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
}

// One workgroup. hist becomes each block's first position per expert;
// tile_expert (ntiles) and the padding of row_pair (ntiles * BM) are
// written in full.
__global__ __launch_bounds__(256) void moe_scan_kernel(
    int* __restrict__ hist, int* __restrict__ row_pair,
    int* __restrict__ tile_expert, int nb, int nE, int BM, int ntiles) {
  __shared__ int part[16][MOE_MAX_EXPERTS + 1];
  __shared__ int cnt[MOE_MAX_EXPERTS];
  __shared__ int seg[MOE_MAX_EXPERTS + 1];
  const int tid = threadIdx.x;
  const int e = tid & 15, g = tid >> 4;
  const int per = (nb + 15) / 16;
  const int b_lo = min(nb, g * per), b_hi = min(nb, b_lo + per);

  int s = 0;
  for (int b = b_lo; b < b_hi; ++b) s += hist[b * MOE_MAX_EXPERTS + e];
  part[g][e] = s;
  __syncthreads();
  if (tid < MOE_MAX_EXPERTS) {
    int run = 0;
    for (int i = 0; i < 16; ++i) {
      const int c = part[i][tid];
      part[i][tid] = run;
      run += c;
    }
    cnt[tid] = run;
  }
  __syncthreads();
  if (tid == 0) {
    int a = 0;
    for (int i = 0; i < MOE_MAX_EXPERTS; ++i) {
      seg[i] = a;
      a += (cnt[i] + BM - 1) / BM * BM;
    }
    seg[MOE_MAX_EXPERTS] = a;
  }
  __syncthreads();

  int run = seg[e] + part[g][e];
  for (int b = b_lo; b < b_hi; ++b) {
    const int c = hist[b * MOE_MAX_EXPERTS + e];
    hist[b * MOE_MAX_EXPERTS + e] = run;
    run += c;
  }
  for (int t = tid; t < ntiles; t += 256) {
    const int p = t * BM;
    int ex = -1;
    for (int i = 0; i < nE; ++i)
      if (p >= seg[i] && p < seg[i + 1]) ex = i;
    tile_expert[t] = ex;
  }
  const int ppad = ntiles * BM;
  for (int i = 0; i < nE; ++i)
    for (int p = seg[i] + cnt[i] + tid; p < min(seg[i + 1], ppad); p += 256)
      row_pair[p] = -1;
  for (int p = seg[MOE_MAX_EXPERTS] + tid; p < ppad; p += 256)
    row_pair[p] = -1;
}

__global__ __launch_bounds__(256) void moe_scatter_kernel(
    const int* __restrict__ ids, const int* __restrict__ first,
    int* __restrict__ row_pair, long long npairs, int nE, int ppad) {
  __shared__ int wc[4][MOE_MAX_EXPERTS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long p = (long long)blockIdx.x * 256 + tid;
  const int id = moe_pair_expert(ids, p, npairs, nE);
  int rank = 0;
#pragma unroll
  for (int e = 0; e < MOE_MAX_EXPERTS; ++e) {
    const unsigned long long m = __ballot(id == e);
    if (lane == 0) wc[wid][e] = __popcll(m);
    if (id == e) rank = __popcll(m & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  if (id < 0) return;
  int pos = first[(long long)blockIdx.x * MOE_MAX_EXPERTS + id] + rank;
  for (int w = 0; w < wid; ++w) pos += wc[w][id];
  if (pos >= 0 && pos < ppad) row_pair[pos] = (int)p;
}

template <int BM, bool GU>
struct MoeGeom {
  static constexpr int BK = 64;                       // reduction step
  static constexpr int WR = BM == 128 ? 128 : 256;    // weight image rows
  static constexpr int BN = GU ? WR / 2 : WR;         // output columns
  static constexpr int NBLK = BM == 128 ? 4 : 2;      // weight blocks per wave
  static constexpr int XIMG = BM * BK * 2;
  static constexpr int WIMG = WR * BK * 2;
  static constexpr int PAIR = XIMG + WIMG;            // one step's images
  static constexpr int NXL = BM * 8 / 256;            // 16-byte loads/thread
  static constexpr int NWL = WR * 8 / 256;
  static constexpr int LDS = 2 * PAIR;
};

// the image block of a wave's accumulator a
template <int BM, bool GU>
__device__ __forceinline__ int moe_block(int a, int wid) {
  using Ge = MoeGeom<BM, GU>;
  constexpr int NG = GU ? Ge::NBLK / 2 : Ge::NBLK;   // blocks per half
  const int half = a / NG, i = a % NG;
  return half * (Ge::BN / 32) + (BM == 128 ? i : wid * NG + i);
}

template <int BM, bool GU>
__global__ __launch_bounds__(256, 2) void moe_gemm_kernel(
    MoePtrs wp, const short* __restrict__ act,
    const int* __restrict__ row_pair, const int* __restrict__ tile_expert,
    const float* __restrict__ wts, void* __restrict__ outp, int K, int NC,
    int npairs, int top_k, int nE, int ncol) {
  using Ge = MoeGeom<BM, GU>;
  constexpr int BK = Ge::BK, WR = Ge::WR, BN = Ge::BN, NBLK = Ge::NBLK;
  constexpr int NXL = Ge::NXL, NWL = Ge::NWL;
  static_assert(BM == 32 || BM == 128, "row tile");
  __shared__ __attribute__((aligned(128))) char smem[Ge::LDS];

  const int tile = blockIdx.x / ncol;
  const int ex = tile_expert[tile];
  if (ex < 0 || ex >= nE) return;                     // workgroup-uniform
  const int n0 = (blockIdx.x % ncol) * BN;
  const long long p0 = (long long)tile * BM;
  const short* wbase = wp.p[ex];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;
  const int hb = lane >> 5;

  // sources of the thread's 16-byte pieces, constant over the steps;
  // nullptr stages zeros
  const short* xs[NXL];
  const short* ws[NWL];
#pragma unroll
  for (int i = 0; i < NXL; ++i) {
    const int s = tid + i * 256;
    const int row = s >> 3, c8 = (s & 7) * 8;
    const int rp = row_pair[p0 + row];
    const bool ok = (unsigned)rp < (unsigned)npairs;
    const long long src = GU ? (long long)(rp / top_k) : p0 + row;
    xs[i] = ok ? act + src * K + c8 : nullptr;
  }
#pragma unroll
  for (int i = 0; i < NWL; ++i) {
    const int s = tid + i * 256;
    const int wr = s >> 3, c8 = (s & 7) * 8;
    const int half = wr / BN;                         // 1 = up rows
    const int c = n0 + (wr - half * BN);
    ws[i] = c < NC ? wbase + ((long long)half * NC + c) * K + c8 : nullptr;
  }

  f32x4v xr[NXL], wr_[NWL];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NXL; ++i)
      xr[i] = xs[i] ? *(const f32x4v*)(xs[i] + k0) : (f32x4v)(0.f);
#pragma unroll
    for (int i = 0; i < NWL; ++i)
      wr_[i] = ws[i] ? *(const f32x4v*)(ws[i] + k0) : (f32x4v)(0.f);
  };
  auto commit = [&](char* pair) {
#pragma unroll
    for (int i = 0; i < NXL; ++i) {
      const int s = tid + i * 256;
      *(f32x4v*)(pair + SUBT_OFF(s >> 3, (s & 7) * 8, BM / 4)) = xr[i];
    }
#pragma unroll
    for (int i = 0; i < NWL; ++i) {
      const int s = tid + i * 256;
      *(f32x4v*)(pair + Ge::XIMG + SUBT_OFF(s >> 3, (s & 7) * 8, WR / 4)) =
          wr_[i];
    }
  };

  f32x16 acc[NBLK];
#pragma unroll
  for (int a = 0; a < NBLK; ++a) acc[a] = (f32x16)(0.f);

  const int trow = (BM == 128 ? wid * 32 : 0) + col;  // the lane's own row
  fetch(0);
  commit(smem);
  __syncthreads();

  const int nk = K / BK;
  for (int ks = 0; ks < nk; ++ks) {
    const bool more = ks + 1 < nk;
    if (more) fetch((ks + 1) * BK);
    const char* ximg = smem + (ks & 1) * Ge::PAIR;
    const char* wimg = ximg + Ge::XIMG;
#pragma unroll
    for (int kc = 0; kc < BK / 16; ++kc) {
      const bf16x8v b = *(const bf16x8v*)(
          ximg + SUBT_OFF(trow, kc * 16 + hb * 8, BM / 4));
#pragma unroll
      for (int a = 0; a < NBLK; ++a) {
        const int wrow = moe_block<BM, GU>(a, wid) * 32 + col;
        const bf16x8v w = *(const bf16x8v*)(
            wimg + SUBT_OFF(wrow, kc * 16 + hb * 8, WR / 4));
        acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, b, acc[a], 0, 0, 0);
      }
    }
    if (more) commit(smem + ((ks + 1) & 1) * Ge::PAIR);
    __syncthreads();     // the other pair is complete, this one is free
  }

  // acc[a] is [column][row]: lane = own row, quads of consecutive columns
  const int rp = row_pair[p0 + trow];
  if (!((unsigned)rp < (unsigned)npairs)) return;
  if constexpr (GU) {
    constexpr int NG = NBLK / 2;
    short* hrow = (short*)outp + (p0 + trow) * NC;
#pragma unroll
    for (int a = 0; a < NG; ++a) {
      const int nb = n0 + moe_block<BM, GU>(a, wid) * 32;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int n = nb + 8 * q4 + 4 * hb;
        if (n < NC) {
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float gf = acc[a][q4 * 4 + e];
            const float s = 1.f / (1.f + __expf(-gf));
            o.v[e] = f2bf(gf * s * acc[NG + a][q4 * 4 + e]);
          }
          *(bf16x4*)(hrow + n) = o;
        }
      }
    }
  } else {
    const float wt = wts[rp];
    float* yrow = (float*)outp + (long long)rp * NC;
#pragma unroll
    for (int a = 0; a < NBLK; ++a) {
      const int nb = n0 + moe_block<BM, GU>(a, wid) * 32;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int n = nb + 8 * q4 + 4 * hb;
        if (n < NC) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o.v[e] = acc[a][q4 * 4 + e] * wt;
          *(f32x4*)(yrow + n) = o;
        }
      }
    }
  }
}

// ys (T*k, emb) fp32 -> out (T, emb) bf16, emb8 = emb / 8
__global__ __launch_bounds__(256) void moe_combine_kernel(
    const f32x4* __restrict__ ys, bf16x8* __restrict__ out, long long total,
    int emb8, int k) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long t = i / emb8;
  const int c = (int)(i % emb8);
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  for (int j = 0; j < k; ++j) {
    const f32x4* row = ys + ((t * k + j) * emb8 + c) * 2;
    const f32x4 a = row[0], b = row[1];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] += a.v[e];
      s[4 + e] += b.v[e];
    }
  }
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o.v[e] = f2bf(s[e]);
  out[i] = o;
}

template <int BM, bool GU>
static void launch_moe_gemm(const MoePtrs& wp, const void* act,
                            const int* row_pair, const int* tile_expert,
                            const float* wts, void* out, int K, int NC,
                            int npairs, int top_k, int nE, int ntiles,
                            hipStream_t stream) {
  constexpr int BN = MoeGeom<BM, GU>::BN;
  const int ncol = (NC + BN - 1) / BN;
  moe_gemm_kernel<BM, GU><<<(unsigned)(ntiles * ncol), 256, 0, stream>>>(
      wp, (const short*)act, row_pair, tile_expert, wts, out, K, NC, npairs,
      top_k, nE, ncol);
}

extern "C" {

void launch_moe_route(const float* logits, int* ids, float* wts, long long T,
                      int nE, int k, hipStream_t stream) {
  moe_route_kernel<<<(unsigned)((T + 255) / 256), 256, 0, stream>>>(
      logits, ids, wts, T, nE, k);
}

// hist: (ceil(npairs / 256), 16) int32 scratch; row_pair (ntiles * BM) and
// tile_expert (ntiles) are written in full
void launch_moe_sort(const int* ids, int* hist, int* row_pair,
                     int* tile_expert, long long npairs, int nE, int BM,
                     int ntiles, hipStream_t stream) {
  const int nb = (int)((npairs + 255) / 256);
  moe_hist_kernel<<<nb, 256, 0, stream>>>(ids, hist, npairs, nE);
  moe_scan_kernel<<<1, 256, 0, stream>>>(hist, row_pair, tile_expert, nb, nE,
                                         BM, ntiles);
  moe_scatter_kernel<<<nb, 256, 0, stream>>>(ids, hist, row_pair, npairs, nE,
                                             ntiles * BM);
}

// the binding and the cases below disagree: the output would stay
// uninitialised
static void moe_no_kernel(int BM) {
  fprintf(stderr, "moe.hip: no kernel for BM = %d\n", BM);
  abort();
}

// h (ntiles * BM, H) bf16; wg1[e] (2H, emb), nE pointers
void launch_moe_gate_up(const void* const* wg1, const void* x,
                        const int* row_pair, const int* tile_expert, void* h,
                        int emb, int H, int npairs, int top_k, int nE, int BM,
                        int ntiles, hipStream_t stream) {
  MoePtrs wp = {};
  for (int e = 0; e < nE; ++e) wp.p[e] = (const short*)wg1[e];
  if (BM == 128)
    return launch_moe_gemm<128, true>(wp, x, row_pair, tile_expert, nullptr,
                                      h, emb, H, npairs, top_k, nE, ntiles,
                                      stream);
  if (BM == 32)
    return launch_moe_gemm<32, true>(wp, x, row_pair, tile_expert, nullptr, h,
                                     emb, H, npairs, top_k, nE, ntiles,
                                     stream);
  moe_no_kernel(BM);
}

// ys (npairs, emb) fp32; w2[e] (emb, H), nE pointers
void launch_moe_down(const void* const* w2, const void* h,
                     const int* row_pair, const int* tile_expert,
                     const float* wts, float* ys, int emb, int H, int npairs,
                     int nE, int BM, int ntiles, hipStream_t stream) {
  MoePtrs wp = {};
  for (int e = 0; e < nE; ++e) wp.p[e] = (const short*)w2[e];
  if (BM == 128)
    return launch_moe_gemm<128, false>(wp, h, row_pair, tile_expert, wts, ys,
                                       H, emb, npairs, 1, nE, ntiles, stream);
  if (BM == 32)
    return launch_moe_gemm<32, false>(wp, h, row_pair, tile_expert, wts, ys,
                                      H, emb, npairs, 1, nE, ntiles, stream);
  moe_no_kernel(BM);
}

void launch_moe_combine(const float* ys, void* out, long long T, int emb,
                        int k, hipStream_t stream) {
  const long long total = T * (emb / 8);
  moe_combine_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(
      (const f32x4*)ys, (bf16x8*)out, total, emb / 8, k);
}

}  // extern "C"
