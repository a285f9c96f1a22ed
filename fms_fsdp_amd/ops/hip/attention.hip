// Causal flash attention (forward + backward) for CDNA4/gfx950.
// MFMA v_mfma_f32_32x32x16_bf16 tiles, LDS-staged K/V with XOR swizzle,
// swapped-QK^T structure (compute S^T = K @ Q^T so each lane owns ONE
// q-row and softmax is lane-local: guide §B "swapped QK^T ... row-reduce
// is 31 fmax + 1 permlane32_swap").
//
// Layouts (bf16, contiguous): q (b, s, h, d), k/v (b, s, kvh, d), d in
// {64, 128}; causal; GQA via kvh | h. lse (b, h, s) fp32 saved for bwd.
// Replaces the reference's torch-SDPA flash call (SURVEY.md §2.3:
// "SDPA FlashAttention-v2 fwd+bwd ... MFMA tiled flash kernel, LDS
// double-buffering, causal block skipping, GQA head-broadcast").
//
// MFMA fragment maps used throughout (guide §3, cdna4 32x32x16 bf16):
//   A[i][k]: lane l -> i = l&31,          k = (l>>5)*8 + e   (e=0..7)
//   B[k][j]: lane l -> k = (l>>5)*8 + e,  j = l&31
//   D[i][j]: lane l, reg r -> j = l&31,   i = (r&3) + 8*(r>>2) + 4*(l>>5)
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "attn_frag.h"
#include "attn_sched.h"
#include "attn_ws.h"

// ---- immediate-offset, software-pipelined transpose reads ------------
// The 16 tr-read addresses of a PV/dq/dkv output loop share ONE runtime
// base (swizzle ^ half-select ^ 16-lane-block, all lane-derived); the
// remaining terms are compile-time. Issuing through `offset:` immediates
// removes the per-read VALU address chain (PMC round-1: VALU is the
// limiter, profiles/attn_pmc_counters_r01.md), and splitting issue from
// wait lets fragment t+1 stream from LDS while fragment t feeds mfmas.
// Counted waits are safe here because DS ops retire IN ORDER: "allow 4
// outstanding" implies everything older (incl. staging ds_writes) is
// done. No SMEM is issued inside these windows.
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void tr_issue4(unsigned base, U2x64& r0,
                                          U2x64& r1) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4 offset:%c5\n\t"
      "ds_read_b64_tr_b16 %1, %4 offset:%c6\n\t"
      "ds_read_b64_tr_b16 %2, %4 offset:%c7\n\t"
      "ds_read_b64_tr_b16 %3, %4 offset:%c8"
      : "=&v"(r0.u[0]), "=&v"(r0.u[1]), "=&v"(r1.u[0]), "=&v"(r1.u[1])
      : "v"(base), "i"(O0), "i"(O1), "i"(O2), "i"(O3)
      : "memory");
}

template <int CNT>
__device__ __forceinline__ void tr_wait(U2x64& r0, U2x64& r1) {
  asm volatile("s_waitcnt lgkmcnt(%c4)"
               : "+v"(r0.u[0]), "+v"(r0.u[1]), "+v"(r1.u[0]), "+v"(r1.u[1])
               : "i"(CNT)
               : "memory");
}

// lane-derived base for the subtiled-image transpose reads: row-group
// XOR (constant 16*hb for every fragment of these loops), the in-subtile
// lane column, the hb*8 key offset (rg = hb*2 -> 256*hb bytes) and the
// 16-lane block select. R4B = R4*128 bytes per column block.
template <int R4B>
__device__ __forceinline__ unsigned tr_base(int lane, int col, int hb) {
  return (unsigned)((((lane & 15) * 8) ^ (16 * hb)) + hb * 256 +
                    (col >> 4) * R4B);
}

// document-mask arrays are clamped where they are read (DOCMASK kernels)
__device__ __forceinline__ int doc_clamp(int v, int lo, int hi) {
  return min(max(v, lo), hi);
}

// ---------------------------------------------------------------------
// Forward. Block = 4 waves x 32 q-rows = 128 q rows; KV tile = 64 keys.
// 1-D grid of (s/128)*(b*h) workgroups; attn_sched_map() (attn_sched.h)
// turns the linear id into (q tile, bh).
//
// DOCMASK: query i sees key j iff docs[b][i] <= j <= i, docs = the (b, s)
// int32 position of the first token of i's document (non-decreasing). Each
// lane holds its row's start (clamped into [0, q], so no content of the
// array can move a loop bound or an address out of range); the KV loop
// starts at the tile of docs[q0], the workgroup's minimum; the wave-uniform
// flags take the wave's own first and last start, so tiles strictly inside
// one document run the unmasked instruction stream.
// ---------------------------------------------------------------------
template <int D, bool DOCMASK = false>
__global__ __launch_bounds__(256, 3) void attn_fwd_kernel(
    const short* __restrict__ qg, const short* __restrict__ kg,
    const short* __restrict__ vg, short* __restrict__ og,
    float* __restrict__ lseg, int B, int S, int H, int KVH, float scale,
    long long vstride, int sched, const int* __restrict__ docs = nullptr) {
  constexpr int KVB = 64;
  constexpr int NC = D / 16;   // QK^T k-chunks
  constexpr int NT = D / 32;   // 32-wide output tiles
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // SUBTILED K/V images (same layout as the backward kernels: coalesced
  // b128 staging, plain reads for the S^T A-operand, hardware transpose
  // reads for the PV A-operand). LDS diet for occupancy: K is
  // SINGLE-buffered, V double-buffered (48 KB at D=128 -> 3 blocks/CU,
  // up from 2 at the fully double-buffered 64 KB; VGPRs fit 3 waves).
  // K(t+1) is staged mid-tile right after the last S-phase read of
  // K(t), costing a second barrier per tile.
  constexpr int KB = KVB * D * 2;
#define KLDS() (smem)
#define VLDS(buf) (smem + KB + ((buf) ? KB : 0))

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int col = lane & 31;   // q-row owner within wave tile
  const int hb = lane >> 5;

  const AttnWork wk = attn_sched_map(blockIdx.x, S / 128, B * H, sched, false);
  const int bh = __builtin_amdgcn_readfirstlane(wk.bh);
  const int b = bh / H;
  const int h = bh % H;
  const int kvh = h / (H / KVH);
  // block q range [q0, q0+128)
  const int q0 = __builtin_amdgcn_readfirstlane(wk.tile) * 128;
  const int qw = q0 + wid * 32;           // wave q range
  const int my_q = qw + col;              // this lane's q row

  const long long qrow_stride = (long long)H * D;
  const long long krow_stride = (long long)KVH * D;
  const short* qbase = qg + ((long long)b * S * H + (long long)h) * D;
  const short* kbase = kg + ((long long)b * S * KVH + (long long)kvh) * D;
  // v may be a strided view (a slice of the fused qkv projection)
  const short* vbase = vg + (long long)b * S * vstride + (long long)kvh * D;

  // document mask: this lane's first visible key, the first and last
  // start of the wave (wave-uniform) and the first KV tile of the block
  int my_start = 0, w_lo = 0, w_hi = 0, tile0 = 0;
  if constexpr (DOCMASK) {
    const int* dsp = docs + (long long)b * S;
    my_start = doc_clamp(dsp[my_q], 0, my_q);
    w_lo = __builtin_amdgcn_readfirstlane(doc_clamp(dsp[qw], 0, qw));
    w_hi = __builtin_amdgcn_readfirstlane(
        doc_clamp(dsp[qw + 31], 0, qw + 31));
    tile0 = __builtin_amdgcn_readfirstlane(doc_clamp(dsp[q0], 0, q0)) / 64;
  }

  // softmax runs in base 2 (v_exp_f32 is natively 2^x; folding log2(e)
  // into the scale drops one v_mul per exponential)
  const float scale2 = scale * 1.4426950408889634f;
  // Q -> B-fragments (registers, reused all tiles), PRE-SCALED by
  // scale*log2e: accS arrives already in softmax units, dropping 16
  // VALU muls per sub-tile (PMC: every kernel is VALU-bound). The bf16
  // rounding of q*scale2 is within the operands' own precision.
  bf16x8v qb[NC];
  {
    const short* qp = qbase + (long long)my_q * qrow_stride + hb * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bf16x8v qv = *(const bf16x8v*)(qp + c * 16);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        qv[e] = (__bf16)((float)qv[e] * scale2);
      qb[c] = qv;
    }
  }

  f32x16 accO[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) accO[t] = (f32x16)(0.f);
  float m_run = -1e30f, l_run = 0.f;

  const int ntiles = (q0 + 128 + KVB - 1) / KVB;
  const int t256 = threadIdx.x;
  // subtiled staging: thread t: key = t&63, colblk pair = t>>6 (each
  // thread copies 2x16B per image; 64-key rows x D cols). Global
  // pointers advance incrementally (no per-tile 64-bit muls) and the
  // LDS offsets are per-thread constants computed once.
  const int skey = t256 & 63;
  const int sd0 = (t256 >> 6) * (D / 4);   // 32 cols per thread @D=128
  const short* kp_s = kbase + (long long)skey * krow_stride + sd0;
  const short* vp_s = vbase + (long long)skey * vstride + sd0;
  const long long kstep = (long long)KVB * krow_stride;
  const long long vstep = (long long)KVB * vstride;
  if constexpr (DOCMASK) {   // tiles in front of the block's first document
    kp_s += tile0 * kstep;
    vp_s += tile0 * vstep;
  }
  int soff[D / 64][2];
#pragma unroll
  for (int c2 = 0; c2 < D / 64; ++c2) {
    soff[c2][0] = SUBT_OFF(skey, sd0 + c2 * 16, 16);
    soff[c2][1] = SUBT_OFF(skey, sd0 + c2 * 16 + 8, 16);
  }
  auto stage_k = [&]() {
#pragma unroll
    for (int c2 = 0; c2 < D / 64; ++c2) {
      *(f32x4*)(KLDS() + soff[c2][0]) = *(const f32x4*)(kp_s + c2 * 16);
      *(f32x4*)(KLDS() + soff[c2][1]) = *(const f32x4*)(kp_s + c2 * 16 + 8);
    }
    kp_s += kstep;
  };
  auto stage_v = [&](int buf) {
#pragma unroll
    for (int c2 = 0; c2 < D / 64; ++c2) {
      *(f32x4*)(VLDS(buf) + soff[c2][0]) = *(const f32x4*)(vp_s + c2 * 16);
      *(f32x4*)(VLDS(buf) + soff[c2][1]) = *(const f32x4*)(vp_s + c2 * 16 + 8);
    }
    vp_s += vstep;
  };
  stage_k();
  stage_v(0);
  __syncthreads();
  // per-buffer tr-read bases for the PV loops (R4 = KVB/4 = 16)
  const unsigned pv_swz = tr_base<2048>(lane, col, hb);
  const unsigned pvb[2] = {(unsigned)(unsigned long long)VLDS(0) + pv_swz,
                           (unsigned)(unsigned long long)VLDS(1) + pv_swz};
  int cur = 0;
  for (int tile = tile0; tile < ntiles; ++tile) {
    const int kv0 = tile * KVB;
    if (tile + 1 < ntiles) stage_v(cur ^ 1);

    // ---- two 32-key sub-tiles, each with its own online-softmax pass.
    // Register economy: one live accS/p set (16 regs) instead of two.
    // defer-max (guide T13, THR=8 nats = 11.5 bits): the O/l rescale
    // runs only when the sub-tile max exceeds the running max by more
    // than THR; P is then bounded by e^THR which the fp32 accumulate
    // tolerates. Decision is made BEFORE this sub-tile's P is
    // exponentiated (the safe order).
    // S-phase + softmax + pack for one sub-tile; PV split out so kt=1's
    // PV can run after the mid-tile K barrier (single-buffered K).
    bf16x8v pb1_0, pb1_1;
    // wave-uniform: causal, and (DOCMASK) not wholly in front of the
    // wave's first document
    const bool act1 = (kv0 + 32) <= qw + 31 && (!DOCMASK || kv0 + 63 >= w_lo);
    const bool act0 = !DOCMASK || kv0 + 31 >= w_lo;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int kv32 = kv0 + kt * 32;
      if (kt == 0 && !act0) continue;
      if (kt == 1 && !act1) break;
      f32x16 accS = (f32x16)(0.f);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int row = kt * 32 + col;
        const bf16x8v a = *(const bf16x8v*)(
            KLDS() + SUBT_OFF(row, c * 16 + hb * 8, 16));
        accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qb[c], accS, 0, 0, 0);
      }
      float p[16];
      // DOCMASK: the lower mask is needed up to the wave's last start
      const bool partial =
          (kv32 + 32) > (qw + 1) || (DOCMASK && kv32 < w_hi);
      float mt = -1e30f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float sv = accS[r];                   // q pre-scaled at load
        const int key = kv32 + DROW(r, hb);
        if (partial && (key > my_q || (DOCMASK && key < my_start)))
          sv = -1e30f;
        p[r] = sv;
        mt = fmaxf(mt, sv);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      float alpha = 1.f;
      if (mt > m_run + 11.5f) {        // defer-max threshold (base-2)
        alpha = exp2f(m_run - mt);
        m_run = mt;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) accO[t][r] *= alpha;
      }
      float s_own = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = exp2f(p[r] - m_run);
        if constexpr (DOCMASK) {
          // a row whose document starts behind this sub-tile still has
          // m_run = -1e30: exp2(-1e30 - m_run) would be 1, not 0
          const int key = kv32 + DROW(r, hb);
          if (partial && (key > my_q || key < my_start)) p[r] = 0.f;
        }
        s_own += p[r];
      }
      l_run = l_run * alpha + s_own + __shfl_xor(s_own, 32, 64);

      const unsigned pvbase = pvb[cur] + kt * 1024;   // rg += kt*8
      if (kt == 0) {
        // PV immediately (software-pipelined immediate-offset reads;
        // first issue BEFORE the P pack so LDS latency hides behind
        // the pack VALU work)
        U2x64 fr[2][2];
        tr_issue4<0, 128, 512, 640>(pvbase, fr[0][0], fr[0][1]);
        const bf16x8v pb0 = pack_pT_chunk(p);
        const bf16x8v pb1 = pack_pT_chunk(p + 8);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int pp = t & 1;
          if (t + 1 < NT) {
            // offsets: (t+1)*2*(KVB/4)*128 = (t+1)*4096 + rg*128
            if (t + 1 == 1)
              tr_issue4<4096, 4096 + 128, 4096 + 512, 4096 + 640>(
                  pvbase, fr[1][0], fr[1][1]);
            else if (t + 1 == 2)
              tr_issue4<8192, 8192 + 128, 8192 + 512, 8192 + 640>(
                  pvbase, fr[0][0], fr[0][1]);
            else
              tr_issue4<12288, 12288 + 128, 12288 + 512, 12288 + 640>(
                  pvbase, fr[1][0], fr[1][1]);
            tr_wait<4>(fr[pp][0], fr[pp][1]);
          } else {
            tr_wait<0>(fr[pp][0], fr[pp][1]);
          }
          accO[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][0].v, pb0,
                                                            accO[t], 0, 0, 0);
          accO[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][1].v, pb1,
                                                            accO[t], 0, 0, 0);
        }
      } else {
        // pack only; PV runs after the K barrier below
        pb1_0 = pack_pT_chunk(p);
        pb1_1 = pack_pT_chunk(p + 8);
      }
    }
    // all waves are done reading K(tile): restage the single K image
    __syncthreads();
    if (tile + 1 < ntiles) stage_k();
    if (act1) {
      const unsigned pvbase = pvb[cur] + 1024;
      U2x64 fr[2][2];
      tr_issue4<0, 128, 512, 640>(pvbase, fr[0][0], fr[0][1]);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int pp = t & 1;
        if (t + 1 < NT) {
          if (t + 1 == 1)
            tr_issue4<4096, 4096 + 128, 4096 + 512, 4096 + 640>(
                pvbase, fr[1][0], fr[1][1]);
          else if (t + 1 == 2)
            tr_issue4<8192, 8192 + 128, 8192 + 512, 8192 + 640>(
                pvbase, fr[0][0], fr[0][1]);
          else
            tr_issue4<12288, 12288 + 128, 12288 + 512, 12288 + 640>(
                pvbase, fr[1][0], fr[1][1]);
          tr_wait<4>(fr[pp][0], fr[pp][1]);
        } else {
          tr_wait<0>(fr[pp][0], fr[pp][1]);
        }
        accO[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][0].v, pb1_0,
                                                          accO[t], 0, 0, 0);
        accO[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][1].v, pb1_1,
                                                          accO[t], 0, 0, 0);
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: o[q][dv] = accO^T / l ----
  const float inv_l = 1.f / l_run;
  short* op = og + ((long long)b * S * H + (long long)h) * D +
              (long long)my_q * qrow_stride;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {   // reg groups of 4 -> dv consecutive 4
      const int dv0 = t * 32 + 8 * g + 4 * hb;
      bf16x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w.v[j] = f2bf(accO[t][g * 4 + j] * inv_l);
      *(bf16x4*)(op + dv0) = w;
    }
  }
  if (hb == 0)   // exported in natural-log units (tests, bwd contract)
    lseg[((long long)bh) * S + my_q] =
        (m_run + __log2f(l_run)) * 0.6931471805599453f;
}
#undef KLDS
#undef VLDS

// ---------------------------------------------------------------------
// Backward preprocess: delta[b,h,s] = rowsum(dO * O) fp32
// ---------------------------------------------------------------------
// LPR = D/8 lanes per row, 64/LPR rows per wave: every lane loads 16 bytes
// of dO and of O, and consecutive lanes read consecutive memory (the rows
// are contiguous). Sub-wave xor reduction over the row's LPR lanes.
template <int LPR>
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(
    const bf16x8* __restrict__ dog, const bf16x8* __restrict__ og,
    float* __restrict__ delta, int S, int H, long long rows) {
  // input rows are (b, s, h) order, delta is (b, h, s)
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long row = gid / LPR;
  float acc = 0.f;
  if (row < rows) {   // a row's lanes agree; idle lanes still shuffle
    const bf16x8 a = dog[gid], c = og[gid];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += bf2f(a.v[j]) * bf2f(c.v[j]);
  }
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1)
    acc += __shfl_xor(acc, off, LPR);
  if (row < rows && (threadIdx.x & (LPR - 1)) == 0) {
    const long long b = row / ((long long)S * H);
    const int si = (int)((row / H) % S);
    const int hi = (int)(row % H);
    delta[(b * H + hi) * (long long)S + si] = acc;
  }
}

// ---------------------------------------------------------------------
// Backward dq, consuming the dS workspace the dkv kernel published:
//   dq^T[dk][q] = sum_key K^T[dk][key] * dS^T[key][q]
// No S/dP recompute, no softmax, no lse/delta reads — the backward
// drops from 7 gemm chains to 5 (dkv computes dS once for both sides).
// A = K^T via tr reads on the K image; B = dS^T via tr reads on the
// staged dS tile. grid over q-tiles; each wave owns its 32 q rows.
// ---------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(
    const short* __restrict__ kg, const short* __restrict__ dsw,
    short* __restrict__ dqg, int B, int S, int H, int KVH, int sched,
    int ws_tiled) {
  constexpr int KVB = 32;
  constexpr int NT = D / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered subtiled images: K (KVB x D) + dS (KVB x 128 q)
  constexpr int KIMGB = KVB * D * 2;
  constexpr int SIMGB = KVB * 128 * 2;
#define KIMG(buf) (smem + ((buf) ? KIMGB + SIMGB : 0))
#define SIMG(buf) (smem + KIMGB + ((buf) ? KIMGB + SIMGB : 0))

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int col = lane & 31;
  const int hb = lane >> 5;

  const AttnWork wk = attn_sched_map(blockIdx.x, S / 128, B * H, sched, false);
  const int bh = __builtin_amdgcn_readfirstlane(wk.bh);
  const int b = bh / H;
  const int h = bh % H;
  const int kvh = h / (H / KVH);
  const int q0 = __builtin_amdgcn_readfirstlane(wk.tile) * 128;
  const int qw = q0 + wid * 32;
  const int my_q = qw + col;

  const long long qrow_stride = (long long)H * D;
  const long long krow_stride = (long long)KVH * D;
  const short* kbase = kg + ((long long)b * S * KVH + (long long)kvh) * D;
  const short* dsbase = dsw + (long long)bh * S * S + q0;

  f32x16 accDQ[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) accDQ[t] = (f32x16)(0.f);

  const int ntiles = (q0 + 128 + KVB - 1) / KVB;
  const int t256 = threadIdx.x;
  // staging: K rows (t&31, D cols split over 8 groups) and dS rows
  // (t&31 keys x 128 q cols split over 8 groups of 16)
  const int skey = t256 & 31;
  const int sgrp = t256 >> 5;            // 0..7
  const int skd0 = sgrp * (D / 8);
  const short* kp_s = kbase + (long long)skey * krow_stride + skd0;
  const long long kstep = (long long)KVB * krow_stride;
  // row-major workspace [bh][key][q], or the key-lane dkv kernel's tiles
  // [bh][key/32][q/32][q%32/16][key%32][q%16]: a thread's 16 q are 32 B
  // contiguous either way, and a key tile step is 32*S elements in both
  const short* sp_s =
      ws_tiled ? dsw + (long long)bh * S * S +
                     (long long)(q0 / 32 + (sgrp >> 1)) * 1024 +
                     (sgrp & 1) * 512 + skey * 16
               : dsbase + (long long)skey * S + sgrp * 16;
  const long long sstep = (long long)KVB * S;
  const int koff = SUBT_OFF(skey, skd0, 8);
  const int koff1 = SUBT_OFF(skey, skd0 + 8, 8);
  const int soff0 = SUBT_OFF(skey, sgrp * 16, 8);
  const int soff1 = SUBT_OFF(skey, sgrp * 16 + 8, 8);
  auto stage = [&](int buf) {
    if constexpr (D == 128) {
      *(f32x4*)(KIMG(buf) + koff) = *(const f32x4*)(kp_s);
      *(f32x4*)(KIMG(buf) + koff1) = *(const f32x4*)(kp_s + 8);
    } else {
      *(f32x4*)(KIMG(buf) + koff) = *(const f32x4*)(kp_s);
    }
    *(f32x4*)(SIMG(buf) + soff0) = *(const f32x4*)(sp_s);
    *(f32x4*)(SIMG(buf) + soff1) = *(const f32x4*)(sp_s + 8);
    kp_s += kstep;
    sp_s += sstep;
  };
  stage(0);
  __syncthreads();
  // tr-read bases (R4 = 8 for both images)
  const unsigned ktr = tr_base<1024>(lane, col, hb);
  const unsigned kib[2] = {(unsigned)(unsigned long long)KIMG(0) + ktr,
                           (unsigned)(unsigned long long)KIMG(1) + ktr};
  // dS image cols = the wave's q window: base col = wid*32
  const unsigned str = (unsigned)((((lane & 15) * 8) ^ (16 * hb)) +
                                  hb * 256 + ((col >> 4) << 10) +
                                  (wid * 32) * 64);
  const unsigned sib[2] = {(unsigned)(unsigned long long)SIMG(0) + str,
                           (unsigned)(unsigned long long)SIMG(1) + str};

  int cur = 0;
  for (int tile = 0; tile < ntiles; ++tile) {
    if (tile + 1 < ntiles) stage(cur ^ 1);
    // B fragments: dS^T, two 16-key chunks
    U2x64 bs[2];
    tr_issue4<0, 128, 512, 512 + 128>(sib[cur], bs[0], bs[1]);
    tr_wait<0>(bs[0], bs[1]);
    const unsigned kbase_t = kib[cur];
    U2x64 fr[2][2];
    tr_issue4<0, 128, 512, 640>(kbase_t, fr[0][0], fr[0][1]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int pp = t & 1;
      if (t + 1 < NT) {
        if (t + 1 == 1)
          tr_issue4<2048, 2048 + 128, 2048 + 512, 2048 + 640>(
              kbase_t, fr[1][0], fr[1][1]);
        else if (t + 1 == 2)
          tr_issue4<4096, 4096 + 128, 4096 + 512, 4096 + 640>(
              kbase_t, fr[0][0], fr[0][1]);
        else
          tr_issue4<6144, 6144 + 128, 6144 + 512, 6144 + 640>(
              kbase_t, fr[1][0], fr[1][1]);
        tr_wait<4>(fr[pp][0], fr[pp][1]);
      } else {
        tr_wait<0>(fr[pp][0], fr[pp][1]);
      }
      accDQ[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][0].v,
                                                         bs[0].v, accDQ[t],
                                                         0, 0, 0);
      accDQ[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][1].v,
                                                         bs[1].v, accDQ[t],
                                                         0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }

  // dq was accumulated UNSCALED dS? No — dkv stored ds already *scale.
  short* dqp = dqg + ((long long)b * S * H + (long long)h) * D +
               (long long)my_q * qrow_stride;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int dk0 = t * 32 + 8 * g + 4 * hb;
      bf16x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w.v[j] = f2bf(accDQ[t][g * 4 + j]);
      *(bf16x4*)(dqp + dk0) = w;
    }
  }
}
#undef KIMG
#undef SIMG

// ---------------------------------------------------------------------
// Backward dq WITHOUT the dS workspace (O(S) memory): the forward
// kernel's layout with the online softmax replaced by the saved lse.
// Each lane owns one q row; Q and dO B-fragments stay in registers for
// the whole key sweep; K and V 32-key tiles are staged as double-
// buffered subtiled images. Per key tile:
//   S^T  = K  Q^T    (A = plain reads of the K image)
//   dP^T = V dO^T    (A = plain reads of the V image)
//   p    = exp2(S*scale*log2e - lse*log2e), 0 where key > q
//   dS   = p * (dP - delta) * scale     -> bf16 B-operand in registers
//   dq^T += K^T dS^T (A = tr reads of the SAME K image)
// Formulas, mfma chunk order and the bf16 rounding of dS are those of
// attn_bwd_dkv_kernel, so both sides of the backward see the same dS.
// Costs the S and dP chains a second time (7 gemm chains across the
// backward instead of 5); selected only when the (b*h, s, s) workspace
// would exceed the limit (attn_ws.h).
// ---------------------------------------------------------------------
// DOCMASK as in the forward (docs = first position of the row's document):
// per-lane start, key sweep from the 32-key tile of docs[q0], wave flags
// from the wave's first and last start.
template <int D, bool DOCMASK = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_recompute_kernel(
    const short* __restrict__ dog, const short* __restrict__ qg,
    const short* __restrict__ kg, const short* __restrict__ vg,
    const float* __restrict__ lseg, const float* __restrict__ deltag,
    short* __restrict__ dqg, int B, int S, int H, int KVH, float scale,
    long long vstride, int sched, const int* __restrict__ docs = nullptr) {
  constexpr int KVB = 32;
  constexpr int NC = D / 16;
  constexpr int NT = D / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered subtiled images: K (KVB x D) + V (KVB x D), R4 = 8
  constexpr int IMGB = KVB * D * 2;
#define KIMG(buf) (smem + ((buf) ? 2 * IMGB : 0))
#define VIMG(buf) (smem + IMGB + ((buf) ? 2 * IMGB : 0))

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31;
  const int hb = lane >> 5;

  const AttnWork wk = attn_sched_map(blockIdx.x, S / 128, B * H, sched, false);
  const int bh = __builtin_amdgcn_readfirstlane(wk.bh);
  const int b = bh / H;
  const int h = bh % H;
  const int kvh = h / (H / KVH);
  const int q0 = __builtin_amdgcn_readfirstlane(wk.tile) * 128;
  const int qw = q0 + wid * 32;
  const int my_q = qw + col;

  const long long qrow_stride = (long long)H * D;
  const long long krow_stride = (long long)KVH * D;
  const long long qoff = ((long long)b * S * H + (long long)h) * D +
                         (long long)my_q * qrow_stride;
  const short* kbase = kg + ((long long)b * S * KVH + (long long)kvh) * D;
  const short* vbase = vg + (long long)b * S * vstride + (long long)kvh * D;

  // Q / dO -> B-fragments (B[k = feature][j = q]), unscaled like dkv's
  bf16x8v qb[NC], dob[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    qb[c] = *(const bf16x8v*)(qg + qoff + hb * 8 + c * 16);
    dob[c] = *(const bf16x8v*)(dog + qoff + hb * 8 + c * 16);
  }
  const float lse_q2 = lseg[(long long)bh * S + my_q] * 1.4426950408889634f;
  const float delta_q = deltag[(long long)bh * S + my_q];
  const float scale2 = scale * 1.4426950408889634f;

  int my_start = 0, w_lo = 0, w_hi = 0, tile0 = 0;
  if constexpr (DOCMASK) {
    const int* dsp = docs + (long long)b * S;
    my_start = doc_clamp(dsp[my_q], 0, my_q);
    w_lo = __builtin_amdgcn_readfirstlane(doc_clamp(dsp[qw], 0, qw));
    w_hi = __builtin_amdgcn_readfirstlane(
        doc_clamp(dsp[qw + 31], 0, qw + 31));
    tile0 = __builtin_amdgcn_readfirstlane(doc_clamp(dsp[q0], 0, q0)) / 32;
  }

  f32x16 accDQ[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) accDQ[t] = (f32x16)(0.f);

  const int ntiles = (q0 + 128) / KVB;
  // staging: thread t: key = t&31, column group = t>>5 (D/8 cols). The
  // next tile is fetched into registers at the top of a tile and written
  // to the other buffer at its end, so the global latency hides behind
  // the tile's mfma work.
  const int skey = threadIdx.x & 31;
  const int skd0 = (threadIdx.x >> 5) * (D / 8);
  const short* kp_s = kbase + (long long)skey * krow_stride + skd0;
  const short* vp_s = vbase + (long long)skey * vstride + skd0;
  const long long kstep = (long long)KVB * krow_stride;
  const long long vstep = (long long)KVB * vstride;
  if constexpr (DOCMASK) {   // tiles in front of the block's first document
    kp_s += tile0 * kstep;
    vp_s += tile0 * vstep;
  }
  const int soff0 = SUBT_OFF(skey, skd0, 8);
  const int soff1 = SUBT_OFF(skey, skd0 + 8, 8);   // D = 128 only
  f32x4v kpre0, kpre1, vpre0, vpre1;
#define DQR_FETCH()                                   \
  do {                                                \
    kpre0 = *(const f32x4v*)(kp_s);                   \
    vpre0 = *(const f32x4v*)(vp_s);                   \
    if constexpr (D == 128) {                         \
      kpre1 = *(const f32x4v*)(kp_s + 8);             \
      vpre1 = *(const f32x4v*)(vp_s + 8);             \
    }                                                 \
    kp_s += kstep;                                    \
    vp_s += vstep;                                    \
  } while (0)
#define DQR_COMMIT(buf)                               \
  do {                                                \
    *(f32x4v*)(KIMG(buf) + soff0) = kpre0;            \
    *(f32x4v*)(VIMG(buf) + soff0) = vpre0;            \
    if constexpr (D == 128) {                         \
      *(f32x4v*)(KIMG(buf) + soff1) = kpre1;          \
      *(f32x4v*)(VIMG(buf) + soff1) = vpre1;          \
    }                                                 \
  } while (0)
  DQR_FETCH();
  DQR_COMMIT(0);
  __syncthreads();
  // tr-read bases into the K images (R4 = 8)
  const unsigned ktr = tr_base<1024>(lane, col, hb);
  const unsigned kib[2] = {(unsigned)(unsigned long long)KIMG(0) + ktr,
                           (unsigned)(unsigned long long)KIMG(1) + ktr};

  int cur = 0;
  for (int tile = tile0; tile < ntiles; ++tile) {
    const int kv0 = tile * KVB;
    const bool more = tile + 1 < ntiles;
    if (more) DQR_FETCH();
    // wave-uniform causal skip: key tiles past this wave's last q row
    // (DOCMASK: or wholly in front of its first document) contribute
    // exactly zero (the wave still stages and syncs)
    if (kv0 <= qw + 31 && (!DOCMASK || kv0 + 31 >= w_lo)) {
      f32x16 accS = (f32x16)(0.f), accDP = (f32x16)(0.f);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int aoff = SUBT_OFF(col, c * 16 + hb * 8, 8);
        const bf16x8v ka = *(const bf16x8v*)(KIMG(cur) + aoff);
        const bf16x8v va = *(const bf16x8v*)(VIMG(cur) + aoff);
        accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qb[c], accS, 0, 0, 0);
        accDP = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, dob[c], accDP,
                                                        0, 0, 0);
      }
      // first K^T fragments stream from LDS behind the softmax VALU work
      const unsigned kbase_t = kib[cur];
      U2x64 fr[2][2];
      tr_issue4<0, 128, 512, 640>(kbase_t, fr[0][0], fr[0][1]);
      const bool partial = (kv0 + 31) > qw || (DOCMASK && kv0 < w_hi);
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // select, never multiply: exp2 of a masked key may be inf
        float pval = exp2f(accS[r] * scale2 - lse_q2);
        const int key = kv0 + DROW(r, hb);
        if (partial && (key > my_q || (DOCMASK && key < my_start)))
          pval = 0.f;
        ds[r] = pval * (accDP[r] - delta_q) * scale;
      }
      // dS^T -> B-operand in registers (two 16-key chunks)
      const bf16x8v db0 = pack_pT_chunk(ds);
      const bf16x8v db1 = pack_pT_chunk(ds + 8);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int pp = t & 1;
        if (t + 1 < NT) {
          if (t + 1 == 1)
            tr_issue4<2048, 2048 + 128, 2048 + 512, 2048 + 640>(
                kbase_t, fr[1][0], fr[1][1]);
          else if (t + 1 == 2)
            tr_issue4<4096, 4096 + 128, 4096 + 512, 4096 + 640>(
                kbase_t, fr[0][0], fr[0][1]);
          else
            tr_issue4<6144, 6144 + 128, 6144 + 512, 6144 + 640>(
                kbase_t, fr[1][0], fr[1][1]);
          tr_wait<4>(fr[pp][0], fr[pp][1]);
        } else {
          tr_wait<0>(fr[pp][0], fr[pp][1]);
        }
        accDQ[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][0].v, db0,
                                                           accDQ[t], 0, 0, 0);
        accDQ[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][1].v, db1,
                                                           accDQ[t], 0, 0, 0);
      }
    }
    if (more) DQR_COMMIT(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // dS already carries *scale: the epilogue is the workspace dq kernel's
  short* dqp = dqg + qoff;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int dk0 = t * 32 + 8 * g + 4 * hb;
      bf16x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w.v[j] = f2bf(accDQ[t][g * 4 + j]);
      *(bf16x4*)(dqp + dk0) = w;
    }
  }
}
#undef DQR_FETCH
#undef DQR_COMMIT
#undef KIMG
#undef VIMG

// ---------------------------------------------------------------------
// Backward dk/dv: 1-D grid over (KV tile, bh) via attn_sched_map();
// each wave owns 32 keys and walks all q-tiles >= its block's kv base.
// dK/dV accumulate in registers;
// V stays in registers; K in a per-wave swizzled LDS tile; Q/dO arrive
// per q-iteration in shared SUBTILED images (coalesced vector staging,
// plain reads for the S/dP B-operands, tr_read for the dV/dK
// B-operands). The P/dS lane<->reg transpose goes through a small
// wave-private LDS buffer. TWO barriers per q-iteration.
// ---------------------------------------------------------------------
template <int D, bool OUT_BF16, bool PUBLISH_DS>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(
    const short* __restrict__ dog, const short* __restrict__ qg,
    const short* __restrict__ kg, const short* __restrict__ vg,
    const float* __restrict__ lseg, const float* __restrict__ deltag,
    void* __restrict__ dkg, void* __restrict__ dvg,
    short* __restrict__ dsw, int B, int S, int H,
    int KVH, float scale, long long vstride, long long dvstride, int sched) {
  constexpr int KVB = 32;   // keys per wave; block = 4 waves = 128 keys
  constexpr int NC = D / 16;
  constexpr int NT = D / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;                           // [4][KVB][D*2] per-wave
  // double-buffered subtiled Q/dO images (stage q-tile t+1 during t)
  constexpr int IMGB = 32 * D * 2;
#define QIMG(buf) (smem + 4 * KVB * D * 2 + ((buf) ? 2 * IMGB : 0))
#define DOIMG(buf) (smem + 4 * KVB * D * 2 + IMGB + ((buf) ? 2 * IMGB : 0))
  // P/dS transpose buffer: rows padded 64 -> 80 B so banks rotate 20
  // per row — the 16-lane transposed reads land on 16 distinct 4-bank
  // groups with no XOR (the old 64 B rows + 2-bit XOR were 4-way
  // conflicted; dkv had 2x the bank conflicts of the other kernels,
  // profiles/attn_pmc_counters_r01.md). 80 preserves 16 B alignment.
  char* p_lds = smem + 4 * KVB * D * 2 + 4 * IMGB;  // [4][KVB][80]

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int col = lane & 31;
  const int hb = lane >> 5;

  // key block 0 walks every q tile: it is the heaviest (heavy_low)
  const AttnWork wk = attn_sched_map(blockIdx.x, S / 128, B * H, sched, true);
  const int bh = __builtin_amdgcn_readfirstlane(wk.bh);
  const int tile = __builtin_amdgcn_readfirstlane(wk.tile);
  const int b = bh / H;
  const int h = bh % H;
  const int kvh = h / (H / KVH);
  const int ngrp = H / KVH;
  const int kv0 = tile * 128 + wid * KVB;

  const long long qrow_stride = (long long)H * D;
  const long long krow_stride = (long long)KVH * D;
  const short* qbase = qg + ((long long)b * S * H + (long long)h) * D;
  const short* dobase = dog + ((long long)b * S * H + (long long)h) * D;
  const short* kbase = kg + ((long long)b * S * KVH + (long long)kvh) * D;
  const short* vbase = vg + (long long)b * S * vstride + (long long)kvh * D;

  char* my_k = k_lds + wid * KVB * D * 2;
  char* my_p = p_lds + wid * KVB * 80;

  // stage this wave's K rows once, in the SUBTILED image format (same
  // as the Q/dO images): the S-phase plain reads hit the proven
  // conflict-free pattern (PMC: the old row-swizzled tile carried the
  // residual bank conflicts)
  {
    constexpr int CHUNKS = KVB * D / 8;     // 16 B chunks
    for (int i = lane; i < CHUNKS; i += 64) {
      const int row = i / (D / 8);
      const int cb = (i % (D / 8)) * 8;
      const long long g = (long long)(kv0 + row) * krow_stride + cb;
      *(f32x4*)(my_k + SUBT_OFF(row, cb, 8)) = *(const f32x4*)(kbase + g);
    }
  }
  // V fragments stay in registers (A-operand rows = this lane's key)
  bf16x8v vreg[NC];
  {
    const short* vp = vbase + (long long)(kv0 + col) * vstride + hb * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) vreg[c] = *(const bf16x8v*)(vp + c * 16);
  }

  f32x16 accDV[NT], accDK[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    accDV[t] = (f32x16)(0.f);
    accDK[t] = (f32x16)(0.f);
  }

  const int q_start = (tile * 128) / 32 * 32;
  const int t256 = threadIdx.x;
  // thread t owns q row t&31 and ADJACENT column chunks (see the dq
  // kernel's staging comment: cacheline locality matters here);
  // incremental global pointers + precomputed LDS offsets
  const int sq = t256 & 31;
  const int sd0 = (t256 >> 5) * ((D == 128) ? 16 : 8);
  const short* qp_s = qbase + ((long long)(q_start + sq)) * qrow_stride + sd0;
  const short* dop_s = dobase + ((long long)(q_start + sq)) * qrow_stride + sd0;
  const long long qstep = 32 * qrow_stride;
  const int soff0 = SUBT_OFF(sq, sd0, 8);
  const int soff1 = SUBT_OFF(sq, sd0 + 8, 8);
  auto stage = [&](int buf) {
    if constexpr (D == 128) {
      *(f32x4*)(QIMG(buf) + soff0) = *(const f32x4*)(qp_s);
      *(f32x4*)(QIMG(buf) + soff1) = *(const f32x4*)(qp_s + 8);
      *(f32x4*)(DOIMG(buf) + soff0) = *(const f32x4*)(dop_s);
      *(f32x4*)(DOIMG(buf) + soff1) = *(const f32x4*)(dop_s + 8);
    } else {  // D=64: 32 rows x 8 chunks, one 16B chunk/thread
      *(f32x4*)(QIMG(buf) + soff0) = *(const f32x4*)(qp_s);
      *(f32x4*)(DOIMG(buf) + soff0) = *(const f32x4*)(dop_s);
    }
    qp_s += qstep;
    dop_s += qstep;
  };
  stage(0);
  __syncthreads();
  // tr-read base offset into the Q/dO images (R4 = 8)
  const unsigned kv_swz = tr_base<1024>(lane, col, hb);
  int cur = 0;
  for (int q0 = q_start; q0 < S; q0 += 32) {
    if (q0 + 32 < S) stage(cur ^ 1);

    // S^T (A=K lds, B=imgq) and dP^T (A=V regs, B=imgdo)
    f32x16 accS = (f32x16)(0.f), accDP = (f32x16)(0.f);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int boff = SUBT_OFF(col, c * 16 + hb * 8, 8);
      const bf16x8v ka = *(const bf16x8v*)(my_k + boff);
      const bf16x8v qbf = *(const bf16x8v*)(QIMG(cur) + boff);
      const bf16x8v dbf = *(const bf16x8v*)(DOIMG(cur) + boff);
      accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qbf, accS, 0, 0, 0);
      accDP = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vreg[c], dbf, accDP,
                                                      0, 0, 0);
    }

    const float lse_q2 =
        lseg[((long long)bh) * S + q0 + col] * 1.4426950408889634f;
    const float delta_q = deltag[((long long)bh) * S + q0 + col];
    const float scale2 = scale * 1.4426950408889634f;
    float pv[16], ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kv0 + DROW(r, hb);
      const int q = q0 + col;
      float pval = exp2f(accS[r] * scale2 - lse_q2);
      if (key > q) pval = 0.f;
      pv[r] = pval;
      ds[r] = pval * (accDP[r] - delta_q) * scale;
    }
    // P -> my_p (wave-private; in-wave LDS ordering suffices)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = DROW(r, hb);
      *(short*)(my_p + key * 80 + col * 2) = f2bf(pv[r]);
    }
    // dV[key][dv] += P(A) @ tr(imgdo)(B). Immediate-offset reads (one
    // base add per t) — the dkv kernel sits at the 255-VGPR edge, so no
    // extra pipeline slots here, but the address chains still go.
#define DKV_TRLOOP(ACC, A0, A1, BASE)                                        \
  do {                                                                       \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) {                         \
      U2x64 f0, f1;                                                          \
      const unsigned b_t = (BASE) + t * 2048;                                \
      tr_issue4<0, 128, 512, 640>(b_t, f0, f1);                              \
      tr_wait<0>(f0, f1);                                                    \
      ACC[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, f0.v, ACC[t],     \
                                                       0, 0, 0);             \
      ACC[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, f1.v, ACC[t],     \
                                                       0, 0, 0);             \
    }                                                                        \
  } while (0)
    {
      bf16x8v pa[2];
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        const int inrow = kc * 32 + hb * 16;
        pa[kc] = *(const bf16x8v*)(my_p + col * 80 + inrow);
      }
      const unsigned dob = (unsigned)(unsigned long long)DOIMG(cur) + kv_swz;
      DKV_TRLOOP(accDV, pa[0], pa[1], dob);
    }
    // dS -> my_p, then dK[key][dk] += dS(A) @ tr(imgq)(B)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = DROW(r, hb);
      *(short*)(my_p + key * 80 + col * 2) = f2bf(ds[r]);
    }
    // publish this (32-key x 32-q) dS tile to the global workspace: the
    // dq kernel consumes it instead of recomputing the S and dP chains
    // (7 gemm chains across the backward -> 5). Vectorized readback from
    // the my_p transpose buffer: lane l covers key l&31, 16B q-chunk
    // (l>>5)*2 + c. Compiled out (PUBLISH_DS = false) on the workspace-
    // free path, where the dq kernel recomputes dS itself.
    if constexpr (PUBLISH_DS) {
      const int key = lane & 31;
      const long long grow = ((long long)bh * S + kv0 + key) * S + q0;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int qc = ((lane >> 5) * 2 + c) * 8;
        *(f32x4*)(dsw + grow + qc) =
            *(const f32x4*)(my_p + key * 80 + qc * 2);
      }
    }
    {
      bf16x8v da[2];
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        const int inrow = kc * 32 + hb * 16;
        da[kc] = *(const bf16x8v*)(my_p + col * 80 + inrow);
      }
      const unsigned qib = (unsigned)(unsigned long long)QIMG(cur) + kv_swz;
      DKV_TRLOOP(accDK, da[0], da[1], qib);
    }
#undef DKV_TRLOOP
    __syncthreads();
    cur ^= 1;
  }
#undef QIMG
#undef DOIMG

  // write dK/dV. D-layout: row i = key_rel = DROW(r,hb), col j = feature
  // = t*32 + (lane&31). OUT_BF16 (no GQA): each element written exactly
  // once -> direct bf16 stores, no fp32 scratch/memset/convert pass.
  // GQA (ngrp>1): head-groups collide on (b, key, kvh) -> fp32 atomics.
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key_abs = kv0 + DROW(r, hb);
      const int feat = t * 32 + col;
      const long long off =
          ((long long)b * S + key_abs) * (long long)(KVH * D) +
          (long long)kvh * D + feat;
      // dv may target a strided slice of a fused dqkv buffer
      const long long offv = ((long long)b * S + key_abs) * dvstride +
                             (long long)kvh * D + feat;
      if (OUT_BF16) {
        ((short*)dkg)[off] = f2bf(accDK[t][r]);
        ((short*)dvg)[offv] = f2bf(accDV[t][r]);
      } else if (ngrp > 1) {
        atomicAdd((float*)dkg + off, accDK[t][r]);
        atomicAdd((float*)dvg + offv, accDV[t][r]);
      } else {
        ((float*)dkg)[off] += accDK[t][r];
        ((float*)dvg)[offv] += accDV[t][r];
      }
    }
  }
}

// ---------------------------------------------------------------------
// Backward dk/dv, KEY ON THE LANE (default body; the kernel above stays
// selectable as FMS_AMD_ATTN_DKV=legacy). Same grid, staging images and
// formulas; the S and dP chains run with their operands swapped,
//   S  = Q  K^T   (A = plain reads of the Q image,  B = K tile)
//   dP = dO V^T   (A = plain reads of the dO image, B = V registers)
// so the accumulators are S[q][key]: lane&31 is the key and register r
// is q row DROW(r, hb). P and dS then ARE the B-operand of
//   dV^T[feat][key] += dO^T P     dK^T[feat][key] += Q^T dS
// straight from the lane's own registers: the k-slice order of an mfma
// is free as long as A agrees, so slice kc takes registers kc*8..kc*8+7
// (q rows 16kc + 4hb + {0..3} and 16kc + 8 + 4hb + {0..3}) and A reads
// exactly those two 4-row groups of the image with ds_read_b64_tr_b16.
// No P/dS transpose buffer, no LDS round trip, ONE barrier per q step.
//  - lse*log2e and delta are per register now: the waves stage the 32+32
//    floats of the next q step into a double-buffered 256 B region.
//  - The next Q/dO chunks are fetched into registers once the softmax
//    math of a step is done and committed to the other image at its end.
//  - dS is published from registers: a permlane32_swap per register pair
//    (pack_pT_chunk) gives each lane 8 consecutive q of its key row. The
//    workspace is tiled (ws_tiled, see pub_off below): one store
//    instruction of a wave writes 1 KB contiguously, and the dq kernel's
//    staging reads 1 KB per 32 lanes.
//  - The [feat][key] accumulators are transposed per 32-feature block
//    through the wave's own K tile (free after the loop), so the stores
//    and GQA atomics keep the row = key, 128 B-per-half-wave pattern.
// ---------------------------------------------------------------------
template <int O>
__device__ __forceinline__ void tr_issue4x2(unsigned b0, unsigned b1,
                                            U2x64& r0, U2x64& r1) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4 offset:%c6\n\t"
      "ds_read_b64_tr_b16 %1, %5 offset:%c7\n\t"
      "ds_read_b64_tr_b16 %2, %4 offset:%c8\n\t"
      "ds_read_b64_tr_b16 %3, %5 offset:%c9"
      : "=&v"(r0.u[0]), "=&v"(r0.u[1]), "=&v"(r1.u[0]), "=&v"(r1.u[1])
      : "v"(b0), "v"(b1), "i"(O), "i"(O + 256), "i"(O + 512), "i"(O + 768)
      : "memory");
}

// fragments of 32-feature block t (t is a constant after unrolling)
__device__ __forceinline__ void kl_issue(int t, unsigned b0, unsigned b1,
                                         U2x64& r0, U2x64& r1) {
  switch (t) {
    case 0: tr_issue4x2<0>(b0, b1, r0, r1); break;
    case 1: tr_issue4x2<2048>(b0, b1, r0, r1); break;
    case 2: tr_issue4x2<4096>(b0, b1, r0, r1); break;
    default: tr_issue4x2<6144>(b0, b1, r0, r1); break;
  }
}

// B-operand slice from 8 accumulator registers, in register order
__device__ __forceinline__ bf16x8v pack_slice(const float* p) {
  U8 b;
  b.u[0] = pack2(p[0], p[1]);
  b.u[1] = pack2(p[2], p[3]);
  b.u[2] = pack2(p[4], p[5]);
  b.u[3] = pack2(p[6], p[7]);
  return b.v;
}

//
// DOCMASK (never with PUBLISH_DS): doce = (b, s) int32 start of the next
// document after the key's (s for the last); query i sees key j iff
// j <= i < doce[j]. Each lane holds its key's end, clamped into
// [key + 1, S]; the q loop stops at the end of the block's last key
// rounded up to 32, which is the block's maximum and workgroup-uniform.
template <int D, bool OUT_BF16, bool PUBLISH_DS, bool DOCMASK = false>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2) void
attn_bwd_dkv_keylane_kernel(
    const short* __restrict__ dog, const short* __restrict__ qg,
    const short* __restrict__ kg, const short* __restrict__ vg,
    const float* __restrict__ lseg, const float* __restrict__ deltag,
    void* __restrict__ dkg, void* __restrict__ dvg,
    short* __restrict__ dsw, int B, int S, int H,
    int KVH, float scale, long long vstride, long long dvstride, int sched,
    int ws_tiled, const int* __restrict__ doce = nullptr) {
  static_assert(!(DOCMASK && PUBLISH_DS), "masked backward is workspace-free");
  constexpr int KVB = 32;   // keys per wave; block = 4 waves = 128 keys
  constexpr int NC = D / 16;
  constexpr int NT = D / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;                           // [4][KVB][D*2] per-wave
  constexpr int IMGB = 32 * D * 2;
#define QIMG(buf) (smem + 4 * KVB * D * 2 + ((buf) ? 2 * IMGB : 0))
#define DOIMG(buf) (smem + 4 * KVB * D * 2 + IMGB + ((buf) ? 2 * IMGB : 0))
  // row constants of a q step: [2][32 lse*log2e | 32 delta] fp32
  float* rowc = (float*)(smem + 4 * KVB * D * 2 + 4 * IMGB);

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31;
  const int hb = lane >> 5;

  const AttnWork wk = attn_sched_map(blockIdx.x, S / 128, B * H, sched, true);
  const int bh = __builtin_amdgcn_readfirstlane(wk.bh);
  const int tile = __builtin_amdgcn_readfirstlane(wk.tile);
  const int b = bh / H;
  const int h = bh % H;
  const int kvh = h / (H / KVH);
  const int ngrp = H / KVH;
  const int kv0 = tile * 128 + wid * KVB;

  const long long qrow_stride = (long long)H * D;
  const long long krow_stride = (long long)KVH * D;
  const short* qbase = qg + ((long long)b * S * H + (long long)h) * D;
  const short* dobase = dog + ((long long)b * S * H + (long long)h) * D;
  const short* kbase = kg + ((long long)b * S * KVH + (long long)kvh) * D;
  const short* vbase = vg + (long long)b * S * vstride + (long long)kvh * D;

  char* my_k = k_lds + wid * KVB * D * 2;

  // this wave's K rows, staged once as a subtiled image
  {
    constexpr int CHUNKS = KVB * D / 8;     // 16 B chunks
    for (int i = lane; i < CHUNKS; i += 64) {
      const int row = i / (D / 8);
      const int cb = (i % (D / 8)) * 8;
      const long long g = (long long)(kv0 + row) * krow_stride + cb;
      *(f32x4*)(my_k + SUBT_OFF(row, cb, 8)) = *(const f32x4*)(kbase + g);
    }
  }
  // V fragments stay in registers (B-operand column = this lane's key)
  bf16x8v vreg[NC];
  {
    const short* vp = vbase + (long long)(kv0 + col) * vstride + hb * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) vreg[c] = *(const bf16x8v*)(vp + c * 16);
  }

  f32x16 accDV[NT], accDK[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    accDV[t] = (f32x16)(0.f);
    accDK[t] = (f32x16)(0.f);
  }

  const int q_start = tile * 128;
  const int t256 = threadIdx.x;
  // staging as in the kernel above: thread t owns q row t&31 and adjacent
  // column chunks. Every wave also carries the step's row constants, even
  // waves lse (pre-multiplied by log2e), odd waves delta, row = lane & 31
  // (duplicates write the same value to the same slot). The loop body is
  // branch-free so that the compiler schedules it as one block: the last
  // step re-fetches its own rows into the image nobody reads again.
  const int sq = t256 & 31;
  const int sd0 = (t256 >> 5) * ((D == 128) ? 16 : 8);
  // uniform row pointers + one 32-bit per-thread offset (Q and dO share
  // their layout): the loop carries scalars, not 64-bit vector pointers
  const short* qp_s = qbase + (long long)q_start * qrow_stride;
  const short* dop_s = dobase + (long long)q_start * qrow_stride;
  const int goff = sq * (int)qrow_stride + sd0;
  const long long qstep = 32 * qrow_stride;
  const int soff0 = SUBT_OFF(sq, sd0, 8);
  const int soff1 = SUBT_OFF(sq, sd0 + 8, 8);
  const int rcw = wid & 1;
  const float* rc_s = (rcw ? deltag : lseg) + (long long)bh * S + q_start;
  const float rc_mul = rcw ? 1.0f : 1.4426950408889634f;
  f32x4v qpre0, qpre1, dpre0, dpre1;
  float rcpre = 0.f;
#define DKV_FETCH()                                   \
  do {                                                \
    qpre0 = *(const f32x4v*)(qp_s + goff);            \
    dpre0 = *(const f32x4v*)(dop_s + goff);           \
    if constexpr (D == 128) {                         \
      qpre1 = *(const f32x4v*)(qp_s + goff + 8);      \
      dpre1 = *(const f32x4v*)(dop_s + goff + 8);     \
    }                                                 \
    rcpre = rc_s[col];                                \
  } while (0)
#define DKV_ADVANCE(on)                               \
  do {                                                \
    qp_s += (on) ? qstep : 0;                         \
    dop_s += (on) ? qstep : 0;                        \
    rc_s += (on) ? 32 : 0;                            \
  } while (0)
#define DKV_COMMIT(buf)                               \
  do {                                                \
    *(f32x4v*)(QIMG(buf) + soff0) = qpre0;            \
    *(f32x4v*)(DOIMG(buf) + soff0) = dpre0;           \
    if constexpr (D == 128) {                         \
      *(f32x4v*)(QIMG(buf) + soff1) = qpre1;          \
      *(f32x4v*)(DOIMG(buf) + soff1) = dpre1;         \
    }                                                 \
    rowc[(buf) * 64 + rcw * 32 + col] = rcpre * rc_mul; \
  } while (0)
  DKV_FETCH();
  DKV_COMMIT(0);
  __syncthreads();

  // tr-read bases into the Q/dO images (R4 = 8): in-subtile lane column,
  // row group hb of a slice (128 B), 16-lane column block. The second
  // read of a fragment sits two row groups on, where the image's 16 B
  // row-group XOR is set: it gets the ^16 base.
  const unsigned tr0 =
      (unsigned)((lane & 15) * 8 + hb * 128 + (col >> 4) * 1024);
  const unsigned tr1 = tr0 ^ 16u;
  const float scale2 = scale * 1.4426950408889634f;
  const int key = kv0 + col;
  int my_end = S, q_end = S;
  if constexpr (DOCMASK) {
    const int* dep = doce + (long long)b * S;
    my_end = doc_clamp(dep[key], key + 1, S);
    const int klast = tile * 128 + 127;
    const int e = __builtin_amdgcn_readfirstlane(
        doc_clamp(dep[klast], klast + 1, S));
    q_end = min(S, (e + 31) & ~31);
  }
  // dS workspace address = uniform base + q0 * pub_qmul + lane part; the
  // second slice sits pub_kc elements on. Row-major [bh][key][q]: lane
  // (key, hb) stores q 16kc + 8hb .. +7 of its key row. Tiled
  // [bh][key/32][q/32][kc][key%32][16 q]: the same 16 B land at
  // kc*1 KB + (2 key + hb)*16 B, so one store instruction of the wave
  // writes 1 KB contiguously and a tile is 2 KB.
  const int pub_off = ws_tiled ? col * 16 + hb * 8 : col * S + hb * 8;
  const int pub_kc = ws_tiled ? 512 : 16;
  const int pub_qmul = ws_tiled ? 32 : 1;
  short* pub_base =
      dsw + (long long)bh * S * S +
      (ws_tiled ? (long long)(kv0 / 32) * S * 32 : (long long)kv0 * S);

  int cur = 0;
  for (int q0 = q_start; q0 < q_end; q0 += 32) {
    const bool more = q0 + 32 < q_end;

    f32x16 accS = (f32x16)(0.f), accDP = (f32x16)(0.f);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int boff = SUBT_OFF(col, c * 16 + hb * 8, 8);
      const bf16x8v ka = *(const bf16x8v*)(my_k + boff);
      const bf16x8v qbf = *(const bf16x8v*)(QIMG(cur) + boff);
      const bf16x8v dbf = *(const bf16x8v*)(DOIMG(cur) + boff);
      accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qbf, ka, accS, 0, 0, 0);
      accDP = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dbf, vreg[c], accDP,
                                                      0, 0, 0);
    }

    // row constants of registers 4g..4g+3: q rows 8g + 4hb + {0..3}
    const f32x4v* lse4 = (const f32x4v*)(rowc + cur * 64) + hb;
    const f32x4v* del4 = (const f32x4v*)(rowc + cur * 64 + 32) + hb;
    const unsigned dob = (unsigned)(unsigned long long)DOIMG(cur);
    const unsigned qib = (unsigned)(unsigned long long)QIMG(cur);
    float pv[16], ds[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4v lse_q2 = lse4[2 * g];
      const f32x4v delta_q = del4[2 * g];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = g * 4 + j;
        const int q = q0 + DROW(r, hb);
        float pval = exp2f(accS[r] * scale2 - lse_q2[j]);
        if (key > q || (DOCMASK && q >= my_end)) pval = 0.f;
        pv[r] = pval;
        ds[r] = pval * (accDP[r] - delta_q[j]) * scale;
      }
    }
    const bf16x8v pb0 = pack_slice(pv), pb1 = pack_slice(pv + 8);
    const bf16x8v db0 = pack_slice(ds), db1 = pack_slice(ds + 8);

    // keep the phases apart in the schedule: hoisting the fetch or the
    // publish shuffles into the softmax math costs more registers than the
    // 256 this kernel has
    __builtin_amdgcn_sched_barrier(0);
    // fetch the next q step now that S, dP and the fp32 P/dS are dead (the
    // registers do not reach further up); the dV and dK chains cover the
    // latency. Ahead of the publish stores, so that the commit's counted
    // wait on these loads leaves the stores in flight.
    DKV_ADVANCE(more);
    DKV_FETCH();
    __builtin_amdgcn_sched_barrier(0);

    // publish this (32-key x 32-q) dS tile, 16 B per lane and slice
    if constexpr (PUBLISH_DS) {
      short* grow = pub_base + (long long)q0 * pub_qmul;   // uniform
      *(bf16x8v*)(grow + pub_off) = pack_pT_chunk(ds);
      *(bf16x8v*)(grow + pub_off + pub_kc) = pack_pT_chunk(ds + 8);
    }

    __builtin_amdgcn_sched_barrier(0);

    U2x64 fr[2][2];
    kl_issue(0, dob + tr0, dob + tr1, fr[0][0], fr[0][1]);
#define DKV_KLLOOP(ACC, B0, B1, BASE, NEXT_ISSUE)                            \
  do {                                                                       \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) {                         \
      const int pp = t & 1;                                                  \
      if (t + 1 < NT) {                                                      \
        kl_issue(t + 1, (BASE) + tr0, (BASE) + tr1, fr[pp ^ 1][0],           \
                 fr[pp ^ 1][1]);                                             \
        tr_wait<4>(fr[pp][0], fr[pp][1]);                                    \
      } else {                                                               \
        NEXT_ISSUE;                                                          \
      }                                                                      \
      ACC[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][0].v, B0,      \
                                                       ACC[t], 0, 0, 0);     \
      ACC[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[pp][1].v, B1,      \
                                                       ACC[t], 0, 0, 0);     \
    }                                                                        \
  } while (0)
    // dV^T += dO^T P; its last block overlaps the first Q^T fragments.
    // NT is even, so the last block sits in fr[1] and fr[0] is free.
    DKV_KLLOOP(accDV, pb0, pb1, dob,
               (kl_issue(0, qib + tr0, qib + tr1, fr[0][0], fr[0][1]),
                tr_wait<4>(fr[1][0], fr[1][1])));
    // dK^T += Q^T dS
    DKV_KLLOOP(accDK, db0, db1, qib, (tr_wait<0>(fr[1][0], fr[1][1])));
#undef DKV_KLLOOP

    DKV_COMMIT(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
#undef DKV_FETCH
#undef DKV_ADVANCE
#undef DKV_COMMIT
#undef QIMG
#undef DOIMG

  // write dK/dV. acc[t][r] is (feat t*32 + DROW(r, hb), key col):
  // transpose each 32x32 fp32 block through this wave's K tile (no other
  // wave touches it; DS ops of a wave execute in order) with a 16 B
  // chunk XOR on the key, then store as the kernel above does: register
  // r = key row DROW(r, hb), lane = feature, 128 B per half-wave.
  auto flush = [&](const f32x16& acc, int t, void* outg, long long rstride) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4v w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = acc[g * 4 + j];
      *(f32x4v*)(my_k + col * 128 + (((2 * g + hb) ^ (col & 7)) * 16)) = w;
    }
    __builtin_amdgcn_wave_barrier();
    // uniform row base per register + one 32-bit lane offset (the 4*hb
    // rows and the feature). dv may target a strided slice of a fused
    // dqkv buffer: rstride is its row stride.
    const long long ubase = ((long long)b * S + kv0) * rstride +
                            (long long)kvh * D + t * 32;
    const int loff = 4 * hb * (int)rstride + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int krel = DROW(r, hb);
      const float val = *(const float*)(my_k + krel * 128 +
                                        (((col >> 2) ^ (krel & 7)) * 16) +
                                        (col & 3) * 4);
      const long long uoff = ubase + (long long)DROW(r, 0) * rstride;
      if (OUT_BF16) {
        ((short*)outg + uoff)[loff] = f2bf(val);
      } else if (ngrp > 1) {
        atomicAdd((float*)outg + uoff + loff, val);
      } else {
        ((float*)outg + uoff)[loff] += val;
      }
    }
  };
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    flush(accDK[t], t, dkg, (long long)(KVH * D));
    flush(accDV[t], t, dvg, dvstride);
  }
}

// Workgroup order of the three causal kernels (attn_sched.h). Default
// balanced; FMS_AMD_ATTN_SCHED=legacy keeps the former x-fastest
// (tile, bh) order. Read once; attn_sched_mode() overrides at run time.
static int g_attn_sched = -1;

static int attn_sched_get() {
  if (g_attn_sched < 0) {
    const char* e = getenv("FMS_AMD_ATTN_SCHED");
    g_attn_sched = (e && strcmp(e, "legacy") == 0) ? ATTN_SCHED_LEGACY
                                                   : ATTN_SCHED_BALANCED;
  }
  return g_attn_sched;
}

// Largest dS workspace attn_bwd may allocate (attn_ws.h), in bytes.
// Default 4 GiB; FMS_AMD_ATTN_BWD_WS_MB overrides (MiB, 0 = never use
// the workspace). Read once; attn_bwd_ws_limit() overrides at run time.
static long long g_attn_ws_limit = -1;

static long long attn_ws_limit_get() {
  if (g_attn_ws_limit < 0) {
    long long mb = ATTN_BWD_WS_DEFAULT_MB;
    const char* e = getenv("FMS_AMD_ATTN_BWD_WS_MB");
    if (e && *e) {
      char* end = nullptr;
      const long long val = strtoll(e, &end, 10);
      if (end != e && *end == '\0' && val >= 0 && val <= (1LL << 40)) mb = val;
    }
    g_attn_ws_limit = mb << 20;
  }
  return g_attn_ws_limit;
}

// dk/dv kernel body: key-on-the-lane (default) or the former key-on-the-
// register body with its LDS transpose buffer. FMS_AMD_ATTN_DKV=legacy
// selects the latter. Read once; attn_dkv_mode() overrides at run time.
#define ATTN_DKV_KEYLANE 0
#define ATTN_DKV_LEGACY 1
static int g_attn_dkv = -1;

static int attn_dkv_get() {
  if (g_attn_dkv < 0) {
    const char* e = getenv("FMS_AMD_ATTN_DKV");
    g_attn_dkv = (e && strcmp(e, "legacy") == 0) ? ATTN_DKV_LEGACY
                                                 : ATTN_DKV_KEYLANE;
  }
  return g_attn_dkv;
}

// Backward kernels for one head dim. ds_ws != null: dkv publishes dS, dq
// consumes it. ds_ws == null: workspace-free, dkv keeps dS to itself and
// dq recomputes it (no ordering dependency between the two kernels).
template <int D>
static void attn_bwd_launch(const void* do_, const void* q, const void* k,
                            const void* v, const float* lse, void* dq,
                            void* dk, void* dv, float* delta_ws, void* ds_ws,
                            int B, int S, int H, int KVH, float scale,
                            int out_bf16, long long vstride,
                            long long dvstride, hipStream_t stream) {
  const unsigned grid = (unsigned)(S / 128) * (unsigned)(B * H);
  const int sched = attn_sched_get();
  const bool keylane = attn_dkv_get() == ATTN_DKV_KEYLANE;
  // the dS workspace layout is private to the dkv/dq pair: the key-lane
  // body publishes 2 KB tiles, the legacy body row-major
  const int ws_tiled = keylane;
  // K tiles + Q/dO images, then the row constants (key-lane) or the P/dS
  // transpose buffer (legacy)
  const int lds_dkv =
      4 * 32 * D * 2 + 4 * 32 * D * 2 + (keylane ? 2 * 64 * 4 : 4 * 32 * 80);
#define DKV_ARGS                                                              \
  (const short*)do_, (const short*)q, (const short*)k, (const short*)v, lse,  \
      delta_ws, dk, dv, (short*)ds_ws, B, S, H, KVH, scale, vstride,          \
      dvstride, sched
#define DKV_LAUNCH(OUT, PUB)                                                  \
  do {                                                                        \
    if (keylane)                                                              \
      attn_bwd_dkv_keylane_kernel<D, OUT, PUB>                                \
          <<<grid, 256, lds_dkv, stream>>>(DKV_ARGS, ws_tiled);               \
    else                                                                      \
      attn_bwd_dkv_kernel<D, OUT, PUB>                                        \
          <<<grid, 256, lds_dkv, stream>>>(DKV_ARGS);                         \
  } while (0)
  if (ds_ws) {
    // dkv FIRST: it publishes the dS workspace the dq kernel consumes
    if (out_bf16)
      DKV_LAUNCH(true, true);
    else
      DKV_LAUNCH(false, true);
    const int lds_dq = 2 * (32 * D * 2 + 32 * 128 * 2);
    attn_bwd_dq_kernel<D><<<grid, 256, lds_dq, stream>>>(
        (const short*)k, (const short*)ds_ws, (short*)dq, B, S, H, KVH, sched,
        ws_tiled);
  } else {
    if (out_bf16)
      DKV_LAUNCH(true, false);
    else
      DKV_LAUNCH(false, false);
    const int lds_dq = 2 * (32 * D * 2 + 32 * D * 2);   // dbuf K + V images
    attn_bwd_dq_recompute_kernel<D><<<grid, 256, lds_dq, stream>>>(
        (const short*)do_, (const short*)q, (const short*)k, (const short*)v,
        lse, delta_ws, (short*)dq, B, S, H, KVH, scale, vstride, sched);
  }
#undef DKV_LAUNCH
#undef DKV_ARGS
}

// Document-masked backward: always workspace-free (skipped tiles would
// leave a workspace unwritten) and always the key-lane dkv body; the dkv
// mode and the workspace limit govern unmasked calls only.
template <int D>
static void attn_bwd_doc_launch(const void* do_, const void* q, const void* k,
                                const void* v, const float* lse, void* dq,
                                void* dk, void* dv, float* delta_ws,
                                const int* doc_start, const int* doc_end,
                                int B, int S, int H, int KVH, float scale,
                                int out_bf16, long long vstride,
                                long long dvstride, hipStream_t stream) {
  const unsigned grid = (unsigned)(S / 128) * (unsigned)(B * H);
  const int sched = attn_sched_get();
  const int lds_dkv = 4 * 32 * D * 2 + 4 * 32 * D * 2 + 2 * 64 * 4;
#define DKV_DOC_LAUNCH(OUT)                                                   \
  attn_bwd_dkv_keylane_kernel<D, OUT, false, true>                            \
      <<<grid, 256, lds_dkv, stream>>>(                                       \
          (const short*)do_, (const short*)q, (const short*)k,                \
          (const short*)v, lse, delta_ws, dk, dv, (short*)nullptr, B, S, H,   \
          KVH, scale, vstride, dvstride, sched, 0, doc_end)
  if (out_bf16)
    DKV_DOC_LAUNCH(true);
  else
    DKV_DOC_LAUNCH(false);
#undef DKV_DOC_LAUNCH
  const int lds_dq = 2 * (32 * D * 2 + 32 * D * 2);   // dbuf K + V images
  attn_bwd_dq_recompute_kernel<D, true><<<grid, 256, lds_dq, stream>>>(
      (const short*)do_, (const short*)q, (const short*)k, (const short*)v,
      lse, delta_ws, (short*)dq, B, S, H, KVH, scale, vstride, sched,
      doc_start);
}

extern "C" {

// bytes < 0: query only. Returns the limit in force before the call.
long long attn_bwd_ws_limit(long long bytes) {
  const long long prev = attn_ws_limit_get();
  if (bytes >= 0) g_attn_ws_limit = bytes;
  return prev;
}

// mode < 0: query only. Returns the mode in force before the call.
int attn_sched_mode(int mode) {
  const int prev = attn_sched_get();
  if (mode >= 0) g_attn_sched = mode;
  return prev;
}

// mode < 0: query only. Returns the mode in force before the call.
int attn_dkv_mode(int mode) {
  const int prev = attn_dkv_get();
  if (mode >= 0) g_attn_dkv = mode;
  return prev;
}

void launch_attn_fwd(const void* q, const void* k, const void* v, void* o,
                     float* lse, int B, int S, int H, int KVH, int D,
                     float scale, long long vstride, hipStream_t stream) {
  const unsigned grid = (unsigned)(S / 128) * (unsigned)(B * H);
  const int sched = attn_sched_get();
  const int lds = 3 * 64 * D * 2;  // single K image + dbuf V
  if (D == 128)
    attn_fwd_kernel<128><<<grid, 256, lds, stream>>>(
        (const short*)q, (const short*)k, (const short*)v, (short*)o, lse, B,
        S, H, KVH, scale, vstride, sched);
  else
    attn_fwd_kernel<64><<<grid, 256, lds, stream>>>(
        (const short*)q, (const short*)k, (const short*)v, (short*)o, lse, B,
        S, H, KVH, scale, vstride, sched);
}

// delta[b,h,s] = rowsum(dO * O); do_ and o contiguous (b,s,h,d), d 64 or 128
void launch_attn_bwd_delta(const void* do_, const void* o, float* delta,
                           int B, int S, int H, int D, hipStream_t stream) {
  const long long rows = (long long)B * S * H;
  const unsigned grid = (unsigned)((rows * (D / 8) + 255) / 256);
  if (D == 128)
    attn_bwd_delta_kernel<16><<<grid, 256, 0, stream>>>(
        (const bf16x8*)do_, (const bf16x8*)o, delta, S, H, rows);
  else
    attn_bwd_delta_kernel<8><<<grid, 256, 0, stream>>>(
        (const bf16x8*)do_, (const bf16x8*)o, delta, S, H, rows);
}

void launch_attn_bwd(const void* do_, const void* q, const void* k,
                     const void* v, const void* o, const float* lse, void* dq,
                     void* dk, void* dv, float* delta_ws, void* ds_ws,
                     int B, int S, int H,
                     int KVH, int D, float scale, int out_bf16,
                     long long vstride, long long dvstride,
                     hipStream_t stream) {
  launch_attn_bwd_delta(do_, o, delta_ws, B, S, H, D, stream);
  if (D == 128)
    attn_bwd_launch<128>(do_, q, k, v, lse, dq, dk, dv, delta_ws, ds_ws, B, S,
                         H, KVH, scale, out_bf16, vstride, dvstride, stream);
  else
    attn_bwd_launch<64>(do_, q, k, v, lse, dq, dk, dv, delta_ws, ds_ws, B, S,
                        H, KVH, scale, out_bf16, vstride, dvstride, stream);
}

// doc_start / doc_end: (b, s) int32, see the DOCMASK kernel comments
void launch_attn_fwd_doc(const void* q, const void* k, const void* v, void* o,
                         float* lse, const int* doc_start, int B, int S,
                         int H, int KVH, int D, float scale,
                         long long vstride, hipStream_t stream) {
  const unsigned grid = (unsigned)(S / 128) * (unsigned)(B * H);
  const int sched = attn_sched_get();
  const int lds = 3 * 64 * D * 2;  // single K image + dbuf V
  if (D == 128)
    attn_fwd_kernel<128, true><<<grid, 256, lds, stream>>>(
        (const short*)q, (const short*)k, (const short*)v, (short*)o, lse, B,
        S, H, KVH, scale, vstride, sched, doc_start);
  else
    attn_fwd_kernel<64, true><<<grid, 256, lds, stream>>>(
        (const short*)q, (const short*)k, (const short*)v, (short*)o, lse, B,
        S, H, KVH, scale, vstride, sched, doc_start);
}

void launch_attn_bwd_doc(const void* do_, const void* q, const void* k,
                         const void* v, const void* o, const float* lse,
                         void* dq, void* dk, void* dv, float* delta_ws,
                         const int* doc_start, const int* doc_end, int B,
                         int S, int H, int KVH, int D, float scale,
                         int out_bf16, long long vstride, long long dvstride,
                         hipStream_t stream) {
  launch_attn_bwd_delta(do_, o, delta_ws, B, S, H, D, stream);
  if (D == 128)
    attn_bwd_doc_launch<128>(do_, q, k, v, lse, dq, dk, dv, delta_ws,
                             doc_start, doc_end, B, S, H, KVH, scale,
                             out_bf16, vstride, dvstride, stream);
  else
    attn_bwd_doc_launch<64>(do_, q, k, v, lse, dq, dk, dv, delta_ws,
                            doc_start, doc_end, B, S, H, KVH, scale,
                            out_bf16, vstride, dvstride, stream);
}

}  // extern "C"
