// MFMA fragment helpers shared by the attention kernels (attention.hip,
// attn_decode.hip): operand vector types, the in-register P -> PV operand
// pack, the subtiled LDS image and its hardware transpose reads.
//
// MFMA fragment maps (cdna4 32x32x16 bf16):
//   A[i][k]: lane l -> i = l&31,          k = (l>>5)*8 + e   (e=0..7)
//   B[k][j]: lane l -> k = (l>>5)*8 + e,  j = l&31
//   D[i][j]: lane l, reg r -> j = l&31,   i = (r&3) + 8*(r>>2) + 4*(l>>5)
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8v;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4v;

union U8 {
  bf16x8v v;
  unsigned u[4];
  bf16x8 s;
};

__device__ __forceinline__ unsigned pack2(float lo, float hi) {
  return ((unsigned)(unsigned short)f2bf(hi) << 16) |
         (unsigned short)f2bf(lo);
}

// Build the PV B-operand for one 16-key chunk from 8 P registers
// (D-layout rows (r&3)+8*(r>>2)+4*hb -> B[k=key][j=q]): cvt_pk pairs +
// permlane32_swap half-exchange (guide T12 / §B P->PV layout).
__device__ __forceinline__ bf16x8v pack_pT_chunk(const float* p) {
  unsigned w01 = pack2(p[0], p[1]);
  unsigned w23 = pack2(p[2], p[3]);
  unsigned w89 = pack2(p[4], p[5]);
  unsigned w1011 = pack2(p[6], p[7]);
  auto r1 = __builtin_amdgcn_permlane32_swap(w01, w89, false, false);
  auto r2 = __builtin_amdgcn_permlane32_swap(w23, w1011, false, false);
  U8 b;
  b.u[0] = r1[0];
  b.u[1] = r2[0];
  b.u[2] = r1[1];
  b.u[3] = r2[1];
  return b.v;
}

// row index inside a 32-row D tile for register r, half hb
#define DROW(r, hb) (((r) & 3) + 8 * ((r) >> 2) + 4 * (hb))

// ---------------------------------------------------------------------
// Shared helpers for the attention kernels: SUBTILED LDS images.
// A [R rows][D cols] bf16 tile is stored as [R/4][D/16][4][16] (each
// subtile 128 B contiguous). This single layout serves BOTH fragment
// patterns:
//  - plain B/A reads (row = lane&31, 8 consecutive cols): 16 B contiguous
//  - transposed reads via gfx950 ds_read_b64_tr_b16: a 16-lane group's
//    lane j at subtile_base + j*8 receives COLUMN j of the 4x16 subtile
//    (semantics verified on hardware: tools/tr_probe.hip).
// ---------------------------------------------------------------------
// column-block-major subtiles: tile = colblk*R4 + rowgrp (R4 = image
// rows / 4). A plain 16-lane-group read then touches 4 CONSECUTIVE
// tiles (alternating LDS bank halves); the rowgrp-bit1 16B XOR spreads
// the remaining overlap. (PMC-driven: row-group-major was 4-way.)
#define SUBT_OFF(row, col, R4) \
  ((((col) >> 4) * (R4) + ((row) >> 2)) * 128 + \
   ((((row) & 3) * 32 + ((col) & 15) * 2) ^ ((((row) >> 2) & 2) << 3)))

union U2x64 {
  unsigned long long u[2];
  bf16x8v v;
};

// Two transpose reads batched behind ONE lgkmcnt wait (each read's 4
// shorts = column lane&15 of the 4x16 subtile at its address).
__device__ __forceinline__ bf16x8v tr_read2(const char* base, int off0,
                                            int off1) {
  U2x64 r;
  const unsigned a0 = (unsigned)(unsigned long long)(base + off0);
  const unsigned a1 = (unsigned)(unsigned long long)(base + off1);
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r.u[0]), "=&v"(r.u[1])
      : "v"(a0), "v"(a1)
      : "memory");
  return r.v;
}

// Four transpose reads -> TWO A-fragments behind ONE lgkmcnt wait: the
// LDS pipe streams all four b64 reads before the single serialization
// point, so back-to-back mfmas consume both fragments densely.
struct TR4 {
  bf16x8v a, b;
};
__device__ __forceinline__ TR4 tr_read4(const char* base, int off0, int off1,
                                        int off2, int off3) {
  U2x64 r0, r1;
  const unsigned a0 = (unsigned)(unsigned long long)(base + off0);
  const unsigned a1 = (unsigned)(unsigned long long)(base + off1);
  const unsigned a2 = (unsigned)(unsigned long long)(base + off2);
  const unsigned a3 = (unsigned)(unsigned long long)(base + off3);
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %5\n\t"
      "ds_read_b64_tr_b16 %2, %6\n\t"
      "ds_read_b64_tr_b16 %3, %7\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0.u[0]), "=&v"(r0.u[1]), "=&v"(r1.u[0]), "=&v"(r1.u[1])
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3)
      : "memory");
  TR4 out;
  out.a = r0.v;
  out.b = r1.v;
  return out;
}
