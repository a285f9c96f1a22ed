// Mamba2 recurrent decode: the SSD recurrence stepped token by token from
// a given state (docs/kernels.md "Recurrent decode"). T = 1 is a decode
// step, T > 1 the tail of a prompt behind its last full chunk. For every
// (b, h) and t = 0..T-1:
//   dtf  = softplus(dt[b,t,h] + dt_bias[h])           (ssd_prep's expression)
//   a    = exp(dtf * A_h),  A_h = -exp(A_log[h])
//   s[p][n] = a * s[p][n] + (dtf * x[b,t,h,p]) * B[b,t,g,n]   g = h / (H/G)
//   y[p] = sum_n s[p][n] * C[b,t,g,n] + D[h] * x[b,t,h,p]
//   out[b,t,h*P+p] = bf16(y[p] * z * sigmoid(z))      (ssd_ygate's silu)
//
// state (b, H, P, N) fp32 is read once and written once per call whatever
// T is: it lives in registers across the token loop.
//
// Mapping: one 64-lane workgroup per (b, h, 16 rows of P), so that a
// batch of one still spreads b*H*ceil(P/16) waves over the chip. Lane
// (pl, nq) = (lane / 4, lane % 4) owns row p = 16*pb + pl and, of that
// row, the N/4 elements n = 16k + 4nq + e (k < N/16, e < 4): state vector
// k of the four lanes of a row is one contiguous 64-byte piece, so the
// state moves as 16-byte accesses with consecutive lanes on consecutive
// bytes. B_t / C_t arrive as the matching 8-byte bf16x4 pieces. The
// n-reduction is N/4 lane-local fmas in four independent chains plus a
// 4-lane xor shuffle. Rows p >= P of the last block (P % 16 == 8) load
// row P-1 and store nothing.
//
// The next token's x / z / dt / B / C loads are issued before the current
// token's arithmetic; the last token re-reads itself. One loop body
// serves every token, the arithmetic is explicit fmaf in a fixed order
// and there are no atomics: one call over T tokens and two calls over a
// split of them give the same bits. No address or loop bound depends on
// array contents. Indexing is 64-bit.
#include "common.h"

template <int N>
struct StepTok {
  short x, z, dt;
  bf16x4 B[N / 16], C[N / 16];
};

template <int N>
__device__ __forceinline__ void step_load(
    StepTok<N>& k, const short* __restrict__ x, const short* __restrict__ dt,
    const short* __restrict__ B, const short* __restrict__ C,
    const short* __restrict__ z, long long row, long long sx, long long sdt,
    long long sB, long long sC, long long sz, int xcol, int h, int ncol) {
  k.x = x[row * sx + xcol];
  k.z = z[row * sz + xcol];
  k.dt = dt[row * sdt + h];
  const short* Bp = B + row * sB + ncol;
  const short* Cp = C + row * sC + ncol;
#pragma unroll
  for (int v = 0; v < N / 16; ++v) {
    k.B[v] = *(const bf16x4*)(Bp + 16 * v);
    k.C[v] = *(const bf16x4*)(Cp + 16 * v);
  }
}

template <int N>
__global__ __launch_bounds__(64) void ssd_step_kernel(
    float* __restrict__ state, const short* __restrict__ x,
    const short* __restrict__ dt, const short* __restrict__ B,
    const short* __restrict__ C, const short* __restrict__ z,
    const float* __restrict__ dt_bias, const float* __restrict__ A_log,
    const float* __restrict__ Dp, short* __restrict__ out, int T, int H,
    int G, int P, int PB, long long sx, long long sdt, long long sB,
    long long sC, long long sz) {
  constexpr int NV = N / 16;             // f32x4 state vectors per lane
  const int lane = threadIdx.x;
  const int pl = lane >> 2, nq = lane & 3;
  long long w = blockIdx.x;
  const int pb = (int)(w % PB);
  w /= PB;
  const int h = (int)(w % H);
  const long long b = w / H;
  const int p = pb * 16 + pl;
  const bool valid = p < P;
  const int pc = valid ? p : P - 1;
  const int g = h / (H / G);
  const int xcol = h * P + pc;
  const int ncol = g * N + 4 * nq;

  float* sp = state + ((b * H + h) * P + pc) * (long long)N + 4 * nq;
  float s[NV][4];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const f32x4 q = *(const f32x4*)(sp + 16 * v);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[v][e] = q.v[e];
  }
  const float bh = dt_bias[h];
  const float A = -__expf(A_log[h]);
  const float Dh = Dp[h];
  const long long r0 = b * T;

  StepTok<N> nxt;
  step_load<N>(nxt, x, dt, B, C, z, r0, sx, sdt, sB, sC, sz, xcol, h, ncol);
  for (int t = 0; t < T; ++t) {
    const StepTok<N> cur = nxt;
    const int tn = t + 1 < T ? t + 1 : t;
    step_load<N>(nxt, x, dt, B, C, z, r0 + tn, sx, sdt, sB, sC, sz, xcol, h,
                 ncol);
    const float xs = bf2f(cur.dt) + bh;
    const float dtf = xs > 20.f ? xs : log1pf(__expf(xs));
    const float a = __expf(dtf * A);
    const float xf = bf2f(cur.x);
    const float xdt = dtf * xf;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float in = xdt * bf2f(cur.B[v].v[e]);
        s[v][e] = fmaf(a, s[v][e], in);
        acc[e] = fmaf(s[v][e], bf2f(cur.C[v].v[e]), acc[e]);
      }
    }
    float y = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    y += __shfl_xor(y, 1, 64);
    y += __shfl_xor(y, 2, 64);
    y = fmaf(Dh, xf, y);
    const float zf = bf2f(cur.z);
    const float sg = 1.f / (1.f + __expf(-zf));
    if (valid && nq == 0)
      out[((r0 + t) * H + h) * (long long)P + p] = f2bf(y * zf * sg);
  }
  if (valid) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      f32x4 q;
#pragma unroll
      for (int e = 0; e < 4; ++e) q.v[e] = s[v][e];
      *(f32x4*)(sp + 16 * v) = q;
    }
  }
}

extern "C" {

// Row r = b*T + t of x / z / dt / B / C starts r * (its stride) elements
// behind the base pointer. N in {16, 32, 64, 128, 256}; P % 8 == 0.
void launch_ssd_step(float* state, const void* x, const void* dt,
                     const void* B, const void* C, const void* z,
                     const float* dt_bias, const float* A_log, const float* D,
                     void* out, long long b, int T, int H, int G, int P,
                     int N, long long sx, long long sdt, long long sB,
                     long long sC, long long sz, hipStream_t stream) {
  const int PB = (P + 15) / 16;
  const unsigned grid = (unsigned)(b * H * PB);
#define SSD_STEP(NV)                                                        \
  ssd_step_kernel<NV><<<grid, 64, 0, stream>>>(                             \
      state, (const short*)x, (const short*)dt, (const short*)B,            \
      (const short*)C, (const short*)z, dt_bias, A_log, D, (short*)out, T,  \
      H, G, P, PB, sx, sdt, sB, sC, sz)
  if (N == 16) SSD_STEP(16);
  else if (N == 32) SSD_STEP(32);
  else if (N == 64) SSD_STEP(64);
  else if (N == 128) SSD_STEP(128);
  else SSD_STEP(256);
#undef SSD_STEP
}

}  // extern "C"
