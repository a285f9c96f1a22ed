// Python bindings for the CDNA4 kernel library (fms_fsdp_amd._C).
// Pure dispatch: shape/dtype checks + launch on the current HIP stream.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <string>
#include <tuple>
#include <vector>

#include "attn_decode_plan.h"
#include "attn_ws.h"

using torch::Tensor;

extern "C" {
void launch_rmsnorm_fwd(const void*, const void*, void*, float*, int, int,
                        float, hipStream_t);
void launch_rmsnorm_bwd(const void*, const void*, const void*, const float*,
                        const void*, void*, float*, int, int, hipStream_t);
void launch_add_rmsnorm_fwd(const void*, const void*, const void*, void*,
                            void*, float*, int, int, float, hipStream_t);
int rmsnorm_bwd_grid(int);
int rmsnorm_bwd_nparts(int, int);
void launch_rmsnorm_bwd_fused(const void*, const void*, const void*,
                              const float*, const void*, void*, float*, int,
                              float*, void*, int, int, int, hipStream_t);
void launch_rmsnorm_dw_store(const float*, void*, int, int, hipStream_t);
void launch_rope(const void*, void*, const float*, const float*, int, int,
                 int, int, int, long long, long long, hipStream_t);
void launch_swiglu_fwd(const void*, void*, long long, int, hipStream_t);
void launch_swiglu_bwd(const void*, const void*, void*, long long, int,
                       hipStream_t);
void launch_transpose_bf16(const void*, void*, long long, long long,
                           long long, hipStream_t);
void launch_ce_fwd_bwd(void*, const long long*, float*, const float*,
                       long long, int, int, hipStream_t);
void launch_adamw(float*, const void*, int, float*, float*, void*, int,
                  long long, float, float, float, float, float, float, float,
                  const float*, hipStream_t);
void launch_sqnorm(const void*, int, float*, long long, hipStream_t);
void launch_attn_fwd(const void*, const void*, const void*, void*, float*,
                     int, int, int, int, int, float, long long, hipStream_t);
void launch_attn_bwd(const void*, const void*, const void*, const void*,
                     const void*, const float*, void*, void*, void*, float*,
                     void*, int, int, int, int, int, float, int,
                     long long, long long, hipStream_t);
void launch_attn_fwd_doc(const void*, const void*, const void*, void*, float*,
                         const int*, int, int, int, int, int, float,
                         long long, hipStream_t);
void launch_attn_bwd_doc(const void*, const void*, const void*, const void*,
                         const void*, const float*, void*, void*, void*,
                         float*, const int*, const int*, int, int, int, int,
                         int, float, int, long long, long long, hipStream_t);
void launch_attn_bwd_delta(const void*, const void*, float*, int, int, int,
                           int, hipStream_t);
void launch_kv_append(const void*, const void*, const void*, void*, void*,
                      void*, const float*, const float*, int, int, int, int,
                      int, long long, long long, long long, long long,
                      long long, hipStream_t);
void launch_attn_decode(const void*, const void*, const void*, void*, float*,
                        float*, float*, int, int, int, int, int, long long,
                        int, float, hipStream_t);
int attn_sched_mode(int);
int attn_dkv_mode(int);
long long attn_bwd_ws_limit(long long);
void launch_cconv_fwd(const void*, const void*, const float*, void*, int,
                      int, int, int, const int*, hipStream_t);
void launch_cconv_bwd(const void*, const void*, const void*, const float*,
                      void*, void*, float*, float*, int, int, int, int,
                      const int*, const int*, hipStream_t);
int launch_gemm_nt(const void*, const void*, void*, int, int, int,
                   hipStream_t);
void launch_segsum_exp_fwd(const float*, void*, long long, int, hipStream_t);
void launch_segsum_exp_bwd(const void*, const float*, float*, long long, int,
                           hipStream_t);
void launch_ssd_prep_fwd(const void*, const float*, const float*, float*,
                         float*, long long, int, int, long long, hipStream_t);
void launch_ssd_prep_bwd(const float*, const float*, const void*,
                         const float*, const float*, void*, float*, float*,
                         long long, int, int, long long, long long,
                         hipStream_t);
void launch_ssd_xdt_fwd(const void*, const float*, const float*, void*, void*,
                        long long, int, int, int, long long, const int*, int,
                        hipStream_t);
void launch_ssd_xdt_bwd(const void*, const void*, const void*, const float*,
                        const float*, void*, float*, float*, long long, int,
                        int, int, long long, long long, const int*, int,
                        hipStream_t);
void launch_ssd_sl_fwd(const float*, const void*, void*, long long, int, int,
                       int, const int*, int, hipStream_t);
void launch_ssd_sl_bwd(const void*, const void*, const float*, void*, float*,
                       long long, int, int, int, const int*, int,
                       hipStream_t);
void launch_ssd_ygate_fwd(const void*, const void*, const float*, const void*,
                          const float*, const void*, void*, long long, int,
                          int, int, int, long long, long long, const int*,
                          int, hipStream_t);
void launch_ssd_ygate_bwd(const void*, const void*, const void*, const float*,
                          const void*, const float*, const void*, void*,
                          void*, float*, void*, float*, void*, long long, int,
                          int, int, int, long long, long long, long long,
                          long long, const int*, int, hipStream_t);
void launch_cconv_update(void*, const void*, const void*, const float*, void*,
                         long long, int, int, int, long long, hipStream_t);
void launch_ssd_step(float*, const void*, const void*, const void*,
                     const void*, const void*, const float*, const float*,
                     const float*, void*, long long, int, int, int, int, int,
                     long long, long long, long long, long long, long long,
                     hipStream_t);
}

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

#define CHECK_BF16_CONTIG(t)                                        \
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, #t " must be bf16"); \
  TORCH_CHECK(t.is_contiguous(), #t " must be contiguous");

std::tuple<Tensor, Tensor> rmsnorm_fwd(Tensor x, Tensor w, double eps) {
  CHECK_BF16_CONTIG(x);
  CHECK_BF16_CONTIG(w);
  const int rows = x.size(0), H = x.size(1);
  TORCH_CHECK(H % 8 == 0, "H must be divisible by 8");
  auto y = torch::empty_like(x);
  auto rinv = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  launch_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                     rinv.data_ptr<float>(), rows, H, (float)eps,
                     cur_stream());
  return {y, rinv};
}

static void check_rmsnorm_bwd_args(const Tensor& dy, const Tensor& x,
                                   const Tensor& w, const Tensor& rinv,
                                   const c10::optional<Tensor>& dextra) {
  CHECK_BF16_CONTIG(dy);
  CHECK_BF16_CONTIG(x);
  CHECK_BF16_CONTIG(w);
  TORCH_CHECK(x.dim() == 2 && dy.sizes() == x.sizes(),
              "dy and x must be (rows, H)");
  const int rows = x.size(0), H = x.size(1);
  TORCH_CHECK(H % 8 == 0, "H must be divisible by 8");
  TORCH_CHECK(w.numel() == H, "w must have H elements");
  TORCH_CHECK(rinv.scalar_type() == torch::kFloat32 && rinv.is_contiguous() &&
                  rinv.numel() == rows,
              "rinv must be fp32 with one element per row");
  if (dextra.has_value()) {
    TORCH_CHECK(dextra->scalar_type() == torch::kBFloat16 &&
                    dextra->is_contiguous() && dextra->sizes() == x.sizes(),
                "dextra must have x's shape and dtype");
  }
}

// dx and dw in one pass over dy and x (rmsnorm.hip): per-block fp32
// partials, summed in a fixed order, so dw is deterministic and needs no
// zero-fill. H > 8192 keeps the two-kernel path with fp32 atomics.
std::tuple<Tensor, Tensor> rmsnorm_bwd(Tensor dy, Tensor x, Tensor w,
                                       Tensor rinv,
                                       c10::optional<Tensor> dextra) {
  check_rmsnorm_bwd_args(dy, x, w, rinv, dextra);
  const int rows = x.size(0), H = x.size(1);
  const void* de = dextra.has_value() ? dextra->data_ptr() : nullptr;
  auto f32 = x.options().dtype(torch::kFloat32);
  auto dx = torch::empty_like(x);
  const int nparts = rmsnorm_bwd_nparts(rows, H);
  if (nparts == 0) {
    auto dw = torch::zeros({H}, f32);
    launch_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                       rinv.data_ptr<float>(), de, dx.data_ptr(),
                       dw.data_ptr<float>(), rows, H, cur_stream());
    return {dx, dw};
  }
  auto dw = torch::empty({H}, f32);
  auto part = torch::empty({nparts, H}, f32);
  launch_rmsnorm_bwd_fused(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                           rinv.data_ptr<float>(), de, dx.data_ptr(),
                           part.data_ptr<float>(), nparts,
                           dw.data_ptr<float>(), nullptr, 0, rows, H,
                           cur_stream());
  return {dx, dw};
}

// rmsnorm_bwd with dw rounded to bf16 straight into dw_dst (a slice of
// the sharded runtime's flat grad buffer): accumulate=false overwrites,
// accumulate=true adds to what is there with one rounding. Returns dx.
Tensor rmsnorm_bwd_into(Tensor dy, Tensor x, Tensor w, Tensor rinv,
                        c10::optional<Tensor> dextra, Tensor dw_dst,
                        bool accumulate) {
  check_rmsnorm_bwd_args(dy, x, w, rinv, dextra);
  const int rows = x.size(0), H = x.size(1);
  TORCH_CHECK(dw_dst.scalar_type() == torch::kBFloat16 &&
                  dw_dst.is_contiguous() && dw_dst.numel() == H &&
                  dw_dst.device() == x.device(),
              "dw_dst must be contiguous bf16 with H elements on x's device");
  const void* de = dextra.has_value() ? dextra->data_ptr() : nullptr;
  auto f32 = x.options().dtype(torch::kFloat32);
  auto dx = torch::empty_like(x);
  const int mode = accumulate ? 2 : 1;
  const int nparts = rmsnorm_bwd_nparts(rows, H);
  if (nparts == 0) {
    auto dw = torch::zeros({H}, f32);
    launch_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                       rinv.data_ptr<float>(), de, dx.data_ptr(),
                       dw.data_ptr<float>(), rows, H, cur_stream());
    launch_rmsnorm_dw_store(dw.data_ptr<float>(), dw_dst.data_ptr(), mode, H,
                            cur_stream());
    return dx;
  }
  auto part = torch::empty({nparts, H}, f32);
  launch_rmsnorm_bwd_fused(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                           rinv.data_ptr<float>(), de, dx.data_ptr(),
                           part.data_ptr<float>(), nparts, nullptr,
                           dw_dst.data_ptr(), mode, rows, H, cur_stream());
  return dx;
}

// Get/set the block count cap of the fused RMSNorm backward (None =
// query). Returns the value in force before the call. Tuning and test
// knob only: the value is an unsynchronised process-global.
int64_t rmsnorm_bwd_grid_py(c10::optional<int64_t> grid) {
  if (grid.has_value())
    TORCH_CHECK(*grid >= 1 && *grid <= 65536,
                "rmsnorm_bwd_grid: expected 1..65536, got ", *grid);
  return rmsnorm_bwd_grid(grid.has_value() ? (int)*grid : -1);
}

std::tuple<Tensor, Tensor, Tensor> add_rmsnorm_fwd(Tensor x, Tensor res,
                                                   Tensor w, double eps) {
  CHECK_BF16_CONTIG(x);
  CHECK_BF16_CONTIG(res);
  const int rows = x.size(0), H = x.size(1);
  auto y = torch::empty_like(x);
  auto s_out = torch::empty_like(x);
  auto rinv = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  launch_add_rmsnorm_fwd(x.data_ptr(), res.data_ptr(), w.data_ptr(),
                         y.data_ptr(), s_out.data_ptr(),
                         rinv.data_ptr<float>(), rows, H, (float)eps,
                         cur_stream());
  return {y, s_out, rinv};
}

// (b, s, h, d) bf16 view, contiguous within a (b, s) row, uniform row
// stride — a last-dim slice of a fused qkv projection qualifies.
static long long row_stride4(const Tensor& t) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, "expected bf16");
  TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1 &&
                  t.stride(2) == t.size(3) &&
                  t.stride(1) >= t.size(2) * t.size(3) &&
                  t.stride(0) == t.size(1) * t.stride(1),
              "expected row-contiguous (b,s,h,d) view");
  return (long long)t.stride(1);
}

std::tuple<Tensor, Tensor> rope_fwd(Tensor q, Tensor k, Tensor cos,
                                    Tensor sin, bool conj) {
  TORCH_CHECK(cos.scalar_type() == torch::kFloat32 && cos.is_contiguous());
  const int b = q.size(0), s = q.size(1), h = q.size(2), d = q.size(3);
  const int kvh = k.size(2);
  const long long qs = row_stride4(q), ks = row_stride4(k);
  TORCH_CHECK((d / 2) % 4 == 0, "head_dim/2 must be divisible by 4");
  auto qo = torch::empty({b, s, h, d}, q.options());
  auto ko = torch::empty({b, s, kvh, d}, k.options());
  launch_rope(q.data_ptr(), qo.data_ptr(), cos.data_ptr<float>(),
              sin.data_ptr<float>(), b, s, h, d, conj, qs,
              (long long)h * d, cur_stream());
  launch_rope(k.data_ptr(), ko.data_ptr(), cos.data_ptr<float>(),
              sin.data_ptr<float>(), b, s, kvh, d, conj, ks,
              (long long)kvh * d, cur_stream());
  return {qo, ko};
}

// Rotate `src` (contiguous (b,s,h,d)) and scatter into `dst`, a
// row-strided view (slice of a fused dqkv grad buffer). Used by the
// fused qkv+rope+attention backward.
void rope_into(Tensor src, Tensor dst, Tensor cos, Tensor sin, bool conj) {
  const int b = src.size(0), s = src.size(1), h = src.size(2),
            d = src.size(3);
  const long long is = row_stride4(src), os = row_stride4(dst);
  TORCH_CHECK(dst.size(2) == h && dst.size(3) == d);
  launch_rope(src.data_ptr(), dst.data_ptr(), cos.data_ptr<float>(),
              sin.data_ptr<float>(), b, s, h, d, conj, is, os,
              cur_stream());
}

Tensor swiglu_fwd(Tensor gu) {
  CHECK_BF16_CONTIG(gu);
  const long long rows = gu.size(0);
  const int H2 = gu.size(1);
  TORCH_CHECK(H2 % 16 == 0);
  auto h = torch::empty({rows, H2 / 2}, gu.options());
  launch_swiglu_fwd(gu.data_ptr(), h.data_ptr(), rows, H2 / 2, cur_stream());
  return h;
}

Tensor swiglu_bwd(Tensor dy, Tensor gu) {
  CHECK_BF16_CONTIG(dy);
  CHECK_BF16_CONTIG(gu);
  const long long rows = gu.size(0);
  const int H2 = gu.size(1);
  auto dgu = torch::empty_like(gu);
  launch_swiglu_bwd(dy.data_ptr(), gu.data_ptr(), dgu.data_ptr(), rows,
                    H2 / 2, cur_stream());
  return dgu;
}

// src (rows, cols) bf16 with unit column stride and a row stride >= cols
// (a column slice of a wider buffer qualifies) -> contiguous (cols, rows).
static bool transpose_src_ok(const Tensor& t) {
  return t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.dim() == 2 &&
         t.size(1) % 8 == 0 && t.size(0) > 0 && t.size(1) > 0 &&
         t.stride(1) == 1 && t.stride(0) >= t.size(1) &&
         t.stride(0) % 8 == 0 &&
         reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// `out`, if given, is the contiguous (cols, rows) destination.
Tensor transpose_bf16(Tensor src, c10::optional<Tensor> out) {
  TORCH_CHECK(transpose_src_ok(src),
              "transpose_bf16: src must be a 2-D bf16 GPU tensor, cols % 8 == "
              "0, unit column stride, row stride a multiple of 8 and >= "
              "cols, 16-byte aligned");
  const long long rows = src.size(0), cols = src.size(1);
  TORCH_CHECK((rows + 63) / 64 * ((cols + 63) / 64) < (1LL << 31),
              "transpose_bf16: too many tiles for one grid");
  Tensor dst;
  if (out.has_value()) {
    dst = *out;
    TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == torch::kBFloat16 &&
                    dst.dim() == 2 && dst.size(0) == cols &&
                    dst.size(1) == rows && dst.is_contiguous() &&
                    reinterpret_cast<uintptr_t>(dst.data_ptr()) % 16 == 0,
                "transpose_bf16: out must be a contiguous, 16-byte aligned "
                "bf16 GPU tensor of shape (cols, rows)");
  } else {
    dst = torch::empty({cols, rows}, src.options());
  }
  launch_transpose_bf16(src.data_ptr(), dst.data_ptr(), rows, cols,
                        src.stride(0), cur_stream());
  return dst;
}

// dW = dy2^T @ x2 into gview (out, in) with the operands that `mode` names
// transposed first, so that the GEMM finds them contiguous along the
// tokens: bit 0 = dy2 (tokens, out), bit 1 = x2 (tokens, in). Mode 3 is
// the forward's GEMM class (BLAS "TN"), 1 is "NN", 2 is "TT"; the
// untransposed call is the "NT" class. The transposed copies come from
// the caching allocator and die with this call (stream-ordered reuse).
// accumulate=false overwrites: beta is 0 and gview's old contents are
// never read.
static int64_t wgrad_tn_count = 0;

void wgrad_tn(Tensor dy2, Tensor x2, Tensor gview, bool accumulate,
              int64_t mode) {
  TORCH_CHECK(mode >= 1 && mode <= 3, "wgrad_tn: mode must be 1, 2 or 3");
  TORCH_CHECK(dy2.dim() == 2 && x2.dim() == 2 && dy2.size(0) == x2.size(0),
              "wgrad_tn: dy2 (tokens, out) and x2 (tokens, in) expected");
  TORCH_CHECK(gview.scalar_type() == torch::kBFloat16 && gview.dim() == 2 &&
                  gview.size(0) == dy2.size(1) && gview.size(1) == x2.size(1),
              "wgrad_tn: gview must be bf16 (out, in)");
  TORCH_CHECK(dy2.size(0) % 8 == 0, "wgrad_tn: tokens % 8 != 0");
  Tensor a = (mode & 1) ? transpose_bf16(dy2, c10::nullopt) : dy2.t();
  Tensor b = (mode & 2) ? transpose_bf16(x2, c10::nullopt).t() : x2;
  at::addmm_out(gview, gview, a, b, accumulate ? 1 : 0, 1);
  ++wgrad_tn_count;
}

// Calls of wgrad_tn so far: lets a test see which route a backward took.
int64_t wgrad_tn_calls() { return wgrad_tn_count; }

// dx = dy2 @ w for dy2 (tokens, out) and a weight w (out, in). As it
// stands the product finds w strided along the reduction (BLAS "NN");
// with w transposed first by transpose.hip it is dy2 @ wT^T, the forward's
// class ("TN"). dy2 is read in place: unit column stride and a row stride
// >= out (the fused dqkv buffer and its column slices qualify). The
// transposed weight comes from the caching allocator and dies with this
// call (stream-ordered reuse): nothing is cached, so nothing has to be
// invalidated when the optimizer or the sharded runtime writes w.
static int64_t dgrad_tn_count = 0;

Tensor dgrad_tn(Tensor dy2, Tensor w) {
  TORCH_CHECK(dy2.is_cuda() && dy2.scalar_type() == torch::kBFloat16 &&
                  dy2.dim() == 2 && dy2.size(0) > 0 && dy2.size(1) > 0 &&
                  dy2.stride(1) == 1 && dy2.stride(0) >= dy2.size(1),
              "dgrad_tn: dy2 must be a bf16 GPU tensor (tokens, out) with "
              "unit column stride and a row stride >= out");
  TORCH_CHECK(transpose_src_ok(w) && w.size(0) % 8 == 0,
              "dgrad_tn: w must be a bf16 GPU tensor (out, in), out % 8 == 0, "
              "in % 8 == 0, unit column stride, row stride a multiple of 8 "
              "and >= in, 16-byte aligned");
  TORCH_CHECK(dy2.size(1) == w.size(0) && dy2.device() == w.device(),
              "dgrad_tn: dy2 (tokens, out) and w (out, in) on one device "
              "expected");
  Tensor wT = transpose_bf16(w, c10::nullopt);   // (in, out), contiguous
  Tensor dx = at::mm(dy2, wT.t());
  ++dgrad_tn_count;
  return dx;
}

// Calls of dgrad_tn so far: lets a test see which route a backward took.
int64_t dgrad_tn_calls() { return dgrad_tn_count; }

void ce_fwd_bwd(Tensor logits, Tensor labels, Tensor loss_sum, Tensor denom,
                int64_t ignore_index) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(labels.scalar_type() == torch::kInt64 && labels.is_contiguous());
  TORCH_CHECK(logits.dim() == 2, "logits must be (rows, V)");
  const int rows = logits.size(0), V = logits.size(1);
  // rows are read and written as 16-byte vectors
  TORCH_CHECK(V % 8 == 0, "V must be divisible by 8");
  TORCH_CHECK(labels.numel() == rows, "labels must have one entry per row");
  TORCH_CHECK(loss_sum.scalar_type() == torch::kFloat32 &&
                  denom.scalar_type() == torch::kFloat32,
              "loss_sum and denom must be fp32");
  launch_ce_fwd_bwd(logits.data_ptr(),
                    reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()),
                    loss_sum.data_ptr<float>(), denom.data_ptr<float>(),
                    (long long)ignore_index, rows, V, cur_stream());
}

void adamw(Tensor p, Tensor g, Tensor m, Tensor v, double step, double lr,
           double b1, double b2, double eps, double wd,
           c10::optional<Tensor> grad_scale,
           c10::optional<Tensor> p_bf16_out) {
  TORCH_CHECK(p.scalar_type() == torch::kFloat32 && p.is_contiguous());
  const long long n = p.numel();
  TORCH_CHECK(n % 4 == 0, "shard size must be divisible by 4");
  auto dt_code = [](torch::ScalarType t) {
    if (t == torch::kBFloat16) return 1;
    if (t == torch::kFloat16) return 2;
    TORCH_CHECK(t == torch::kFloat32, "dtype must be fp32/bf16/fp16");
    return 0;
  };
  const int gdt = dt_code(g.scalar_type());
  TORCH_CHECK(g.numel() == n && g.is_contiguous(),
              "g must be contiguous with p's element count");
  TORCH_CHECK(m.scalar_type() == torch::kFloat32 && m.numel() == n &&
                  m.is_contiguous(),
              "m must be contiguous fp32 with p's element count");
  TORCH_CHECK(v.scalar_type() == torch::kFloat32 && v.numel() == n &&
                  v.is_contiguous(),
              "v must be contiguous fp32 with p's element count");
  int odt = 0;
  if (p_bf16_out.has_value()) {
    odt = dt_code(p_bf16_out->scalar_type());
    TORCH_CHECK(odt != 0, "low-precision publish target must be bf16/fp16");
    TORCH_CHECK(p_bf16_out->numel() == n && p_bf16_out->is_contiguous(),
                "publish target must be contiguous with p's element count");
  }
  if (grad_scale.has_value())
    TORCH_CHECK(grad_scale->scalar_type() == torch::kFloat32 &&
                    grad_scale->numel() == 1,
                "grad_scale must be a single fp32 value");
  const float bc1 = 1.f - powf((float)b1, (float)step);
  const float bc2 = 1.f - powf((float)b2, (float)step);
  launch_adamw(p.data_ptr<float>(), g.data_ptr(), gdt, m.data_ptr<float>(),
               v.data_ptr<float>(),
               p_bf16_out.has_value() ? p_bf16_out->data_ptr() : nullptr, odt,
               n,
               (float)lr, (float)b1, (float)b2, (float)eps, (float)wd, bc1,
               bc2,
               grad_scale.has_value() ? grad_scale->data_ptr<float>() : nullptr,
               cur_stream());
}

void sq_norm_accum(Tensor t, Tensor out) {
  TORCH_CHECK(t.is_contiguous());
  const long long n = t.numel();
  TORCH_CHECK(n % 4 == 0);
  const int dt = t.scalar_type() == torch::kBFloat16 ? 1
                 : t.scalar_type() == torch::kFloat16 ? 2 : 0;
  launch_sqnorm(t.data_ptr(), dt, out.data_ptr<float>(), n, cur_stream());
}

// Get/set the causal-attention workgroup order ("balanced" | "legacy",
// attn_sched.h). Returns the mode in force before the call, so one
// process can A/B both orders.
std::string attn_sched_mode_py(c10::optional<std::string> mode) {
  int m = -1;
  if (mode.has_value()) {
    TORCH_CHECK(*mode == "balanced" || *mode == "legacy",
                "attn_sched_mode: expected 'balanced' or 'legacy', got '",
                *mode, "'");
    m = (*mode == "legacy") ? 1 : 0;
  }
  return attn_sched_mode(m) == 1 ? "legacy" : "balanced";
}

// Get/set the dk/dv kernel body of the attention backward ("keylane" |
// "legacy", attention.hip). Returns the mode in force before the call,
// so one process can A/B both bodies.
std::string attn_dkv_mode_py(c10::optional<std::string> mode) {
  int m = -1;
  if (mode.has_value()) {
    TORCH_CHECK(*mode == "keylane" || *mode == "legacy",
                "attn_dkv_mode: expected 'keylane' or 'legacy', got '", *mode,
                "'");
    m = (*mode == "legacy") ? 1 : 0;
  }
  return attn_dkv_mode(m) == 1 ? "legacy" : "keylane";
}

// Get/set the largest dS workspace attn_bwd may allocate, in bytes
// (attn_ws.h; 0 = always workspace-free). Returns the limit in force
// before the call.
int64_t attn_bwd_ws_limit_py(c10::optional<int64_t> bytes) {
  long long v = -1;
  if (bytes.has_value()) {
    TORCH_CHECK(*bytes >= 0, "attn_bwd_ws_limit: expected bytes >= 0, got ",
                *bytes);
    v = *bytes;
  }
  return attn_bwd_ws_limit(v);
}

std::tuple<Tensor, Tensor> attn_fwd(Tensor q, Tensor k, Tensor v) {
  CHECK_BF16_CONTIG(q);
  CHECK_BF16_CONTIG(k);
  const long long vs = row_stride4(v);  // strided (fused-qkv slice) ok
  const int b = q.size(0), s = q.size(1), h = q.size(2), d = q.size(3);
  const int kvh = k.size(2);
  TORCH_CHECK(d == 64 || d == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(s % 128 == 0, "seq len must be a multiple of 128");
  auto o = torch::empty_like(q);
  auto lse = torch::empty({b, h, s}, q.options().dtype(torch::kFloat32));
  const float scale = 1.f / sqrtf((float)d);
  launch_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  lse.data_ptr<float>(), b, s, h, kvh, d, scale, vs,
                  cur_stream());
  return {o, lse};
}

// ---- KV-cache decode (attn_decode.hip) --------------------------------
static bool aligned16(const Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// k/v cache pair: contiguous bf16 (b, capacity, kvh, d) on `dev`
static void check_kv_cache(const Tensor& kcache, const Tensor& vcache,
                           const torch::Device& dev) {
  TORCH_CHECK(kcache.scalar_type() == torch::kBFloat16 &&
                  vcache.scalar_type() == torch::kBFloat16,
              "the kv cache must be bf16");
  TORCH_CHECK(kcache.is_cuda() && vcache.is_cuda() &&
                  kcache.device() == dev && vcache.device() == dev,
              "the kv cache must live on q's GPU");
  TORCH_CHECK(kcache.dim() == 4 && kcache.sizes() == vcache.sizes(),
              "k and v cache must both be (b, capacity, kvh, d)");
  TORCH_CHECK(kcache.is_contiguous() && vcache.is_contiguous(),
              "the kv cache must be contiguous");
  TORCH_CHECK(aligned16(kcache) && aligned16(vcache),
              "the kv cache must be 16-byte aligned");
}

// Row stride of a (b, s, h, d) bf16 view with contiguous heads whose
// (b, s) rows sit at one uniform distance. Unlike row_stride4 this takes
// the stride from whichever of b and s has more than one entry: at s == 1
// (every decode step) a slice of the fused projection reports an arbitrary
// stride(1).
static long long append_row_stride(const Tensor& t) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, "expected bf16");
  TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1 && t.stride(2) == t.size(3),
              "expected a (b,s,h,d) view with contiguous heads");
  const int64_t hd = t.size(2) * t.size(3);
  int64_t rs = hd;
  if (t.size(1) > 1) {
    rs = t.stride(1);
    TORCH_CHECK(t.size(0) <= 1 || t.stride(0) == t.size(1) * rs,
                "expected a uniform (b, s) row stride");
  } else if (t.size(0) > 1) {
    rs = t.stride(0);
  }
  TORCH_CHECK(rs >= hd, "expected non-overlapping (b, s) rows");
  return rs;
}

// Rotate q and k by the (s, d/2) fp32 tables (rows = the positions being
// written), write rotated k and raw v into cache rows [pos, pos + s) and
// return contiguous rotated q: split + rope + append in one launch.
// Without tables only k and v are copied and q comes back as it is.
// q (b,s,h,d), k/v (b,s,kvh,d): row-strided bf16 views (fused-qkv slices).
Tensor kv_append(Tensor q, Tensor k, Tensor v, Tensor kcache, Tensor vcache,
                 int64_t pos, c10::optional<Tensor> cos,
                 c10::optional<Tensor> sin) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda() &&
                  k.device() == q.device() && v.device() == q.device(),
              "kv_append: q, k, v must be on one GPU");
  const long long qs = append_row_stride(q), ks = append_row_stride(k),
                  vs = append_row_stride(v);
  check_kv_cache(kcache, vcache, q.device());
  const int64_t b = q.size(0), s = q.size(1), h = q.size(2), d = q.size(3);
  const int64_t kvh = k.size(2), cap = kcache.size(1);
  TORCH_CHECK(k.size(0) == b && k.size(1) == s && k.size(3) == d &&
                  v.sizes() == k.sizes(),
              "kv_append: k and v must be (b, s, kvh, d) with q's b, s, d");
  TORCH_CHECK(kcache.size(0) == b && kcache.size(2) == kvh &&
                  kcache.size(3) == d,
              "kv_append: cache shape does not match k");
  TORCH_CHECK(d % 8 == 0, "kv_append: head_dim must be a multiple of 8");
  TORCH_CHECK(pos >= 0 && pos + s <= cap, "kv_append: rows [", pos, ", ",
              pos + s, ") do not fit the capacity ", cap);
  TORCH_CHECK(qs % 8 == 0 && ks % 8 == 0 && vs % 8 == 0,
              "kv_append: row strides must be multiples of 8 elements");
  TORCH_CHECK(aligned16(q) && aligned16(k) && aligned16(v),
              "kv_append: q, k, v must be 16-byte aligned");
  TORCH_CHECK(cos.has_value() == sin.has_value(),
              "kv_append: cos and sin come together");
  TORCH_CHECK(b * s * (h + 2 * kvh) * d / 8 < (1LL << 31) * 256,
              "kv_append: too many elements for one grid");
  const float *cp = nullptr, *sp = nullptr;
  if (cos.has_value()) {
    for (const Tensor* t : {&*cos, &*sin})
      TORCH_CHECK(t->scalar_type() == torch::kFloat32 && t->is_contiguous() &&
                      t->is_cuda() && t->device() == q.device() &&
                      t->dim() == 2 && t->size(0) == s &&
                      t->size(1) == d / 2 && aligned16(*t),
                  "kv_append: cos/sin must be contiguous fp32 (s, d/2) "
                  "tables with one row per appended position");
    cp = cos->data_ptr<float>();
    sp = sin->data_ptr<float>();
  }
  if (b == 0 || s == 0) return q;
  Tensor qo = cp ? torch::empty({b, s, h, d}, q.options()) : q;
  launch_kv_append(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                   cp ? qo.data_ptr() : nullptr, kcache.data_ptr(),
                   vcache.data_ptr(), cp, sp, (int)b, (int)s, (int)h,
                   (int)kvh, (int)d, qs, ks, vs, cap, pos, cur_stream());
  return qo;
}

// Split count attn_decode picks for (b, kvh, kv_len) on n_cu compute units.
int64_t attn_decode_plan_py(int64_t b, int64_t kvh, int64_t kv_len,
                            int64_t n_cu) {
  return attn_decode_plan(b, kvh, kv_len, n_cu);
}

// q (b, 1, h, d) against cache rows [0, kv_len): (o (b,1,h,d) bf16,
// lse (b, h) fp32, natural log). The newest key is already in the cache,
// so there is no causal mask. splits = 0 takes attn_decode_plan's count, a
// positive value forces it; either is clamped to the number of key tiles.
// splits > 1 allocates the fp32 partial workspace for this call.
std::tuple<Tensor, Tensor> attn_decode(Tensor q, Tensor kcache, Tensor vcache,
                                       int64_t kv_len, int64_t splits) {
  TORCH_CHECK(q.is_cuda(), "attn_decode: q must be on a GPU");
  CHECK_BF16_CONTIG(q);
  check_kv_cache(kcache, vcache, q.device());
  TORCH_CHECK(q.dim() == 4 && q.size(1) == 1,
              "attn_decode: q must be (b, 1, h, d)");
  const int64_t b = q.size(0), h = q.size(2), d = q.size(3);
  const int64_t cap = kcache.size(1), kvh = kcache.size(2);
  TORCH_CHECK(kcache.size(0) == b && kcache.size(3) == d,
              "attn_decode: cache shape does not match q");
  TORCH_CHECK(d == 64 || d == 128, "attn_decode: head_dim must be 64 or 128");
  TORCH_CHECK(kv_len >= 1 && kv_len <= cap, "attn_decode: kv_len ", kv_len,
              " outside [1, capacity ", cap, "]");
  TORCH_CHECK(kvh >= 1 && h % kvh == 0,
              "attn_decode: kvheads must divide nheads");
  TORCH_CHECK(h / kvh <= 64,
              "attn_decode: at most 64 query heads per kv head");
  TORCH_CHECK(aligned16(q), "attn_decode: q must be 16-byte aligned");
  TORCH_CHECK(splits >= 0, "attn_decode: splits must be >= 0");
  TORCH_CHECK(kv_len < (1LL << 31) - 64, "attn_decode: kv_len too large");
  auto o = torch::empty_like(q);
  auto f32 = q.options().dtype(torch::kFloat32);
  auto lse = torch::empty({b, h}, f32);
  if (b == 0) return {o, lse};
  if (splits == 0) {
    int n_cu = 0;
    TORCH_CHECK(hipDeviceGetAttribute(&n_cu,
                                      hipDeviceAttributeMultiprocessorCount,
                                      q.get_device()) == hipSuccess,
                "attn_decode: cannot query the compute unit count");
    splits = attn_decode_plan(b, kvh, kv_len, n_cu);
  }
  splits = attn_decode_clamp_splits(splits, kv_len);
  const int64_t ncb = (h / kvh + 31) / 32;
  TORCH_CHECK(b * kvh * ncb * splits < (1LL << 31),
              "attn_decode: too many workgroups for one grid");
  Tensor ws_o, ws_ml;
  if (splits > 1) {
    ws_o = torch::empty({b, h, splits, d}, f32);
    ws_ml = torch::empty({b, h, splits, 2}, f32);
  }
  launch_attn_decode(q.data_ptr(), kcache.data_ptr(), vcache.data_ptr(),
                     o.data_ptr(), lse.data_ptr<float>(),
                     splits > 1 ? ws_o.data_ptr<float>() : nullptr,
                     splits > 1 ? ws_ml.data_ptr<float>() : nullptr, (int)b,
                     (int)h, (int)kvh, (int)d, (int)kv_len, cap, (int)splits,
                     1.f / sqrtf((float)d), cur_stream());
  return {o, lse};
}

std::tuple<Tensor, Tensor, Tensor> attn_bwd(Tensor do_, Tensor q, Tensor k,
                                            Tensor v, Tensor o, Tensor lse,
                                            c10::optional<Tensor> dv_out) {
  CHECK_BF16_CONTIG(do_);
  const long long vs = row_stride4(v);
  const int b = q.size(0), s = q.size(1), h = q.size(2), d = q.size(3);
  const int kvh = k.size(2);
  auto dq = torch::empty_like(q);
  const bool out_bf16 = (kvh == h);  // no GQA collisions: direct bf16
  auto opts = q.options().dtype(out_bf16 ? torch::kBFloat16 : torch::kFloat32);
  auto dk = out_bf16 ? torch::empty({b, s, kvh, d}, opts)
                     : torch::zeros({b, s, kvh, d}, opts);
  // dv may land directly in a strided slice of a fused dqkv buffer
  // (bf16 path only — the GQA path accumulates in fp32 scratch)
  Tensor dv;
  long long dvs = (long long)kvh * d;
  if (dv_out.has_value() && out_bf16) {
    dv = *dv_out;
    dvs = row_stride4(dv);
  } else {
    dv = out_bf16 ? torch::empty({b, s, kvh, d}, opts)
                  : torch::zeros({b, s, kvh, d}, opts);
  }
  auto delta = torch::empty({b, h, s}, q.options().dtype(torch::kFloat32));
  // dS workspace (b, h, s, s) bf16: written by dkv, consumed by dq —
  // the backward's P/dP recompute runs once instead of twice. ~2.1 GB
  // at the 7B shape; the caching allocator reuses it across layers.
  // Quadratic in s, so above attn_bwd_ws_limit no workspace is allocated
  // and the launcher runs the O(s)-memory recompute path (null ds_ws).
  Tensor ds_ws;
  if (attn_bwd_use_workspace(b, h, s, attn_bwd_ws_limit(-1)))
    ds_ws = torch::empty({(long long)b * h, (long long)s, (long long)s},
                         q.options());
  const float scale = 1.f / sqrtf((float)d);
  launch_attn_bwd(do_.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                  o.data_ptr(), lse.data_ptr<float>(), dq.data_ptr(),
                  dk.data_ptr(), dv.data_ptr(), delta.data_ptr<float>(),
                  ds_ws.defined() ? ds_ws.data_ptr() : nullptr, b, s,
                  h, kvh, d, scale, out_bf16 ? 1 : 0, vs, dvs, cur_stream());
  if (out_bf16) return {dq, dk, dv};
  return {dq, dk.to(torch::kBFloat16), dv.to(torch::kBFloat16)};
}

// The backward's preprocess on its own: delta (b, h, s) fp32 =
// rowsum(dO * O) over head_dim, dO and O contiguous (b, s, h, d) bf16.
Tensor attn_bwd_delta(Tensor do_, Tensor o) {
  CHECK_BF16_CONTIG(do_);
  CHECK_BF16_CONTIG(o);
  TORCH_CHECK(do_.dim() == 4 && do_.sizes() == o.sizes(),
              "do and o must be (b, s, h, d) of one shape");
  const int b = o.size(0), s = o.size(1), h = o.size(2), d = o.size(3);
  TORCH_CHECK(d == 64 || d == 128, "head_dim must be 64 or 128");
  auto delta = torch::empty({b, h, s}, o.options().dtype(torch::kFloat32));
  launch_attn_bwd_delta(do_.data_ptr(), o.data_ptr(), delta.data_ptr<float>(),
                        b, s, h, d, cur_stream());
  return delta;
}

// (b, s) int32 document boundaries of the masked attention kernels
static void check_doc_array(const Tensor& t, const Tensor& q,
                            const char* name) {
  TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must be int32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == q.size(0) && t.size(1) == q.size(1),
              name, " must have shape (b, s)");
  TORCH_CHECK(t.device() == q.device(), name, " must be on q's device");
}

// Document-masked causal attention: query i sees key j iff
// doc_start[b, i] <= j <= i. Otherwise attn_fwd.
std::tuple<Tensor, Tensor> attn_fwd_doc(Tensor q, Tensor k, Tensor v,
                                        Tensor doc_start) {
  CHECK_BF16_CONTIG(q);
  CHECK_BF16_CONTIG(k);
  const long long vs = row_stride4(v);  // strided (fused-qkv slice) ok
  const int b = q.size(0), s = q.size(1), h = q.size(2), d = q.size(3);
  const int kvh = k.size(2);
  TORCH_CHECK(d == 64 || d == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(s % 128 == 0, "seq len must be a multiple of 128");
  check_doc_array(doc_start, q, "doc_start");
  auto o = torch::empty_like(q);
  auto lse = torch::empty({b, h, s}, q.options().dtype(torch::kFloat32));
  const float scale = 1.f / sqrtf((float)d);
  launch_attn_fwd_doc(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                      lse.data_ptr<float>(), doc_start.data_ptr<int>(), b, s,
                      h, kvh, d, scale, vs, cur_stream());
  return {o, lse};
}

// Backward of attn_fwd_doc. doc_end[b, j] = start of the document after
// j's (s for the last): the same mask seen from the key. Always the
// workspace-free kernels: no dS workspace is allocated at any limit.
std::tuple<Tensor, Tensor, Tensor> attn_bwd_doc(
    Tensor do_, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse,
    c10::optional<Tensor> dv_out, Tensor doc_start, Tensor doc_end) {
  CHECK_BF16_CONTIG(do_);
  const long long vs = row_stride4(v);
  const int b = q.size(0), s = q.size(1), h = q.size(2), d = q.size(3);
  const int kvh = k.size(2);
  check_doc_array(doc_start, q, "doc_start");
  check_doc_array(doc_end, q, "doc_end");
  auto dq = torch::empty_like(q);
  const bool out_bf16 = (kvh == h);  // no GQA collisions: direct bf16
  auto opts = q.options().dtype(out_bf16 ? torch::kBFloat16 : torch::kFloat32);
  auto dk = out_bf16 ? torch::empty({b, s, kvh, d}, opts)
                     : torch::zeros({b, s, kvh, d}, opts);
  Tensor dv;
  long long dvs = (long long)kvh * d;
  if (dv_out.has_value() && out_bf16) {
    dv = *dv_out;
    dvs = row_stride4(dv);
  } else {
    dv = out_bf16 ? torch::empty({b, s, kvh, d}, opts)
                  : torch::zeros({b, s, kvh, d}, opts);
  }
  auto delta = torch::empty({b, h, s}, q.options().dtype(torch::kFloat32));
  const float scale = 1.f / sqrtf((float)d);
  launch_attn_bwd_doc(do_.data_ptr(), q.data_ptr(), k.data_ptr(),
                      v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                      dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                      delta.data_ptr<float>(), doc_start.data_ptr<int>(),
                      doc_end.data_ptr<int>(), b, s, h, kvh, d, scale,
                      out_bf16 ? 1 : 0, vs, dvs, cur_stream());
  if (out_bf16) return {dq, dk, dv};
  return {dq, dk.to(torch::kBFloat16), dv.to(torch::kBFloat16)};
}

// Flat document array of the masked SSD / conv entry points (a DocMask's
// start or end, (b, l) int32): one element per token row of `like`, on
// its device. Returns the pointer, or nullptr when no mask was given.
// Runs with the other argument checks, before any launch.
static const int* doc_ptr(const c10::optional<Tensor>& t, long long rows,
                          const Tensor& like, const char* nm) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->scalar_type() == torch::kInt32, nm, " must be int32");
  TORCH_CHECK(t->is_contiguous(), nm, " must be contiguous");
  TORCH_CHECK(t->device() == like.device(), nm,
              " must be on the device of the activations");
  TORCH_CHECK(t->numel() == rows, nm, " must have b*l elements");
  return t->data_ptr<int>();
}

// chunks per row of the masked SSD kernels: l a multiple of Q, rows of l
static int doc_nc(long long rows, int64_t l, int64_t Q) {
  TORCH_CHECK(l > 0 && l % Q == 0 && rows % l == 0,
              "row length l must be a multiple of Q and divide the rows");
  TORCH_CHECK(l < (1LL << 31) && rows / Q < (1LL << 31),
              "masked SSD kernels index chunks and row positions in 32 bits");
  return (int)(l / Q);
}

static Tensor cconv_fwd_impl(Tensor x, Tensor w, Tensor bias,
                             c10::optional<Tensor> doc_start) {
  CHECK_BF16_CONTIG(x);
  CHECK_BF16_CONTIG(w);
  const int b = x.size(0), l = x.size(1), c = x.size(2);
  const int W = w.size(1);
  TORCH_CHECK(c % 8 == 0 && W >= 2 && W <= 4);
  TORCH_CHECK(bias.scalar_type() == torch::kFloat32);
  const int* ds = doc_ptr(doc_start, (long long)b * l, x, "doc_start");
  auto y = torch::empty_like(x);
  launch_cconv_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr<float>(),
                   y.data_ptr(), b * l, l, c, W, ds, cur_stream());
  return y;
}

Tensor cconv_fwd(Tensor x, Tensor w, Tensor bias) {
  return cconv_fwd_impl(x, w, bias, c10::nullopt);
}

// Document-masked conv: tap x[r] of output t counts iff r >= doc_start[t].
Tensor cconv_fwd_doc(Tensor x, Tensor w, Tensor bias, Tensor doc_start) {
  return cconv_fwd_impl(x, w, bias, doc_start);
}

static std::tuple<Tensor, Tensor, Tensor> cconv_bwd_impl(
    Tensor dy, Tensor x, Tensor w, Tensor bias,
    c10::optional<Tensor> doc_start, c10::optional<Tensor> doc_end) {
  CHECK_BF16_CONTIG(dy);
  CHECK_BF16_CONTIG(x);
  const int b = x.size(0), l = x.size(1), c = x.size(2);
  const int W = w.size(1);
  TORCH_CHECK(c % 8 == 0 && W >= 2 && W <= 4);
  const int* ds = doc_ptr(doc_start, (long long)b * l, x, "doc_start");
  const int* de = doc_ptr(doc_end, (long long)b * l, x, "doc_end");
  auto g = torch::empty_like(x);
  auto dx = torch::empty_like(x);
  auto dw = torch::zeros({c, W}, x.options().dtype(torch::kFloat32));
  auto db = torch::zeros({c}, x.options().dtype(torch::kFloat32));
  launch_cconv_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                   bias.data_ptr<float>(), g.data_ptr(), dx.data_ptr(),
                   dw.data_ptr<float>(), db.data_ptr<float>(), b * l, l, c, W,
                   ds, de, cur_stream());
  return {dx, dw, db};
}

std::tuple<Tensor, Tensor, Tensor> cconv_bwd(Tensor dy, Tensor x, Tensor w,
                                             Tensor bias) {
  return cconv_bwd_impl(dy, x, w, bias, c10::nullopt, c10::nullopt);
}

// Backward of cconv_fwd_doc; doc_end[t] = start of the document after t's.
std::tuple<Tensor, Tensor, Tensor> cconv_bwd_doc(Tensor dy, Tensor x,
                                                 Tensor w, Tensor bias,
                                                 Tensor doc_start,
                                                 Tensor doc_end) {
  return cconv_bwd_impl(dy, x, w, bias, doc_start, doc_end);
}

Tensor segsum_exp_fwd(Tensor cs) {
  TORCH_CHECK(cs.scalar_type() == torch::kFloat32 && cs.is_contiguous());
  const long long N = cs.numel() / cs.size(-1);
  const int Q = cs.size(-1);
  TORCH_CHECK(Q % 8 == 0);
  std::vector<int64_t> shape(cs.sizes().begin(), cs.sizes().end());
  shape.push_back(Q);
  auto out = torch::empty(shape, cs.options().dtype(torch::kBFloat16));
  launch_segsum_exp_fwd(cs.data_ptr<float>(), out.data_ptr(), N, Q,
                        cur_stream());
  return out;
}

Tensor segsum_exp_bwd(Tensor g, Tensor cs) {
  CHECK_BF16_CONTIG(g);
  const long long N = cs.numel() / cs.size(-1);
  const int Q = cs.size(-1);
  auto dcs = torch::empty_like(cs);
  launch_segsum_exp_bwd(g.data_ptr(), cs.data_ptr<float>(),
                        dcs.data_ptr<float>(), N, Q, cur_stream());
  return dcs;
}


Tensor gemm_nt(Tensor A, Tensor B) {
  CHECK_BF16_CONTIG(A);
  CHECK_BF16_CONTIG(B);
  const int M = A.size(0), K = A.size(1), N = B.size(1);
  TORCH_CHECK(B.size(0) == K);
  auto C = torch::empty({M, N}, A.options());
  const int rc = launch_gemm_nt(A.data_ptr(), B.data_ptr(), C.data_ptr(), M,
                                N, K, cur_stream());
  TORCH_CHECK(rc == 0, "gemm_nt: shape not supported (M%256/N%256/K%64)");
  return C;
}

// ---- fused SSD scan pieces (see ops/hip/ssd.hip) ----
// strided 2-D bf16 slice (rows, cols) with unit inner stride
static long long slice_stride(const Tensor& t, const char* nm) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, nm, " must be bf16");
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, nm, " must be 2-D row-major");
  return t.stride(0);
}

// fp32 contiguous (N, Q) per-(chunk, head) rows: dtf / dacs and their grads
static void check_nq(const Tensor& t, long long N, long long Q,
                     const char* nm) {
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, nm, " must be fp32");
  TORCH_CHECK(t.is_contiguous(), nm, " must be contiguous");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == N && t.size(1) == Q, nm,
              " must have shape (rows/Q*H, Q)");
}

// contiguous bf16 tensor of exactly `numel` elements
static void check_bf16_numel(const Tensor& t, long long numel,
                             const char* nm) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, nm, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), nm, " must be contiguous");
  TORCH_CHECK(t.numel() == numel, nm, " has the wrong element count");
}

// per-head fp32 parameter vector (dt_bias, A_log, D)
static void check_head_vec(const Tensor& t, long long H, const char* nm) {
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.is_contiguous() &&
                  t.numel() == H,
              nm, " must be contiguous fp32 with H elements");
}

// x / z slices of the fused projections: (rows, H*P) with rows % Q == 0
static long long check_xslice(const Tensor& t, int64_t H, int64_t P,
                              int64_t Q, const char* nm) {
  const long long st = slice_stride(t, nm);
  TORCH_CHECK(H > 0 && P > 0 && P % 8 == 0, "P must be divisible by 8");
  TORCH_CHECK(Q > 0 && Q % 8 == 0, "Q must be divisible by 8");
  TORCH_CHECK(t.size(1) == H * P, nm, " must have H*P columns");
  TORCH_CHECK(t.size(0) % Q == 0, nm, " rows must be a multiple of Q");
  return st;
}

static void check_prep_q(long long rows, int64_t Q) {
  TORCH_CHECK(Q > 0 && Q <= 256 && Q % 64 == 0 && rows % Q == 0,
              "Q must be 64, 128, 192 or 256 and divide the row count");
}

std::tuple<Tensor, Tensor> ssd_prep_fwd(Tensor dt, Tensor bias, Tensor alog,
                                        int64_t Q) {
  const long long sdt = slice_stride(dt, "dt");
  const long long rows = dt.size(0);
  const int H = dt.size(1);
  check_prep_q(rows, Q);
  check_head_vec(bias, H, "bias");
  check_head_vec(alog, H, "alog");
  const long long N = rows / Q * H;
  auto opt = dt.options().dtype(torch::kFloat32);
  auto dtf = torch::empty({N, Q}, opt);
  auto dacs = torch::empty({N, Q}, opt);
  launch_ssd_prep_fwd(dt.data_ptr(), bias.data_ptr<float>(),
                      alog.data_ptr<float>(), dtf.data_ptr<float>(),
                      dacs.data_ptr<float>(), N, H, (int)Q, sdt,
                      cur_stream());
  return {dtf, dacs};
}

std::tuple<Tensor, Tensor, Tensor> ssd_prep_bwd(Tensor ddtf, Tensor ddacs,
                                                Tensor dt, Tensor bias,
                                                Tensor alog, int64_t Q) {
  const long long sdt = slice_stride(dt, "dt");
  const long long rows = dt.size(0);
  const int H = dt.size(1);
  check_prep_q(rows, Q);
  check_head_vec(bias, H, "bias");
  check_head_vec(alog, H, "alog");
  const long long N = rows / Q * H;
  check_nq(ddtf, N, Q, "ddtf");
  check_nq(ddacs, N, Q, "ddacs");
  auto ddt = torch::empty({rows, (long long)H},
                          dt.options().dtype(torch::kBFloat16));
  auto dbias = torch::zeros({H}, dt.options().dtype(torch::kFloat32));
  auto dalog = torch::zeros({H}, dt.options().dtype(torch::kFloat32));
  launch_ssd_prep_bwd(ddtf.data_ptr<float>(), ddacs.data_ptr<float>(),
                      dt.data_ptr(), bias.data_ptr<float>(),
                      alog.data_ptr<float>(), ddt.data_ptr(),
                      dbias.data_ptr<float>(), dalog.data_ptr<float>(), N, H,
                      (int)Q, sdt, H, cur_stream());
  return {ddt, dbias, dalog};
}

// The masked (`_doc`) siblings of the xdt / sl / ygate entry points take
// the flat document starts and the row length l behind the unmasked
// arguments; see "Document mask" in docs/kernels.md for what each masks.
static std::tuple<Tensor, Tensor> ssd_xdt_fwd_impl(
    Tensor x, Tensor dtf, Tensor dacs, int64_t H, int64_t P, int64_t Q,
    c10::optional<Tensor> doc_start, int64_t l) {
  const long long sx = check_xslice(x, H, P, Q, "x");
  const long long rows = x.size(0);
  check_nq(dtf, rows / Q * H, Q, "dtf");
  check_nq(dacs, rows / Q * H, Q, "dacs");
  const int* ds = doc_ptr(doc_start, rows, x, "doc_start");
  const int nc = ds ? doc_nc(rows, l, Q) : 1;
  auto xdt = torch::empty({rows, H * P},
                          x.options().dtype(torch::kBFloat16));
  auto xdtd = torch::empty_like(xdt);
  const long long total8 = rows * H * P / 8;
  launch_ssd_xdt_fwd(x.data_ptr(), dtf.data_ptr<float>(),
                     dacs.data_ptr<float>(), xdt.data_ptr(), xdtd.data_ptr(),
                     total8, (int)H, (int)Q, (int)P, sx, ds, nc,
                     cur_stream());
  return {xdt, xdtd};
}

std::tuple<Tensor, Tensor> ssd_xdt_fwd(Tensor x, Tensor dtf, Tensor dacs,
                                       int64_t H, int64_t P, int64_t Q) {
  return ssd_xdt_fwd_impl(x, dtf, dacs, H, P, Q, c10::nullopt, 0);
}

std::tuple<Tensor, Tensor> ssd_xdt_fwd_doc(Tensor x, Tensor dtf, Tensor dacs,
                                           int64_t H, int64_t P, int64_t Q,
                                           Tensor doc_start, int64_t l) {
  return ssd_xdt_fwd_impl(x, dtf, dacs, H, P, Q, doc_start, l);
}

static std::tuple<Tensor, Tensor, Tensor> ssd_xdt_bwd_impl(
    Tensor dxdt, Tensor dxdtd, Tensor x, Tensor dtf, Tensor dacs, int64_t H,
    int64_t P, int64_t Q, c10::optional<Tensor> doc_start, int64_t l) {
  const long long sx = check_xslice(x, H, P, Q, "x");
  const long long rows = x.size(0);
  check_nq(dtf, rows / Q * H, Q, "dtf");
  check_nq(dacs, rows / Q * H, Q, "dacs");
  const int* ds = doc_ptr(doc_start, rows, x, "doc_start");
  const int nc = ds ? doc_nc(rows, l, Q) : 1;
  check_bf16_numel(dxdt, rows * H * P, "dxdt");
  check_bf16_numel(dxdtd, rows * H * P, "dxdtd");
  auto dx = torch::empty({rows, H * P}, x.options().dtype(torch::kBFloat16));
  auto ddtf = torch::empty_like(dtf);
  auto sdec = torch::empty_like(dacs);
  launch_ssd_xdt_bwd(dxdt.data_ptr(), dxdtd.data_ptr(), x.data_ptr(),
                     dtf.data_ptr<float>(), dacs.data_ptr<float>(),
                     dx.data_ptr(), ddtf.data_ptr<float>(),
                     sdec.data_ptr<float>(), rows * H, (int)H, (int)Q,
                     (int)P, sx, H * P, ds, nc, cur_stream());
  return {dx, ddtf, sdec};
}

std::tuple<Tensor, Tensor, Tensor> ssd_xdt_bwd(Tensor dxdt, Tensor dxdtd,
                                               Tensor x, Tensor dtf,
                                               Tensor dacs, int64_t H,
                                               int64_t P, int64_t Q) {
  return ssd_xdt_bwd_impl(dxdt, dxdtd, x, dtf, dacs, H, P, Q, c10::nullopt,
                          0);
}

std::tuple<Tensor, Tensor, Tensor> ssd_xdt_bwd_doc(
    Tensor dxdt, Tensor dxdtd, Tensor x, Tensor dtf, Tensor dacs, int64_t H,
    int64_t P, int64_t Q, Tensor doc_start, int64_t l) {
  return ssd_xdt_bwd_impl(dxdt, dxdtd, x, dtf, dacs, H, P, Q, doc_start, l);
}

// dacs (N, Q) fp32 and per-group scores (N/H*G, Q, Q) bf16; returns Q
static int check_sl(const Tensor& dacs, const Tensor& scores, int64_t H,
                    int64_t G) {
  TORCH_CHECK(H > 0 && G > 0 && H % G == 0, "H must be a multiple of G");
  TORCH_CHECK(dacs.dim() == 2, "dacs must be (N, Q)");
  const long long N = dacs.size(0), Q = dacs.size(1);
  TORCH_CHECK(Q > 0 && Q % 8 == 0, "Q must be divisible by 8");
  TORCH_CHECK(N % H == 0, "dacs rows must be a multiple of H");
  check_nq(dacs, N, Q, "dacs");
  TORCH_CHECK(scores.scalar_type() == torch::kBFloat16 &&
                  scores.is_contiguous(),
              "scores must be contiguous bf16");
  TORCH_CHECK(scores.dim() == 3 && scores.size(0) == N / H * G &&
                  scores.size(1) == Q && scores.size(2) == Q,
              "scores must have shape (N/H*G, Q, Q)");
  return (int)Q;
}

static Tensor ssd_sl_fwd_impl(Tensor dacs, Tensor scores, int64_t H,
                              int64_t G, c10::optional<Tensor> doc_start,
                              int64_t l) {
  const int Q = check_sl(dacs, scores, H, G);
  const long long N = dacs.size(0);
  const int* ds = doc_ptr(doc_start, N / H * Q, dacs, "doc_start");
  const int nc = ds ? doc_nc(N / H * Q, l, Q) : 1;
  auto out = torch::empty({N, (long long)Q, (long long)Q},
                          scores.options());
  launch_ssd_sl_fwd(dacs.data_ptr<float>(), scores.data_ptr(),
                    out.data_ptr(), N * Q * (Q / 8), (int)H, (int)G, Q, ds,
                    nc, cur_stream());
  return out;
}

Tensor ssd_sl_fwd(Tensor dacs, Tensor scores, int64_t H, int64_t G) {
  return ssd_sl_fwd_impl(dacs, scores, H, G, c10::nullopt, 0);
}

Tensor ssd_sl_fwd_doc(Tensor dacs, Tensor scores, int64_t H, int64_t G,
                      Tensor doc_start, int64_t l) {
  return ssd_sl_fwd_impl(dacs, scores, H, G, doc_start, l);
}

static std::tuple<Tensor, Tensor> ssd_sl_bwd_impl(
    Tensor g, Tensor scores, Tensor dacs, int64_t H, int64_t G,
    c10::optional<Tensor> doc_start, int64_t l) {
  const int Q = check_sl(dacs, scores, H, G);
  const long long N = dacs.size(0);
  check_bf16_numel(g, N * Q * Q, "g");
  const int* ds = doc_ptr(doc_start, N / H * Q, dacs, "doc_start");
  const int nc = ds ? doc_nc(N / H * Q, l, Q) : 1;
  auto dsh = torch::empty({N, (long long)Q, (long long)Q}, g.options());
  auto dcs = torch::zeros_like(dacs);
  launch_ssd_sl_bwd(g.data_ptr(), scores.data_ptr(), dacs.data_ptr<float>(),
                    dsh.data_ptr(), dcs.data_ptr<float>(), N, (int)H, (int)G,
                    Q, ds, nc, cur_stream());
  return {dsh, dcs};
}

std::tuple<Tensor, Tensor> ssd_sl_bwd(Tensor g, Tensor scores, Tensor dacs,
                                      int64_t H, int64_t G) {
  return ssd_sl_bwd_impl(g, scores, dacs, H, G, c10::nullopt, 0);
}

std::tuple<Tensor, Tensor> ssd_sl_bwd_doc(Tensor g, Tensor scores,
                                          Tensor dacs, int64_t H, int64_t G,
                                          Tensor doc_start, int64_t l) {
  return ssd_sl_bwd_impl(g, scores, dacs, H, G, doc_start, l);
}

static void check_ygate(const Tensor& ydiag, const Tensor& yoff,
                        const Tensor& dacs, const Tensor& x, const Tensor& Dp,
                        const Tensor& z, int64_t H, int64_t G, int64_t Q) {
  TORCH_CHECK(G > 0 && H % G == 0, "H must be a multiple of G");
  TORCH_CHECK(z.size(0) == x.size(0), "x and z must have the same rows");
  check_bf16_numel(ydiag, x.numel(), "ydiag");
  check_bf16_numel(yoff, x.numel(), "yoff");
  check_nq(dacs, x.size(0) / Q * H, Q, "dacs");
  check_head_vec(Dp, H, "D");
}

static Tensor ssd_ygate_fwd_impl(Tensor ydiag, Tensor yoff, Tensor dacs,
                                 Tensor x, Tensor Dp, Tensor z, int64_t H,
                                 int64_t G, int64_t P, int64_t Q,
                                 c10::optional<Tensor> doc_start, int64_t l) {
  const long long sx = check_xslice(x, H, P, Q, "x");
  const long long sz = check_xslice(z, H, P, Q, "z");
  const long long rows = x.size(0);
  check_ygate(ydiag, yoff, dacs, x, Dp, z, H, G, Q);
  const int* ds = doc_ptr(doc_start, rows, x, "doc_start");
  const int nc = ds ? doc_nc(rows, l, Q) : 1;
  auto out = torch::empty({rows, H * P}, x.options().dtype(torch::kBFloat16));
  launch_ssd_ygate_fwd(ydiag.data_ptr(), yoff.data_ptr(),
                       dacs.data_ptr<float>(), x.data_ptr(),
                       Dp.data_ptr<float>(), z.data_ptr(), out.data_ptr(),
                       rows * H * P / 8, (int)H, (int)G, (int)Q, (int)P, sx,
                       sz, ds, nc, cur_stream());
  return out;
}

Tensor ssd_ygate_fwd(Tensor ydiag, Tensor yoff, Tensor dacs, Tensor x,
                     Tensor Dp, Tensor z, int64_t H, int64_t G, int64_t P,
                     int64_t Q) {
  return ssd_ygate_fwd_impl(ydiag, yoff, dacs, x, Dp, z, H, G, P, Q,
                            c10::nullopt, 0);
}

Tensor ssd_ygate_fwd_doc(Tensor ydiag, Tensor yoff, Tensor dacs, Tensor x,
                         Tensor Dp, Tensor z, int64_t H, int64_t G,
                         int64_t P, int64_t Q, Tensor doc_start, int64_t l) {
  return ssd_ygate_fwd_impl(ydiag, yoff, dacs, x, Dp, z, H, G, P, Q,
                            doc_start, l);
}

static std::vector<Tensor> ssd_ygate_bwd_impl(
    Tensor dout, Tensor ydiag, Tensor yoff, Tensor dacs, Tensor x, Tensor Dp,
    Tensor z, int64_t H, int64_t G, int64_t P, int64_t Q,
    c10::optional<Tensor> doc_start, int64_t l) {
  const long long sx = check_xslice(x, H, P, Q, "x");
  const long long sz = check_xslice(z, H, P, Q, "z");
  const long long rows = x.size(0);
  check_ygate(ydiag, yoff, dacs, x, Dp, z, H, G, Q);
  check_bf16_numel(dout, rows * H * P, "dout");
  const int* ds = doc_ptr(doc_start, rows, x, "doc_start");
  const int nc = ds ? doc_nc(rows, l, Q) : 1;
  auto o = x.options().dtype(torch::kBFloat16);
  auto dydiag = torch::empty({rows, H * P}, o);
  auto dyoff = torch::empty({rows, H * P}, o);
  auto ddacs = torch::empty_like(dacs);
  auto dx = torch::empty({rows, H * P}, o);
  auto dD_rows = torch::empty({rows, H}, x.options().dtype(torch::kFloat32));
  auto dz = torch::empty({rows, H * P}, o);
  launch_ssd_ygate_bwd(dout.data_ptr(), ydiag.data_ptr(), yoff.data_ptr(),
                       dacs.data_ptr<float>(), x.data_ptr(),
                       Dp.data_ptr<float>(), z.data_ptr(), dydiag.data_ptr(),
                       dyoff.data_ptr(), ddacs.data_ptr<float>(),
                       dx.data_ptr(), dD_rows.data_ptr<float>(),
                       dz.data_ptr(), rows * H, (int)H, (int)G, (int)Q,
                       (int)P, sx, sz, H * P, H * P, ds, nc, cur_stream());
  return {dydiag, dyoff, ddacs, dx, dD_rows, dz};
}

std::vector<Tensor> ssd_ygate_bwd(Tensor dout, Tensor ydiag, Tensor yoff,
                                  Tensor dacs, Tensor x, Tensor Dp, Tensor z,
                                  int64_t H, int64_t G, int64_t P,
                                  int64_t Q) {
  return ssd_ygate_bwd_impl(dout, ydiag, yoff, dacs, x, Dp, z, H, G, P, Q,
                            c10::nullopt, 0);
}

std::vector<Tensor> ssd_ygate_bwd_doc(Tensor dout, Tensor ydiag, Tensor yoff,
                                      Tensor dacs, Tensor x, Tensor Dp,
                                      Tensor z, int64_t H, int64_t G,
                                      int64_t P, int64_t Q, Tensor doc_start,
                                      int64_t l) {
  return ssd_ygate_bwd_impl(dout, ydiag, yoff, dacs, x, Dp, z, H, G, P, Q,
                            doc_start, l);
}

// ---- Mamba2 recurrent decode (ssd_step.hip, causal_conv1d.hip) --------
// Row stride of a (b, T, cols) bf16 view the step kernels read in place: a
// last-dim slice of a projection. Unit last stride and one uniform
// distance between the (b, t) rows, taken from b at T == 1 (the rule of
// append_row_stride); 16-byte aligned base, stride a multiple of 8.
static long long step_row_stride(const Tensor& t, int64_t b, int64_t T,
                                 int64_t cols, const torch::Device& dev,
                                 const char* op, const char* nm) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, op, ": ", nm,
              " must be bf16");
  TORCH_CHECK(t.is_cuda() && t.device() == dev, op, ": ", nm,
              " must live on the state's GPU");
  TORCH_CHECK(t.dim() == 3 && t.size(0) == b && t.size(1) == T &&
                  t.size(2) == cols,
              op, ": ", nm, " must have shape (", b, ", ", T, ", ", cols, ")");
  TORCH_CHECK(t.stride(2) == 1, op, ": ", nm, " needs a unit last stride");
  int64_t rs = cols;
  if (T > 1) {
    rs = t.stride(1);
    TORCH_CHECK(b <= 1 || t.stride(0) == T * rs, op, ": ", nm,
                " needs one uniform (b, t) row stride");
  } else if (b > 1) {
    rs = t.stride(0);
  }
  TORCH_CHECK(rs >= cols, op, ": ", nm, " rows overlap");
  TORCH_CHECK(rs % 8 == 0, op, ": ", nm,
              " row stride must be a multiple of 8 elements");
  TORCH_CHECK(aligned16(t), op, ": ", nm, " must be 16-byte aligned");
  return rs;
}

static void check_step_vec(const Tensor& t, int64_t n,
                           const torch::Device& dev, const char* op,
                           const char* nm) {
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.is_contiguous() &&
                  t.dim() == 1 && t.numel() == n && t.is_cuda() &&
                  t.device() == dev,
              op, ": ", nm, " must be contiguous fp32 (", n,
              ") on the state's GPU");
}

// T >= 1 tokens of the SSD recurrence from `state` (b, H, P, N) fp32,
// updated in place; x/z (b, T, H*P), B/C (b, T, G*N), dt (b, T, H) bf16
// row-strided views; returns out (b, T, H*P) bf16.
Tensor ssd_step(Tensor state, Tensor x, Tensor dt, Tensor B, Tensor C,
                Tensor z, Tensor dt_bias, Tensor A_log, Tensor D, int64_t H,
                int64_t G, int64_t P, int64_t N) {
  const char* op = "ssd_step";
  TORCH_CHECK(state.is_cuda(), op, ": state must be on a GPU");
  TORCH_CHECK(state.scalar_type() == torch::kFloat32, op,
              ": state must be fp32");
  TORCH_CHECK(N == 16 || N == 32 || N == 64 || N == 128 || N == 256, op,
              ": d_state must be 16, 32, 64, 128 or 256, got ", N);
  TORCH_CHECK(P > 0 && P % 8 == 0, op,
              ": headdim must be a multiple of 8, got ", P);
  TORCH_CHECK(H > 0 && G > 0 && H % G == 0, op,
              ": nheads must be a multiple of ngroups, got ", H, " and ", G);
  TORCH_CHECK(state.dim() == 4 && state.size(1) == H && state.size(2) == P &&
                  state.size(3) == N,
              op, ": state must have shape (b, H, P, N)");
  TORCH_CHECK(state.is_contiguous(), op, ": state must be contiguous");
  TORCH_CHECK(aligned16(state), op, ": state must be 16-byte aligned");
  const int64_t b = state.size(0);
  TORCH_CHECK(x.dim() == 3 && x.size(1) >= 1, op,
              ": x must be (b, T, H*P) with T >= 1");
  const int64_t T = x.size(1);
  const auto dev = state.device();
  const long long sx = step_row_stride(x, b, T, H * P, dev, op, "x");
  const long long sz = step_row_stride(z, b, T, H * P, dev, op, "z");
  const long long sB = step_row_stride(B, b, T, G * N, dev, op, "B");
  const long long sC = step_row_stride(C, b, T, G * N, dev, op, "C");
  // dt rows are read one bf16 at a time: any stride and alignment do
  TORCH_CHECK(dt.scalar_type() == torch::kBFloat16 && dt.is_cuda() &&
                  dt.device() == dev && dt.dim() == 3 && dt.size(0) == b &&
                  dt.size(1) == T && dt.size(2) == H && dt.stride(2) == 1,
              op, ": dt must be a bf16 (b, T, H) view with a unit last "
              "stride on the state's GPU");
  long long sdt = H;
  if (T > 1) {
    sdt = dt.stride(1);
    TORCH_CHECK(b <= 1 || dt.stride(0) == T * sdt, op,
                ": dt needs one uniform (b, t) row stride");
  } else if (b > 1) {
    sdt = dt.stride(0);
  }
  TORCH_CHECK(sdt >= H, op, ": dt rows overlap");
  check_step_vec(dt_bias, H, dev, op, "dt_bias");
  check_step_vec(A_log, H, dev, op, "A_log");
  check_step_vec(D, H, dev, op, "D");
  TORCH_CHECK(T < (1LL << 31) && H * P < (1LL << 31) &&
                  G * N < (1LL << 31) &&
                  b * H * ((P + 15) / 16) < (1LL << 31),
              op, ": too many rows for one grid");
  auto out = torch::empty({b, T, H * P},
                          state.options().dtype(torch::kBFloat16));
  if (b == 0) return out;
  launch_ssd_step(state.data_ptr<float>(), x.data_ptr(), dt.data_ptr(),
                  B.data_ptr(), C.data_ptr(), z.data_ptr(),
                  dt_bias.data_ptr<float>(), A_log.data_ptr<float>(),
                  D.data_ptr<float>(), out.data_ptr(), b, (int)T, (int)H,
                  (int)G, (int)P, (int)N, sx, sdt, sB, sC, sz, cur_stream());
  return out;
}

// T >= 1 rows of the causal conv behind conv_state (b, W-1, C) bf16, which
// is updated in place; x (b, T, C) row-strided; returns y (b, T, C).
Tensor cconv_update(Tensor conv_state, Tensor x, Tensor w, Tensor bias) {
  const char* op = "cconv_update";
  TORCH_CHECK(conv_state.is_cuda(), op, ": conv_state must be on a GPU");
  TORCH_CHECK(conv_state.scalar_type() == torch::kBFloat16, op,
              ": conv_state must be bf16");
  TORCH_CHECK(conv_state.dim() == 3 && conv_state.is_contiguous(), op,
              ": conv_state must be contiguous (b, W-1, C)");
  TORCH_CHECK(aligned16(conv_state), op,
              ": conv_state must be 16-byte aligned");
  const auto dev = conv_state.device();
  const int64_t b = conv_state.size(0), c = conv_state.size(2);
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16 && w.is_contiguous() &&
                  w.dim() == 2 && w.size(0) == c && w.is_cuda() &&
                  w.device() == dev && aligned16(w),
              op, ": w must be contiguous bf16 (C, W) on the state's GPU");
  const int64_t W = w.size(1);
  TORCH_CHECK(W >= 2 && W <= 4, op, ": width must be 2, 3 or 4, got ", W);
  TORCH_CHECK(conv_state.size(1) == W - 1, op,
              ": conv_state must hold W-1 rows");
  TORCH_CHECK(c > 0 && c % 8 == 0, op,
              ": channels must be a multiple of 8, got ", c);
  TORCH_CHECK(x.dim() == 3 && x.size(1) >= 1, op,
              ": x must be (b, T, C) with T >= 1");
  const int64_t T = x.size(1);
  const long long sx = step_row_stride(x, b, T, c, dev, op, "x");
  check_step_vec(bias, c, dev, op, "bias");
  TORCH_CHECK(aligned16(bias), op, ": bias must be 16-byte aligned");
  TORCH_CHECK(T < (1LL << 31) && b * (c / 8) < (1LL << 31) * 256, op,
              ": too many elements for one grid");
  auto y = torch::empty({b, T, c}, conv_state.options());
  if (b == 0) return y;
  launch_cconv_update(conv_state.data_ptr(), x.data_ptr(), w.data_ptr(),
                      bias.data_ptr<float>(), y.data_ptr(), b, (int)T, (int)c,
                      (int)W, sx, cur_stream());
  return y;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("ssd_step", &ssd_step);
  mod.def("cconv_update", &cconv_update);
  mod.def("segsum_exp_fwd", &segsum_exp_fwd);
  mod.def("segsum_exp_bwd", &segsum_exp_bwd);
  mod.def("cconv_fwd", &cconv_fwd);
  mod.def("cconv_bwd", &cconv_bwd);
  mod.def("cconv_fwd_doc", &cconv_fwd_doc);
  mod.def("cconv_bwd_doc", &cconv_bwd_doc);
  mod.def("rmsnorm_fwd", &rmsnorm_fwd);
  mod.def("rmsnorm_bwd", &rmsnorm_bwd);
  mod.def("rmsnorm_bwd_into", &rmsnorm_bwd_into);
  mod.def("rmsnorm_bwd_grid", &rmsnorm_bwd_grid_py,
          pybind11::arg("grid") = pybind11::none());
  mod.def("add_rmsnorm_fwd", &add_rmsnorm_fwd);
  mod.def("rope_fwd", &rope_fwd);
  mod.def("rope_into", &rope_into);
  mod.def("swiglu_fwd", &swiglu_fwd);
  mod.def("swiglu_bwd", &swiglu_bwd);
  mod.def("transpose_bf16", &transpose_bf16, pybind11::arg("src"),
          pybind11::arg("out") = pybind11::none());
  mod.def("wgrad_tn", &wgrad_tn);
  mod.def("wgrad_tn_calls", &wgrad_tn_calls);
  mod.def("dgrad_tn", &dgrad_tn);
  mod.def("dgrad_tn_calls", &dgrad_tn_calls);
  mod.def("ce_fwd_bwd", &ce_fwd_bwd);
  mod.def("adamw", &adamw);
  mod.def("sq_norm_accum", &sq_norm_accum);
  mod.def("gemm_nt", &gemm_nt);
  mod.def("ssd_prep_fwd", &ssd_prep_fwd);
  mod.def("ssd_prep_bwd", &ssd_prep_bwd);
  mod.def("ssd_xdt_fwd", &ssd_xdt_fwd);
  mod.def("ssd_xdt_bwd", &ssd_xdt_bwd);
  mod.def("ssd_sl_fwd", &ssd_sl_fwd);
  mod.def("ssd_sl_bwd", &ssd_sl_bwd);
  mod.def("ssd_ygate_fwd", &ssd_ygate_fwd);
  mod.def("ssd_ygate_bwd", &ssd_ygate_bwd);
  mod.def("ssd_xdt_fwd_doc", &ssd_xdt_fwd_doc);
  mod.def("ssd_xdt_bwd_doc", &ssd_xdt_bwd_doc);
  mod.def("ssd_sl_fwd_doc", &ssd_sl_fwd_doc);
  mod.def("ssd_sl_bwd_doc", &ssd_sl_bwd_doc);
  mod.def("ssd_ygate_fwd_doc", &ssd_ygate_fwd_doc);
  mod.def("ssd_ygate_bwd_doc", &ssd_ygate_bwd_doc);
  mod.def("attn_fwd", &attn_fwd);
  mod.def("attn_bwd", &attn_bwd);
  mod.def("kv_append", &kv_append, pybind11::arg("q"), pybind11::arg("k"),
          pybind11::arg("v"), pybind11::arg("kcache"),
          pybind11::arg("vcache"), pybind11::arg("pos"),
          pybind11::arg("cos") = pybind11::none(),
          pybind11::arg("sin") = pybind11::none());
  mod.def("attn_decode", &attn_decode, pybind11::arg("q"),
          pybind11::arg("kcache"), pybind11::arg("vcache"),
          pybind11::arg("kv_len"), pybind11::arg("splits") = 0);
  mod.def("attn_decode_plan", &attn_decode_plan_py);
  mod.def("attn_bwd_delta", &attn_bwd_delta);
  mod.def("attn_fwd_doc", &attn_fwd_doc);
  mod.def("attn_bwd_doc", &attn_bwd_doc);
  mod.def("attn_sched_mode", &attn_sched_mode_py,
          pybind11::arg("mode") = pybind11::none());
  mod.def("attn_dkv_mode", &attn_dkv_mode_py,
          pybind11::arg("mode") = pybind11::none());
  mod.def("attn_bwd_ws_limit", &attn_bwd_ws_limit_py,
          pybind11::arg("bytes") = pybind11::none());
}
