// Torch bindings for the kubetorch_amd MI355X kernels (kernels.hip).
// Host-only translation unit; compiled by hipcc against torch-ROCm's
// native HIP API surface (c10/hip). No CUDA-compat shims.

#include <cmath>
#include <cstdlib>

#include <torch/extension.h>

// torch-ROCm registers GPU tensors under DeviceType::CUDA; its native HIP
// guard/stream accessors for that device type are the "masquerading" ones.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

extern "C" {
void kt_rmsnorm_fwd(const void* x, const void* res, const void* w, void* y,
                    void* s_out, void* invrms, int N, int H, float eps,
                    hipStream_t stream);
void kt_rmsnorm_bwd(const void* dy, const void* ds, const void* x,
                    const void* w, const void* invrms, void* dx,
                    void* dw_partial, void* dw, int P, int N, int H,
                    hipStream_t stream);
void kt_rope(const void* x, void* o, const void* cost, const void* sint,
             long total_quads, int S, int Hh, int D, long src_t_stride,
             long src_h_stride, float sign, float oscale, hipStream_t stream);
void kt_attn_grad_pack(const void* dq, const void* dk, const void* dv,
                       void* out, const void* cost, const void* sint, long B,
                       int S, int Hq, int Hkv, int D, const long* strides,
                       float oscale, hipStream_t stream);
void kt_swiglu_fwd(const void* gu, void* out, long N, int I,
                   hipStream_t stream);
void kt_swiglu_bwd(const void* dout, const void* gu, void* dgu, long N, int I,
                   hipStream_t stream);
void kt_cross_entropy_fwd(void* logits, const void* targets, void* loss,
                          int N, int V, float scale, long ignore_index,
                          hipStream_t stream);
void kt_scale_bf16(const void* in, void* out, const void* scale, long n,
                   hipStream_t stream);
void kt_adamw(void* p, const void* g, void* m, void* v, long n, float lr,
              float beta1, float beta2, float eps, float wd, float bc1,
              float bc2, float grad_scale, hipStream_t stream);
void kt_attn_fwd(const void* q, const void* k, const void* v, void* o,
                 void* lse, int B, int Hq, int Hkv, int S, float scale,
                 hipStream_t stream);
void kt_attn_fwd_ck(const void* q, const void* k, const void* v, void* o,
                    void* lse, int B, int Hq, int Hkv, int S, float scale,
                    const long* strides, hipStream_t stream);
void kt_attn_fwd_ck_tr(const void* q, const void* k, const void* v, void* o,
                       void* lse, int B, int Hq, int Hkv, int S, float scale,
                       const long* strides, hipStream_t stream);
void kt_attn_fwd_v3(const void* q, const void* k, const void* v, void* o,
                    void* lse, int B, int Hq, int Hkv, int S, float scale,
                    const long* strides, hipStream_t stream);
void kt_pack_segments(const void* ptrs, const void* nbytes, const void* offs,
                      void* base, int nseg, long max_nbytes, int to_base,
                      hipStream_t stream);
void kt_transpose_bf16(const void* src, long src_stride, void* dst, long R,
                       long C, hipStream_t stream);
void kt_transpose_segments_bf16(const void* src, void* dst, const void* table,
                                int nseg, long max_tiles, hipStream_t stream);
void kt_attn_bwd_ck(const void* q, const void* k, const void* v,
                    const void* o, const void* do_, const void* lse, void* d,
                    void* dq_acc, void* dq, void* dk, void* dv, int B, int Hq,
                    int Hkv, int S, float scale, int mask_mode, int pipe,
                    hipStream_t stream);
void kt_paged_kv_write(const void* k_new, const void* v_new, void* k_pages,
                       void* v_pages, const void* slot_mapping, long T,
                       int Hkv, int hd, int page_size, long num_pages,
                       long k_st, long k_sh, long v_st, long v_sh,
                       hipStream_t stream);
void kt_paged_kv_write_fp8(const void* k_new, const void* v_new,
                           void* k_pages, void* v_pages,
                           const void* slot_mapping, const void* k_inv,
                           const void* v_inv, long T, int Hkv, int hd,
                           int page_size, long num_pages, long k_st,
                           long k_sh, long v_st, long v_sh,
                           hipStream_t stream);
int kt_paged_attention_decode(const void* q, const void* k_pages,
                              const void* v_pages, const void* block_table,
                              const void* seq_lens, void* out, void* po,
                              void* pm, void* pl, int B, int Hq, int Hkv,
                              int hd, int page_size, int num_pages,
                              int max_blocks, int num_splits, float scale,
                              int fp8, const void* k_scale,
                              const void* v_scale, hipStream_t stream);
int kt_paged_attention_prefill(const void* q, const void* k_pages,
                               const void* v_pages, const void* block_table,
                               const void* cu_q_lens, const void* seq_lens,
                               void* out, long T, long q_st, long q_sh, int B,
                               int Hq, int Hkv, int hd, int page_size,
                               int num_pages, int max_blocks, int max_q_len,
                               float scale, int fp8, const void* k_scale,
                               const void* v_scale, hipStream_t stream);
void kt_sample_tokens(const void* logits, long row_stride, int B, int V,
                      const void* temperature, const void* top_k,
                      const void* top_p, const void* seed, const void* offset,
                      void* out, hipStream_t stream);
void kt_token_logprobs(const void* logits, long row_stride, int B, int V,
                       const void* token, const void* temperature, int top_n,
                       void* logprob, void* rank, void* top_ids,
                       void* top_logprobs, hipStream_t stream);
int kt_linear_w8_plan(long N, long K);
void kt_linear_w8(const void* x, long x_stride, const void* wq,
                  const void* scale, void* y, void* part, int M, int N, int K,
                  int S, hipStream_t stream);
}

namespace {

#define CHECK_BF16_CONTIG(t)                                         \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");                  \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16"); \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

hipStream_t cur_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

std::vector<at::Tensor> rmsnorm_fwd(const at::Tensor& x,
                                    const std::optional<at::Tensor>& res,
                                    const at::Tensor& w, double eps) {
  CHECK_BF16_CONTIG(x);
  CHECK_BF16_CONTIG(w);
  const int H = (int)x.size(-1);
  const long N = x.numel() / H;
  TORCH_CHECK(H % 8 == 0, "H must be a multiple of 8");
  TORCH_CHECK(w.numel() == H, "weight shape mismatch");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty_like(x);
  auto invrms = at::empty({N}, x.options().dtype(at::kFloat));
  at::Tensor s;
  const void* res_ptr = nullptr;
  void* s_ptr = nullptr;
  if (res.has_value()) {
    CHECK_BF16_CONTIG(res.value());
    TORCH_CHECK(res->sizes() == x.sizes(), "residual shape mismatch");
    s = at::empty_like(x);
    res_ptr = res->data_ptr();
    s_ptr = s.data_ptr();
  }
  kt_rmsnorm_fwd(x.data_ptr(), res_ptr, w.data_ptr(), y.data_ptr(), s_ptr,
                 invrms.data_ptr(), (int)N, H, (float)eps, cur_stream(x));
  if (res.has_value()) return {y, invrms, s};
  return {y, invrms};
}

std::vector<at::Tensor> rmsnorm_bwd(const at::Tensor& dy,
                                    const std::optional<at::Tensor>& ds,
                                    const at::Tensor& x, const at::Tensor& w,
                                    const at::Tensor& invrms) {
  CHECK_BF16_CONTIG(dy);
  CHECK_BF16_CONTIG(x);
  CHECK_BF16_CONTIG(w);
  const int H = (int)x.size(-1);
  const long N = x.numel() / H;
  TORCH_CHECK(H % 8 == 0, "H must be a multiple of 8");
  TORCH_CHECK(w.numel() == H, "weight shape mismatch");
  TORCH_CHECK(dy.sizes() == x.sizes(), "dy shape mismatch");
  TORCH_CHECK(invrms.is_cuda() && invrms.scalar_type() == at::kFloat &&
                  invrms.is_contiguous() && invrms.numel() == N,
              "invrms must be N contiguous fp32 values on GPU");
  // The kernel keeps its dw accumulator in H*4 bytes of dynamic LDS next to
  // the 64 B static scratch of block_reduce_sum. The limit is read from the
  // runtime (hipDeviceAttributeMaxSharedMemoryPerBlock of x's device),
  // the bound the HIP runtime holds a launch's static + dynamic LDS to,
  // rather than assumed from the size of a CU's LDS.
  int lds_max = 0;
  TORCH_CHECK(hipDeviceGetAttribute(&lds_max,
                                    hipDeviceAttributeMaxSharedMemoryPerBlock,
                                    x.device().index()) == hipSuccess,
              "cannot read the LDS limit");
  TORCH_CHECK((size_t)H * sizeof(float) + 64 <= (size_t)lds_max,
              "H too large for the rmsnorm_bwd LDS accumulator");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto dx = at::empty_like(x);
  auto dw = at::empty_like(w);
  const int P = N < 512 ? (int)N : 512;
  auto dw_partial = at::empty({P, H}, x.options().dtype(at::kFloat));
  const void* ds_ptr = nullptr;
  if (ds.has_value()) {
    CHECK_BF16_CONTIG(ds.value());
    TORCH_CHECK(ds->sizes() == x.sizes(), "ds shape mismatch");
    ds_ptr = ds->data_ptr();
  }
  kt_rmsnorm_bwd(dy.data_ptr(), ds_ptr, x.data_ptr(), w.data_ptr(),
                 invrms.data_ptr(), dx.data_ptr(), dw_partial.data_ptr(),
                 dw.data_ptr(), P, (int)N, H, cur_stream(x));
  return {dx, dw};
}

at::Tensor rope(const at::Tensor& x, const at::Tensor& cost,
                const at::Tensor& sint, int64_t S, double sign,
                double oscale) {
  // x: [T, Hh, D] with T = B*S (strided views OK if the head dim is
  // contiguous — e.g. qkv-split slices / transposed grads); output packed.
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  TORCH_CHECK(x.dim() == 3, "rope expects [T, Hh, D]");
  TORCH_CHECK(x.stride(2) == 1, "head dim must be contiguous");
  TORCH_CHECK(cost.scalar_type() == at::kFloat && cost.is_contiguous());
  const int D = (int)x.size(2);
  const int Hh = (int)x.size(1);
  TORCH_CHECK(D % 8 == 0, "head dim must be a multiple of 8");
  TORCH_CHECK(cost.size(0) >= S && cost.size(1) == D / 2, "cos table shape");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto o = at::empty(x.sizes(), x.options());
  const long total_quads = (long)x.size(0) * Hh * (D / 8);
  kt_rope(x.data_ptr(), o.data_ptr(), cost.data_ptr(), sint.data_ptr(),
          total_quads, (int)S, Hh, D, x.stride(0), x.stride(1), (float)sign,
          (float)oscale, cur_stream(x));
  return o;
}

at::Tensor attn_grad_pack(const at::Tensor& dq, const at::Tensor& dk_e,
                          const at::Tensor& dv_e, const at::Tensor& cost,
                          const at::Tensor& sint, int64_t n_kv,
                          double q_oscale) {
  // dq, dk_e, dv_e: [B, Hq, S, D] in any layout with a contiguous head dim
  // ([B,H,S,D] buffers and transposed [B,S,H,D] buffers both go in as they
  // are). Returns the packed [B, S, (Hq + 2*n_kv)*D] gradient of the qkv
  // GEMM output. Every check is made before the launch.
  TORCH_CHECK(dq.dim() == 4, "dq must be [B, Hq, S, D]");
  TORCH_CHECK(dk_e.sizes() == dq.sizes() && dv_e.sizes() == dq.sizes(),
              "dq, dk_e and dv_e must have the same shape");
  const int64_t B = dq.size(0), Hq = dq.size(1), S = dq.size(2),
                D = dq.size(3);
  TORCH_CHECK(D > 0 && D % 8 == 0, "head dim must be a multiple of 8");
  TORCH_CHECK(n_kv >= 1 && Hq % n_kv == 0, "Hq must be a multiple of n_kv");
  long strides[9];
  int si = 0;
  for (const at::Tensor* t : {&dq, &dk_e, &dv_e}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16,
                "gradients must be bf16 GPU tensors");
    TORCH_CHECK(t->device() == dq.device(), "gradients on different devices");
    TORCH_CHECK(t->stride(3) == 1, "head dim must be contiguous");
    for (int d = 0; d < 3; ++d) {
      // a dim of size 1 is only ever indexed at 0: its stride is free
      TORCH_CHECK(t->size(d) == 1 ||
                      (t->stride(d) >= 0 && t->stride(d) % 8 == 0),
                  "strides must be non-negative multiples of 8 elements");
      strides[si++] = t->size(d) == 1 ? 0 : t->stride(d);
    }
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "gradients must be 16 B aligned");
  }
  for (const at::Tensor* t : {&cost, &sint}) {
    TORCH_CHECK(t->is_cuda() && t->device() == dq.device() &&
                    t->scalar_type() == at::kFloat && t->is_contiguous() &&
                    t->dim() == 2,
                "cos/sin must be contiguous fp32 [>=S, D/2] GPU tables");
    TORCH_CHECK(t->size(0) >= S && t->size(1) == D / 2, "cos/sin table shape");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "cos/sin must be 16 B aligned");
  }
  // the kernel keeps the position and the offset inside a token's row in int
  TORCH_CHECK(S < (int64_t(1) << 31) &&
                  (Hq + 2 * n_kv) * D < (int64_t(1) << 31),
              "shape out of range");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dq.device());
  auto out = at::empty({B, S, (Hq + 2 * n_kv) * D}, dq.options());
  if (out.numel() == 0) return out;
  kt_attn_grad_pack(dq.data_ptr(), dk_e.data_ptr(), dv_e.data_ptr(),
                    out.data_ptr(), cost.data_ptr(), sint.data_ptr(), (long)B,
                    (int)S, (int)Hq, (int)n_kv, (int)D, strides,
                    (float)q_oscale, cur_stream(dq));
  return out;
}

at::Tensor swiglu_fwd(const at::Tensor& gu) {
  CHECK_BF16_CONTIG(gu);
  const int twoI = (int)gu.size(-1);
  TORCH_CHECK(twoI % 16 == 0, "2*I must be a multiple of 16");
  const int I = twoI / 2;
  const long N = gu.numel() / twoI;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(gu.device());
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto out = at::empty(sizes, gu.options());
  kt_swiglu_fwd(gu.data_ptr(), out.data_ptr(), N, I, cur_stream(gu));
  return out;
}

at::Tensor swiglu_bwd(const at::Tensor& dout, const at::Tensor& gu) {
  CHECK_BF16_CONTIG(dout);
  CHECK_BF16_CONTIG(gu);
  const int twoI = (int)gu.size(-1);
  TORCH_CHECK(twoI % 16 == 0, "2*I must be a multiple of 16");
  const int I = twoI / 2;
  const long N = gu.numel() / twoI;
  TORCH_CHECK(dout.size(-1) == I && dout.numel() == N * I,
              "dout shape mismatch");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(gu.device());
  auto dgu = at::empty_like(gu);
  kt_swiglu_bwd(dout.data_ptr(), gu.data_ptr(), dgu.data_ptr(), N, I,
                cur_stream(gu));
  return dgu;
}

at::Tensor cross_entropy_fwd_(at::Tensor logits, const at::Tensor& targets,
                              double scale, int64_t ignore_index) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(targets.scalar_type() == at::kLong && targets.is_contiguous());
  const int V = (int)logits.size(-1);
  const long N = logits.numel() / V;
  TORCH_CHECK(V % 8 == 0, "V must be a multiple of 8");
  TORCH_CHECK(targets.numel() == N, "targets shape mismatch");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  auto loss = at::empty({N}, logits.options().dtype(at::kFloat));
  kt_cross_entropy_fwd(logits.data_ptr(), targets.data_ptr(), loss.data_ptr(),
                       (int)N, V, (float)scale, ignore_index,
                       cur_stream(logits));
  return loss;
}

at::Tensor scale_bf16(const at::Tensor& x, const at::Tensor& scale) {
  // bf16(x * scale) with the fp32 scale read from device memory (no sync,
  // no rounding of the factor to bf16).
  CHECK_BF16_CONTIG(x);
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat &&
                  scale.numel() == 1 && scale.device() == x.device(),
              "scale must be one fp32 value on x's device");
  TORCH_CHECK(x.numel() % 8 == 0, "numel must be a multiple of 8");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto out = at::empty_like(x);
  if (x.numel() > 0)
    kt_scale_bf16(x.data_ptr(), out.data_ptr(), scale.data_ptr(), x.numel(),
                  cur_stream(x));
  return out;
}

void adamw_(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v,
            double lr, double beta1, double beta2, double eps, double wd,
            int64_t step, double grad_scale) {
  CHECK_BF16_CONTIG(p);
  CHECK_BF16_CONTIG(g);
  TORCH_CHECK(m.scalar_type() == at::kFloat && v.scalar_type() == at::kFloat);
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() &&
              p.numel() == v.numel());
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  const float bc1 = 1.f - powf((float)beta1, (float)step);
  const float bc2 = 1.f - powf((float)beta2, (float)step);
  kt_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
           (float)lr, (float)beta1, (float)beta2, (float)eps, (float)wd, bc1,
           bc2, (float)grad_scale, cur_stream(p));
}

// Host checks shared by the dense attention bindings. The kernels trust
// their arguments, so every check runs before the first allocation and
// launch: a call that fails here has written nothing.
void check_attn_tensor(const char* fn, const char* name, const at::Tensor& t,
                       const at::Tensor& q) {
  TORCH_CHECK(t.is_cuda(), fn, ": ", name, " must be on GPU");
  TORCH_CHECK(t.device() == q.device(), fn, ": ", name,
              " must be on the same device as q");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, fn, ": ", name,
              " must be bf16");
  TORCH_CHECK(t.dim() == 4 && t.size(3) == 128, fn, ": ", name,
              " must be [B,H,S,128]");
  TORCH_CHECK(t.stride(3) == 1, fn, ": ", name,
              " last dim must be contiguous");
}

struct AttnDims {
  int B, Hq, Hkv, S;
};

// q [B,Hq,S,128], k/v [B,Hkv,S,128]; S must be a multiple of `s_tile`
// (the kernel's query tile: no padded instantiation is validated).
AttnDims check_attn_qkv(const char* fn, const at::Tensor& q,
                        const at::Tensor& k, const at::Tensor& v,
                        int s_tile) {
  check_attn_tensor(fn, "q", q, q);
  check_attn_tensor(fn, "k", k, q);
  check_attn_tensor(fn, "v", v, q);
  TORCH_CHECK(k.sizes() == v.sizes(), fn, ": k and v shapes differ");
  TORCH_CHECK(q.size(0) >= 1 && q.size(1) >= 1 && q.size(2) >= 1, fn,
              ": B, Hq and S must be >= 1");
  TORCH_CHECK(k.size(0) == q.size(0), fn, ": k batch ", k.size(0),
              " != q batch ", q.size(0));
  TORCH_CHECK(k.size(2) == q.size(2), fn, ": k sequence length ", k.size(2),
              " != q sequence length ", q.size(2));
  TORCH_CHECK(k.size(1) >= 1 && q.size(1) % k.size(1) == 0, fn,
              ": GQA requires Hkv >= 1 and Hq % Hkv == 0");
  TORCH_CHECK(q.size(2) % s_tile == 0, fn, ": S must be a multiple of ",
              s_tile, ", got ", q.size(2));
  return {(int)q.size(0), (int)q.size(1), (int)k.size(1), (int)q.size(2)};
}

// The CK kernels take element strides as 32-bit ck_tile::index_t. This
// bounds each stride on its own and nothing more: not the products the
// kernels form inside a tile window (stride(2) * (S - 1)), not the
// launcher's own (index_t)Hq * S for the lse batch stride, and not overlap:
// a q expanded over batch or heads (stride 0) passes, and o, allocated with
// q's strides, then aliases itself.
void check_attn_strides(const char* fn, const char* name,
                        const at::Tensor& t) {
  for (int d = 0; d < 3; ++d)
    TORCH_CHECK(t.stride(d) >= 0 && t.stride(d) < (1LL << 31), fn, ": ", name,
                " stride(", d, ") = ", t.stride(d),
                " does not fit the kernel's 32-bit index");
}

std::vector<at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k,
                                 const at::Tensor& v, double scale) {
  // q: [B, Hq, S, 128]; k/v: [B, Hkv, S, 128]; causal, bf16.
  const auto [B, Hq, Hkv, S] = check_attn_qkv("attn_fwd", q, k, v, 128);
  TORCH_CHECK(S >= 256, "attn_fwd: S must be a multiple of 128, >= 256");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous(),
              "attn_fwd: q, k and v must be contiguous");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  auto o = at::empty_like(q);
  auto lse = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  kt_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
              lse.data_ptr(), B, Hq, Hkv, S, (float)scale, cur_stream(q));
  return {o, lse};
}

std::vector<at::Tensor> attn_fwd_ck_impl(const at::Tensor& q,
                                         const at::Tensor& k,
                                         const at::Tensor& v, double scale,
                                         bool trload) {
  // CK-tile FMHA fwd: q [B,Hq,S,128], k/v [B,Hkv,S,128], causal, LSE out.
  // Strided inputs are supported (last dim must be contiguous) — [B,S,H,D]
  // permuted views go straight in, no transpose copies.
  // S % 128: the kernels' M0 tile; the padded tail path is not validated.
  const char* name = trload ? "attn_fwd_ck_tr" : "attn_fwd_ck";
  const auto [B, Hq, Hkv, S] = check_attn_qkv(name, q, k, v, 128);
  check_attn_strides(name, "q", q);  // o takes q's strides
  check_attn_strides(name, "k", k);
  check_attn_strides(name, "v", v);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  // write O in the same (possibly permuted) layout as q
  auto o = at::empty_strided(q.sizes(), q.strides(), q.options());
  auto lse = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  const long strides[12] = {
      q.stride(2), q.stride(1), q.stride(0),
      k.stride(2), k.stride(1), k.stride(0),
      v.stride(2), v.stride(1), v.stride(0),
      o.stride(2), o.stride(1), o.stride(0),
  };
  auto fn = trload ? kt_attn_fwd_ck_tr : kt_attn_fwd_ck;  // see also v3
  fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
     lse.data_ptr(), B, Hq, Hkv, S, (float)scale, strides, cur_stream(q));
  return {o, lse};
}

std::vector<at::Tensor> attn_fwd_ck(const at::Tensor& q, const at::Tensor& k,
                                    const at::Tensor& v, double scale) {
  return attn_fwd_ck_impl(q, k, v, scale, false);
}

std::vector<at::Tensor> attn_fwd_ck_tr(const at::Tensor& q,
                                       const at::Tensor& k,
                                       const at::Tensor& v, double scale) {
  return attn_fwd_ck_impl(q, k, v, scale, true);
}

std::vector<at::Tensor> attn_fwd_v3(const at::Tensor& q, const at::Tensor& k,
                                    const at::Tensor& v, double scale,
                                    bool prescaled) {
  // AITER-schedule v3 kernel (8 warps, M0=256) with LSE output.
  // S % 256: its M0 tile.
  const auto [B, Hq, Hkv, S] = check_attn_qkv("attn_fwd_v3", q, k, v, 256);
  check_attn_strides("attn_fwd_v3", "q", q);  // o takes q's strides
  check_attn_strides("attn_fwd_v3", "k", k);
  check_attn_strides("attn_fwd_v3", "v", v);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  // LSE-correct scaling contract: the v3 pipeline tracks the rowmax `m` of
  // the RAW gemm0 scores and its LSE epilogue computes m/log2e + log(l),
  // which is only the natural-log LSE when the gemm0 scores are already in
  // the scaled log2 domain. So Q must carry (scale * log2e) and the kernel
  // gets scale_s = ln2 (MakeKargs multiplies by log2e -> effective in-kernel
  // scale 1.0). O is mathematically unchanged; LSE becomes exact.
  // prescaled=true: the caller already folded scale*log2e into Q (free via
  // the RoPE kernel's oscale) -- skip the extra elementwise pass here.
  auto qs = prescaled ? q : q.mul(scale * 1.4426950408889634);
  auto o = at::empty_strided(q.sizes(), q.strides(), q.options());
  auto lse = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  const long strides[12] = {
      qs.stride(2), qs.stride(1), qs.stride(0),
      k.stride(2), k.stride(1), k.stride(0),
      v.stride(2), v.stride(1), v.stride(0),
      o.stride(2), o.stride(1), o.stride(0),
  };
  kt_attn_fwd_v3(qs.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                 lse.data_ptr(), B, Hq, Hkv, S, (float)0.6931471805599453,
                 strides, cur_stream(q));
  return {o, lse};
}

std::vector<at::Tensor> attn_bwd_ck(const at::Tensor& grad_out,
                                    const at::Tensor& q, const at::Tensor& k,
                                    const at::Tensor& v, const at::Tensor& o,
                                    const at::Tensor& lse, double scale) {
  // CK-tile GQA-native FMHA backward (attention_ck_bwd.hip). Contiguous
  // [B,H,S,128] bf16 in; returns (dq, dk, dv) with dk/dv Hq-EXPANDED — the
  // autograd wrapper sums KV-head groups.
  // S % 128: the N0 key block of pipes 0-2 and a multiple of every tile.
  const auto [B, Hq, Hkv, S] = check_attn_qkv("attn_bwd_ck", q, k, v, 128);
  check_attn_tensor("attn_bwd_ck", "grad_out", grad_out, q);
  check_attn_tensor("attn_bwd_ck", "o", o, q);
  TORCH_CHECK(grad_out.sizes() == q.sizes() && o.sizes() == q.sizes(),
              "attn_bwd_ck: grad_out and o must have q's shape");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous() &&
                  o.is_contiguous() && lse.is_contiguous(),
              "attn_bwd_ck: q, k, v, o and lse must be contiguous");
  // the launcher holds per-batch element strides in ck_tile::index_t
  TORCH_CHECK((int64_t)Hq * S * 128 < (1LL << 31),
              "attn_bwd_ck: Hq*S*128 does not fit the kernel's 32-bit index");
  TORCH_CHECK(lse.is_cuda() && lse.device() == q.device() &&
                  lse.sizes() == at::IntArrayRef({B, Hq, S}) &&
                  lse.scalar_type() == at::kFloat,
              "attn_bwd_ck: lse must be fp32 [B,Hq,S] on q's device");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  auto go = grad_out.contiguous();
  auto dq = at::empty_like(q);
  auto dk = at::empty({B, Hq, S, 128}, k.options());
  auto dv = at::empty({B, Hq, S, 128}, v.options());
  auto d = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  // dq is accumulated atomically across key blocks -> fp32, zero-init
  auto dq_acc = at::zeros({B, Hq, S, 128}, q.options().dtype(at::kFloat));
  // KT_CKBWD_MASK selects the causal-mask convention at runtime (the
  // round-2 root cause turned out to be contraction depth, not the mask;
  // the knob stays for window-attention experiments): 0=top-left (fwd
  // convention), 1=bottom-right, 2=swapped lr window. KT_CKBWD_PIPE selects the
  // pipeline: 0=std (KRKTRVR IGLP, 32x32x16 warp tiles), 1=trload
  // (gfx950 transposed-fragment loads, 16x16x32), 2=trload M0=64,
  // 3=trload N0=64. All four pass the float64 rules of
  // tests/test_attention_dense.py on gfx950; 3 has no timing on record.
  int mask_mode = 0;
  if (const char* mm = std::getenv("KT_CKBWD_MASK")) mask_mode = atoi(mm);
  // default pipe 1 (gfx950 trload, 311 TF measured) — fastest correct
  // in-tree pipeline; pipe 0 = classic IGLP (221 TF), 2 = M0=64 (203 TF)
  int pipe = 1;
  if (const char* pp = std::getenv("KT_CKBWD_PIPE")) pipe = atoi(pp);
  kt_attn_bwd_ck(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                 go.data_ptr(), lse.data_ptr(), d.data_ptr(),
                 dq_acc.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                 dv.data_ptr(), B, Hq, Hkv, S, (float)scale, mask_mode, pipe,
                 cur_stream(q));
  return {dq, dk, dv};
}

void pack_segments(const at::Tensor& base, const at::Tensor& ptrs,
                   const at::Tensor& nbytes, const at::Tensor& offs,
                   bool to_base, int64_t max_nbytes) {
  // One-kernel state-dict pack (to_base=true) / unpack (false) between the
  // flat `base` buffer and the tensors whose data pointers are in `ptrs`.
  // Offsets must be 16B-aligned (ops.aligned_offsets). ptrs/nbytes/offs are
  // int64 CUDA tensors (device-side descriptor table).
  TORCH_CHECK(base.is_cuda() && base.is_contiguous());
  TORCH_CHECK(ptrs.is_cuda() && ptrs.scalar_type() == at::kLong);
  TORCH_CHECK(nbytes.is_cuda() && offs.is_cuda());
  const int nseg = (int)ptrs.numel();
  TORCH_CHECK(nbytes.numel() == nseg && offs.numel() == nseg);
  TORCH_CHECK(nseg > 0 && nseg < 65536, "1..65535 segments");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(base.device());
  kt_pack_segments(ptrs.data_ptr(), nbytes.data_ptr(), offs.data_ptr(),
                   base.data_ptr(), nseg, (long)max_nbytes, to_base ? 1 : 0,
                   cur_stream(base));
}

at::Tensor transpose_bf16(const at::Tensor& src) {
  // dst[C, R] = src[R, C]^T. src rows may be strided (a column slice of a
  // wider matrix); every 16 B vector the kernel touches must be aligned.
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kBFloat16,
              "src must be a bf16 GPU tensor");
  TORCH_CHECK(src.dim() == 2, "src must be 2-D");
  const int64_t R = src.size(0), C = src.size(1);
  TORCH_CHECK(R > 0 && C > 0 && R % 8 == 0 && C % 8 == 0,
              "rows and cols must be positive multiples of 8");
  TORCH_CHECK(src.stride(1) == 1 && src.stride(0) >= C &&
                  src.stride(0) % 8 == 0,
              "src needs unit column stride and a row stride >= cols that "
              "is a multiple of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(src.data_ptr()) % 16 == 0,
              "src must be 16 B aligned");
  const int64_t tiles = ((R + 63) / 64) * ((C + 63) / 64);
  TORCH_CHECK(tiles < (int64_t(1) << 31), "too many tiles");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
  auto dst = at::empty({C, R}, src.options());
  kt_transpose_bf16(src.data_ptr(), src.stride(0), dst.data_ptr(), R, C,
                    cur_stream(src));
  return dst;
}

void transpose_segments_bf16(const at::Tensor& flat_src, at::Tensor flat_dst,
                             const at::Tensor& table, int64_t max_tiles) {
  // table: int64 [nseg, 4] on the device = {src offset, dst offset, rows,
  // cols} per 2-D segment. The table lives on the device and is not read
  // back here: ops.transpose_table() validates it against both buffers on
  // the host when it is built.
  CHECK_BF16_CONTIG(flat_src);
  CHECK_BF16_CONTIG(flat_dst);
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kLong &&
                  table.is_contiguous() && table.dim() == 2 &&
                  table.size(1) == 4,
              "table must be a contiguous int64 [nseg, 4] GPU tensor");
  TORCH_CHECK(flat_src.device() == flat_dst.device() &&
              flat_src.device() == table.device());
  const int64_t nseg = table.size(0);
  TORCH_CHECK(nseg > 0 && nseg < 65536, "1..65535 segments");
  TORCH_CHECK(max_tiles > 0 && max_tiles < (int64_t(1) << 31));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(flat_src.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(flat_dst.data_ptr()) % 16 == 0,
              "flat buffers must be 16 B aligned");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(flat_src.device());
  kt_transpose_segments_bf16(flat_src.data_ptr(), flat_dst.data_ptr(),
                             table.data_ptr(), (int)nseg, (long)max_tiles,
                             cur_stream(flat_src));
}

// Shared checks of a paged KV pool pair [num_pages, n_kv, page_size, hd]:
// both bf16, or both OCP e4m3 (returns true) with per-kv-head scales.
// `scales` are the op's k_scale and v_scale, or its k and v inverse scales:
// [n_kv] fp32 on the pools' device, given exactly when the pools are fp8.
// Their values are not looked at (that would be a device sync).
bool check_page_pools(const at::Tensor& k_pages, const at::Tensor& v_pages,
                      const c10::optional<at::Tensor>& k_scale,
                      const c10::optional<at::Tensor>& v_scale) {
  const bool fp8 = k_pages.scalar_type() == at::kFloat8_e4m3fn;
  if (fp8) {
    TORCH_CHECK(k_pages.is_cuda() && v_pages.is_cuda(),
                "k_pages/v_pages must be on GPU");
    TORCH_CHECK(v_pages.scalar_type() == at::kFloat8_e4m3fn,
                "k_pages is float8_e4m3fn, v_pages is not");
    TORCH_CHECK(k_pages.is_contiguous() && v_pages.is_contiguous(),
                "k_pages/v_pages must be contiguous");
    for (const auto* s : {&k_scale, &v_scale}) {
      TORCH_CHECK(s->has_value(), "fp8 pools need k and v scales");
      const at::Tensor& t = s->value();
      TORCH_CHECK(t.is_cuda() && t.device() == k_pages.device() &&
                      t.scalar_type() == at::kFloat && t.is_contiguous() &&
                      t.dim() == 1 && k_pages.dim() == 4 &&
                      t.size(0) == k_pages.size(1),
                  "k/v scales must be [n_kv] contiguous fp32 on the pools' "
                  "device");
    }
  } else {
    CHECK_BF16_CONTIG(k_pages);
    CHECK_BF16_CONTIG(v_pages);
    TORCH_CHECK(!k_scale.has_value() && !v_scale.has_value(),
                "k/v scales are for float8_e4m3fn pools only");
  }
  TORCH_CHECK(k_pages.dim() == 4, "k_pages must be [pages, n_kv, page, hd]");
  TORCH_CHECK(v_pages.sizes() == k_pages.sizes(), "k/v pool shape mismatch");
  TORCH_CHECK(v_pages.device() == k_pages.device(), "k/v pool device");
  const int64_t ps = k_pages.size(2), hd = k_pages.size(3);
  TORCH_CHECK(ps == 16 || ps == 32 || ps == 64,
              "page_size must be 16, 32 or 64, got ", ps);
  TORCH_CHECK(hd == 64 || hd == 128, "head_dim must be 64 or 128, got ", hd);
  TORCH_CHECK(k_pages.size(0) * ps < (int64_t)INT32_MAX,
              "num_pages*page_size must fit int32");
  return fp8;
}

const void* scale_ptr(const c10::optional<at::Tensor>& s) {
  return s.has_value() ? s->data_ptr() : nullptr;
}

void paged_kv_write(const at::Tensor& k_new, const at::Tensor& v_new,
                    at::Tensor k_pages, at::Tensor v_pages,
                    const at::Tensor& slot_mapping,
                    const c10::optional<at::Tensor>& k_inv_scale,
                    const c10::optional<at::Tensor>& v_inv_scale) {
  // k_new / v_new: [T, n_kv, hd] bf16, token and head dims may be strided
  // (qkv-split views, prefill-cache views); slot_mapping: [T] int32 flat
  // physical token index page*page_size + offset, negative = write nothing.
  // fp8 pools: k_inv_scale / v_inv_scale [n_kv] fp32 hold 1/scale.
  const bool fp8 = check_page_pools(k_pages, v_pages, k_inv_scale, v_inv_scale);
  const int Hkv = (int)k_pages.size(1), ps = (int)k_pages.size(2);
  const int hd = (int)k_pages.size(3);
  for (const at::Tensor* t : {&k_new, &v_new}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16,
                "k_new/v_new must be bf16 on GPU");
    TORCH_CHECK(t->device() == k_pages.device(), "k_new/v_new device");
    TORCH_CHECK(t->dim() == 3 && t->size(1) == Hkv && t->size(2) == hd,
                "k_new/v_new must be [T, n_kv, hd] matching the pool");
    TORCH_CHECK(t->size(0) == k_new.size(0), "k_new/v_new length mismatch");
    if (t->numel() == 0) continue;
    TORCH_CHECK(t->stride(2) == 1, "head dim must be contiguous");
    // 16 B vector loads: every row start must be 16 B aligned
    TORCH_CHECK(t->stride(0) % 8 == 0 && t->stride(1) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "k_new/v_new rows must be 16-byte aligned");
  }
  const int64_t T = k_new.size(0);
  TORCH_CHECK(slot_mapping.is_cuda() && slot_mapping.scalar_type() == at::kInt &&
                  slot_mapping.is_contiguous() && slot_mapping.dim() == 1 &&
                  slot_mapping.size(0) == T &&
                  slot_mapping.device() == k_pages.device(),
              "slot_mapping must be [T] contiguous int32 on the pool's device");
  if (T == 0) return;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(k_pages.device());
  if (fp8) {
    kt_paged_kv_write_fp8(
        k_new.data_ptr(), v_new.data_ptr(), k_pages.data_ptr(),
        v_pages.data_ptr(), slot_mapping.data_ptr(), scale_ptr(k_inv_scale),
        scale_ptr(v_inv_scale), (long)T, Hkv, hd, ps, (long)k_pages.size(0),
        k_new.stride(0), k_new.stride(1), v_new.stride(0), v_new.stride(1),
        cur_stream(k_pages));
    return;
  }
  kt_paged_kv_write(k_new.data_ptr(), v_new.data_ptr(), k_pages.data_ptr(),
                    v_pages.data_ptr(), slot_mapping.data_ptr(), (long)T, Hkv,
                    hd, ps, (long)k_pages.size(0), k_new.stride(0),
                    k_new.stride(1), v_new.stride(0), v_new.stride(1),
                    cur_stream(k_pages));
}

at::Tensor paged_attention_decode(const at::Tensor& q,
                                  const at::Tensor& k_pages,
                                  const at::Tensor& v_pages,
                                  const at::Tensor& block_table,
                                  const at::Tensor& seq_lens, double scale,
                                  int64_t num_splits,
                                  const c10::optional<at::Tensor>& k_scale,
                                  const c10::optional<at::Tensor>& v_scale) {
  // q: [B, Hq, hd]; block_table: [B, max_blocks] int32 (-1 = unused);
  // seq_lens: [B] int32 valid tokens per row (0 = inactive, zero output).
  CHECK_BF16_CONTIG(q);
  const bool fp8 = check_page_pools(k_pages, v_pages, k_scale, v_scale);
  const int64_t num_pages = k_pages.size(0);
  const int Hkv = (int)k_pages.size(1), ps = (int)k_pages.size(2);
  const int hd = (int)k_pages.size(3);
  TORCH_CHECK(q.dim() == 3 && q.size(2) == hd,
              "q must be [B, Hq, hd] with the pool's head_dim");
  TORCH_CHECK(q.device() == k_pages.device(), "q and pools on one device");
  const int64_t B = q.size(0), Hq = q.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "GQA requires Hq % Hkv == 0");
  const int64_t G = Hq / Hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8,
              "group Hq/Hkv must be 1, 2, 4 or 8, got ", G);
  TORCH_CHECK(block_table.is_cuda() && block_table.scalar_type() == at::kInt &&
                  block_table.is_contiguous() && block_table.dim() == 2 &&
                  block_table.size(0) == B &&
                  block_table.device() == q.device(),
              "block_table must be [B, max_blocks] contiguous int32 on q's "
              "device");
  TORCH_CHECK(seq_lens.is_cuda() && seq_lens.scalar_type() == at::kInt &&
                  seq_lens.is_contiguous() && seq_lens.dim() == 1 &&
                  seq_lens.size(0) == B && seq_lens.device() == q.device(),
              "seq_lens must be [B] contiguous int32 on q's device");
  const int64_t max_blocks = block_table.size(1);
  // the kernel's token counters are int32 and step past the end by up to
  // one chunk (128 tokens) before the loop test
  TORCH_CHECK(max_blocks * ps < (int64_t)INT32_MAX - 256,
              "max_blocks*page_size must fit int32");
  TORCH_CHECK(num_splits >= 1 && num_splits <= 256,
              "num_splits must be in [1, 256], got ", num_splits);
  TORCH_CHECK(B * Hkv * num_splits < (int64_t)INT32_MAX, "grid too large");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  auto out = at::empty_like(q);
  if (B == 0) return out;
  at::Tensor po, pm, pl;
  void *po_p = nullptr, *pm_p = nullptr, *pl_p = nullptr;
  if (num_splits > 1) {
    auto f32 = q.options().dtype(at::kFloat);
    po = at::empty({B, Hq, num_splits, hd}, f32);
    pm = at::empty({B, Hq, num_splits}, f32);
    pl = at::empty({B, Hq, num_splits}, f32);
    po_p = po.data_ptr();
    pm_p = pm.data_ptr();
    pl_p = pl.data_ptr();
  }
  const int rc = kt_paged_attention_decode(
      q.data_ptr(), k_pages.data_ptr(), v_pages.data_ptr(),
      block_table.data_ptr(), seq_lens.data_ptr(), out.data_ptr(), po_p, pm_p,
      pl_p, (int)B, (int)Hq, Hkv, hd, ps, (int)num_pages, (int)max_blocks,
      (int)num_splits, (float)scale, (int)fp8, scale_ptr(k_scale),
      scale_ptr(v_scale), cur_stream(q));
  TORCH_CHECK(rc == 0, "paged_attention_decode: no kernel for head_dim ", hd,
              " group ", G);
  return out;
}

at::Tensor paged_attention_prefill(const at::Tensor& q,
                                   const at::Tensor& k_pages,
                                   const at::Tensor& v_pages,
                                   const at::Tensor& block_table,
                                   const at::Tensor& cu_q_lens,
                                   const at::Tensor& seq_lens,
                                   int64_t max_q_len, double scale,
                                   const c10::optional<at::Tensor>& k_scale,
                                   const c10::optional<at::Tensor>& v_scale) {
  // q: [T, Hq, hd] packed rows, token and head dims may be strided (a view
  // of the qkv GEMM output); block_table: [B, max_blocks] int32;
  // cu_q_lens: [B+1] int32 cumulative query counts; seq_lens: [B] int32
  // valid tokens per row including this call's query tokens; max_q_len:
  // host bound on every row's query count (sizes the grid, no device sync).
  const bool fp8 = check_page_pools(k_pages, v_pages, k_scale, v_scale);
  const int64_t num_pages = k_pages.size(0);
  const int Hkv = (int)k_pages.size(1), ps = (int)k_pages.size(2);
  const int hd = (int)k_pages.size(3);
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16,
              "q must be bf16 on GPU");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == hd,
              "q must be [T, Hq, hd] with the pool's head_dim");
  TORCH_CHECK(q.device() == k_pages.device(), "q and pools on one device");
  const int64_t T = q.size(0), Hq = q.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "GQA requires Hq % Hkv == 0");
  const int64_t G = Hq / Hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8,
              "group Hq/Hkv must be 1, 2, 4 or 8, got ", G);
  if (q.numel() > 0) {
    TORCH_CHECK(q.stride(2) == 1, "q head dim must be contiguous");
    TORCH_CHECK(q.stride(0) % 8 == 0 && q.stride(1) % 8 == 0 &&
                    q.stride(0) >= 0 && q.stride(1) >= 0 &&
                    reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
                "q rows must be 16-byte aligned");
  }
  TORCH_CHECK(block_table.is_cuda() && block_table.scalar_type() == at::kInt &&
                  block_table.is_contiguous() && block_table.dim() == 2 &&
                  block_table.device() == q.device(),
              "block_table must be [B, max_blocks] contiguous int32 on q's "
              "device");
  const int64_t B = block_table.size(0);
  TORCH_CHECK(cu_q_lens.is_cuda() && cu_q_lens.scalar_type() == at::kInt &&
                  cu_q_lens.is_contiguous() && cu_q_lens.dim() == 1 &&
                  cu_q_lens.size(0) == B + 1 &&
                  cu_q_lens.device() == q.device(),
              "cu_q_lens must be [B+1] contiguous int32 on q's device");
  TORCH_CHECK(seq_lens.is_cuda() && seq_lens.scalar_type() == at::kInt &&
                  seq_lens.is_contiguous() && seq_lens.dim() == 1 &&
                  seq_lens.size(0) == B && seq_lens.device() == q.device(),
              "seq_lens must be [B] contiguous int32 on q's device");
  const int64_t max_blocks = block_table.size(1);
  TORCH_CHECK(max_blocks * ps < (int64_t)INT32_MAX - 256,
              "max_blocks*page_size must fit int32");
  TORCH_CHECK(scale > 0 && std::isfinite(scale),
              "scale must be positive and finite");
  TORCH_CHECK(max_q_len >= 0 && max_q_len < (int64_t)INT32_MAX - 256,
              "max_q_len must be in [0, 2^31)");
  TORCH_CHECK(B <= 65535 && Hkv <= 65535, "grid too large");
  TORCH_CHECK(T * Hq * hd < (int64_t(1) << 46), "q too large");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  auto out = at::zeros({T, Hq, hd}, q.options());
  if (T == 0 || B == 0 || max_q_len == 0) return out;
  const int rc = kt_paged_attention_prefill(
      q.data_ptr(), k_pages.data_ptr(), v_pages.data_ptr(),
      block_table.data_ptr(), cu_q_lens.data_ptr(), seq_lens.data_ptr(),
      out.data_ptr(), (long)T, (long)q.stride(0), (long)q.stride(1), (int)B,
      (int)Hq, Hkv, hd, ps, (int)num_pages, (int)max_blocks, (int)max_q_len,
      (float)scale, (int)fp8, scale_ptr(k_scale), scale_ptr(v_scale),
      cur_stream(q));
  TORCH_CHECK(rc == 0, "paged_attention_prefill: no kernel for head_dim ", hd,
              " group ", G);
  return out;
}

at::Tensor sample_tokens(const at::Tensor& logits,
                         const at::Tensor& temperature,
                         const at::Tensor& top_k, const at::Tensor& top_p,
                         const at::Tensor& seed, const at::Tensor& offset) {
  // logits: [B, V] bf16, last dim contiguous, row base and stride 16 B
  // aligned (ops.sample_tokens sends everything else to the reference).
  // The five parameter vectors are [B] on the logits' device; their values
  // are not looked at here (that would be a device sync).
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16 &&
                  logits.dim() == 2,
              "logits must be [B, V] bf16 on GPU");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V <= 262144, "V must be in [1, 262144], got ", V);
  TORCH_CHECK(B < (int64_t)INT32_MAX, "batch too large");
  TORCH_CHECK(V == 1 || logits.stride(1) == 1,
              "logits' last dim must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0 &&
                  (B <= 1 ||
                   (logits.stride(0) >= 0 && logits.stride(0) % 8 == 0)),
              "logits rows must be 16-byte aligned");
  const struct {
    const at::Tensor* t;
    at::ScalarType dt;
    const char* name;
  } params[] = {{&temperature, at::kFloat, "temperature must be [B] fp32"},
                {&top_k, at::kInt, "top_k must be [B] int32"},
                {&top_p, at::kFloat, "top_p must be [B] fp32"},
                {&seed, at::kLong, "seed must be [B] int64"},
                {&offset, at::kLong, "offset must be [B] int64"}};
  for (const auto& p : params) {
    TORCH_CHECK(p.t->is_cuda() && p.t->device() == logits.device() &&
                    p.t->scalar_type() == p.dt && p.t->dim() == 1 &&
                    p.t->size(0) == B && p.t->is_contiguous(),
                p.name, ", contiguous, on the logits' device");
  }
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  auto out = at::empty({B}, logits.options().dtype(at::kLong));
  if (B == 0) return out;
  kt_sample_tokens(logits.data_ptr(), B > 1 ? (long)logits.stride(0) : 0,
                   (int)B, (int)V, temperature.data_ptr(), top_k.data_ptr(),
                   top_p.data_ptr(), seed.data_ptr(), offset.data_ptr(),
                   out.data_ptr(), cur_stream(logits));
  return out;
}

std::vector<at::Tensor> token_logprobs(const at::Tensor& logits,
                                       const at::Tensor& token,
                                       const at::Tensor& temperature,
                                       int64_t top_n) {
  // logits as for sample_tokens (ops.token_logprobs sends everything else
  // to the reference); token [B] int64 and temperature [B] fp32 on the
  // logits' device. Their values are not looked at here (that would be a
  // device sync): the kernel reads no logit for a token outside [0, V).
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16 &&
                  logits.dim() == 2,
              "logits must be [B, V] bf16 on GPU");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V <= 262144, "V must be in [1, 262144], got ", V);
  TORCH_CHECK(B < (int64_t)INT32_MAX, "batch too large");
  TORCH_CHECK(V == 1 || logits.stride(1) == 1,
              "logits' last dim must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0 &&
                  (B <= 1 ||
                   (logits.stride(0) >= 0 && logits.stride(0) % 8 == 0)),
              "logits rows must be 16-byte aligned");
  TORCH_CHECK(top_n >= 0 && top_n <= 32, "top_n must be in [0, 32], got ",
              top_n);
  TORCH_CHECK(token.is_cuda() && token.device() == logits.device() &&
                  token.scalar_type() == at::kLong && token.dim() == 1 &&
                  token.size(0) == B && token.is_contiguous(),
              "token must be [B] int64, contiguous, on the logits' device");
  TORCH_CHECK(temperature.is_cuda() &&
                  temperature.device() == logits.device() &&
                  temperature.scalar_type() == at::kFloat &&
                  temperature.dim() == 1 && temperature.size(0) == B &&
                  temperature.is_contiguous(),
              "temperature must be [B] fp32, contiguous, on the logits' "
              "device");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  auto f32 = logits.options().dtype(at::kFloat);
  auto i32 = logits.options().dtype(at::kInt);
  auto logprob = at::empty({B}, f32);
  auto rank = at::empty({B}, i32);
  auto top_ids = at::empty({B, top_n}, i32);
  auto top_lp = at::empty({B, top_n}, f32);
  if (B > 0)
    kt_token_logprobs(logits.data_ptr(), B > 1 ? (long)logits.stride(0) : 0,
                      (int)B, (int)V, token.data_ptr(),
                      temperature.data_ptr(), (int)top_n, logprob.data_ptr(),
                      rank.data_ptr(), top_ids.data_ptr(), top_lp.data_ptr(),
                      cur_stream(logits));
  return {logprob, rank, top_ids, top_lp};
}

at::Tensor linear_w8(const at::Tensor& x, const at::Tensor& wq,
                     const at::Tensor& scale, int64_t num_splits) {
  // x: [M, K] bf16, 1 <= M <= 32, last dim contiguous, row base and stride
  // 16 B aligned; wq: [N, K] e4m3 contiguous, K % 128 == 0; scale: [N] fp32
  // (ops.linear_w8 sends everything else to the composition). num_splits 0
  // is the kernel's own choice from (N, K). The scale values are not looked
  // at here (that would be a device sync).
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2,
              "x must be [M, K] bf16 on GPU");
  TORCH_CHECK(wq.is_cuda() && wq.device() == x.device() &&
                  wq.scalar_type() == at::kFloat8_e4m3fn && wq.dim() == 2 &&
                  wq.is_contiguous(),
              "weight_q must be [N, K] float8_e4m3fn, contiguous, on x's "
              "device");
  const int64_t M = x.size(0), K = x.size(1), N = wq.size(0);
  TORCH_CHECK(wq.size(1) == K, "x's last dim must be weight_q's K");
  TORCH_CHECK(scale.is_cuda() && scale.device() == x.device() &&
                  scale.scalar_type() == at::kFloat && scale.dim() == 1 &&
                  scale.size(0) == N && scale.is_contiguous(),
              "weight_scale must be [N] fp32, contiguous, on x's device");
  TORCH_CHECK(M >= 1 && M <= 32, "M must be in [1, 32], got ", M);
  TORCH_CHECK(K >= 128 && K % 128 == 0 && K <= (1 << 24),
              "K must be a multiple of 128 up to 2^24, got ", K);
  TORCH_CHECK(N >= 1 && N <= (1 << 30), "N must be in [1, 2^30], got ", N);
  const int64_t xs = M > 1 ? x.stride(0) : K;
  TORCH_CHECK(x.stride(1) == 1, "x's last dim must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  xs >= 0 && xs % 8 == 0 && xs <= (1 << 24),
              "x rows must be 16-byte aligned, with a stride up to 2^24");
  TORCH_CHECK(num_splits >= 0 && num_splits <= 64,
              "num_splits must be in [0, 64], got ", num_splits);
  const int S = num_splits > 0 ? (int)num_splits : kt_linear_w8_plan(N, K);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({M, N}, x.options());
  at::Tensor part;
  if (S > 1) part = at::empty({S, M, N}, x.options().dtype(at::kFloat));
  kt_linear_w8(x.data_ptr(), (long)xs, wq.data_ptr(), scale.data_ptr(),
               y.data_ptr(), S > 1 ? part.data_ptr() : nullptr, (int)M, (int)N,
               (int)K, S, cur_stream(x));
  return y;
}

int64_t linear_w8_splits(int64_t N, int64_t K) {
  TORCH_CHECK(N >= 1 && K >= 128 && K % 128 == 0, "bad [N, K]");
  return kt_linear_w8_plan(N, K);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("attn_fwd", &attn_fwd,
          "Causal GQA attention fwd (bf16, D=128) -> (o, lse)");
  mod.def("attn_fwd_ck", &attn_fwd_ck,
          "CK-tile FMHA fwd (bf16, D=128, causal, GQA) -> (o, lse)");
  mod.def("attn_fwd_ck_tr", &attn_fwd_ck_tr,
          "CK-tile FMHA fwd, gfx950 tr-load variant -> (o, lse)");
  mod.def("attn_fwd_v3", &attn_fwd_v3,
          "CK-tile FMHA v3 (AITER schedule) fwd with LSE -> (o, lse)",
          pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
          pybind11::arg("scale"), pybind11::arg("prescaled") = false);
  mod.def("rmsnorm_fwd", &rmsnorm_fwd, "RMSNorm forward (bf16)");
  mod.def("rmsnorm_bwd", &rmsnorm_bwd, "RMSNorm backward (bf16)");
  mod.def("rope", &rope, "RoPE rotate-half (bf16), sign=+1 fwd / -1 bwd",
          pybind11::arg("x"), pybind11::arg("cost"), pybind11::arg("sint"),
          pybind11::arg("S"), pybind11::arg("sign"),
          pybind11::arg("oscale") = 1.0);
  mod.def("attn_grad_pack", &attn_grad_pack,
          "GQA group sum + RoPE^T + qkv packing of (dq, dk_exp, dv_exp)",
          pybind11::arg("dq"), pybind11::arg("dk_e"), pybind11::arg("dv_e"),
          pybind11::arg("cost"), pybind11::arg("sint"), pybind11::arg("n_kv"),
          pybind11::arg("q_oscale"));
  mod.def("swiglu_fwd", &swiglu_fwd, "SwiGLU forward (bf16)");
  mod.def("swiglu_bwd", &swiglu_bwd, "SwiGLU backward (bf16)");
  mod.def("cross_entropy_fwd_", &cross_entropy_fwd_,
          "Fused CE: returns per-row loss, overwrites logits with grad");
  mod.def("scale_bf16", &scale_bf16,
          "bf16(x * scale), scale one fp32 value in device memory");
  mod.def("adamw_", &adamw_, "Fused AdamW on a flat bf16 bucket");
  mod.def("transpose_bf16", &transpose_bf16,
          "dst[C,R] = src[R,C]^T (bf16, LDS-tiled; src rows may be strided)");
  mod.def("transpose_segments_bf16", &transpose_segments_bf16,
          "Transpose every 2-D segment of a flat bf16 buffer in one launch");
  mod.def("pack_segments", &pack_segments,
          "One-kernel multi-tensor pack/unpack vs a flat buffer");
  mod.def("attn_bwd_ck", &attn_bwd_ck,
          "CK-tile GQA-native FMHA backward -> (dq, dk_exp, dv_exp)");
  mod.def("paged_kv_write", &paged_kv_write,
          "Scatter [T, n_kv, hd] k/v rows into paged pools by slot_mapping");
  mod.def("paged_attention_decode", &paged_attention_decode,
          "Single-token GQA attention over a block-table paged KV cache");
  mod.def("paged_attention_prefill", &paged_attention_prefill,
          "Causal GQA attention of packed query tokens over a paged KV cache");
  mod.def("sample_tokens", &sample_tokens,
          "Per-row temperature / top-k / top-p / seeded token sampling");
  mod.def("token_logprobs", &token_logprobs,
          "Per-row log-probability and rank of a token, and the top_n tokens");
  mod.def("linear_w8", &linear_w8,
          "y = x @ (e4m3 weight * scale)^T for M <= 32 rows of bf16 x");
  mod.def("linear_w8_splits", &linear_w8_splits,
          "The split-K factor linear_w8 chooses for an [N, K] weight");
}
