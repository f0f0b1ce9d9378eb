// The extern "C" launchers of the kubetorch_amd HIP kernels, declared once.
// bindings.cpp calls them through this header and every .hip file that
// defines one includes it, so a definition whose parameter list differs from
// its declaration does not compile (C linkage cannot be overloaded) instead
// of linking and reading garbage arguments.
//
// Depends on nothing but the HIP runtime API: it is included by translation
// units with and without torch headers and the __HIP_NO_HALF_* guards.
#pragma once

#include <hip/hip_runtime_api.h>

extern "C" {

// kernels.hip
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
void kt_pack_segments(const void* ptrs, const void* nbytes, const void* offs,
                      void* base, int nseg, long max_nbytes, int to_base,
                      hipStream_t stream);
void kt_transpose_bf16(const void* src, long src_stride, void* dst, long R,
                       long C, hipStream_t stream);
void kt_transpose_segments_bf16(const void* src, void* dst, const void* table,
                                int nseg, long max_tiles, hipStream_t stream);

// attention.hip
void kt_attn_fwd(const void* q, const void* k, const void* v, void* o,
                 void* lse, int B, int Hq, int Hkv, int S, float scale,
                 hipStream_t stream);

// attention_ck.hip
void kt_attn_fwd_ck(const void* q, const void* k, const void* v, void* o,
                    void* lse, int B, int Hq, int Hkv, int S, float scale,
                    const long* strides, hipStream_t stream);
void kt_attn_fwd_ck_tr(const void* q, const void* k, const void* v, void* o,
                       void* lse, int B, int Hq, int Hkv, int S, float scale,
                       const long* strides, hipStream_t stream);
void kt_attn_fwd_v3(const void* q, const void* k, const void* v, void* o,
                    void* lse, int B, int Hq, int Hkv, int S, float scale,
                    const long* strides, hipStream_t stream);

// attention_ck_bwd.hip
void kt_attn_bwd_ck(const void* q, const void* k, const void* v,
                    const void* o, const void* do_, const void* lse, void* d,
                    void* dq_acc, void* dq, void* dk, void* dv, int B, int Hq,
                    int Hkv, int S, float scale, int mask_mode, int pipe,
                    hipStream_t stream);

// paged_attention.hip. fp8 != 0: the pools are e4m3 and the two scale
// arguments are [Hkv] fp32 device arrays (1/scale for the write); otherwise
// bf16 pools, and the scales are not read.
void kt_paged_kv_write(const void* k_new, const void* v_new, void* k_pages,
                       void* v_pages, const void* slot_mapping,
                       const void* k_inv, const void* v_inv, int fp8, long T,
                       int Hkv, int hd, int page_size, long num_pages,
                       long k_st, long k_sh, long v_st, long v_sh,
                       hipStream_t stream);
int kt_paged_attention_decode(const void* q, const void* k_pages,
                              const void* v_pages, const void* block_table,
                              const void* seq_lens, void* out, void* po,
                              void* pm, void* pl, int B, int Hq, int Hkv,
                              int hd, int page_size, int num_pages,
                              int max_blocks, int num_splits, float scale,
                              int fp8, const void* k_scale,
                              const void* v_scale, hipStream_t stream);

// paged_prefill.hip
int kt_paged_attention_prefill(const void* q, const void* k_pages,
                               const void* v_pages, const void* block_table,
                               const void* cu_q_lens, const void* seq_lens,
                               void* out, long T, long q_st, long q_sh, int B,
                               int Hq, int Hkv, int hd, int page_size,
                               int num_pages, int max_blocks, int max_q_len,
                               float scale, int fp8, const void* k_scale,
                               const void* v_scale, hipStream_t stream);

// sampler.hip, logprobs.hip
void kt_sample_tokens(const void* logits, long row_stride, int B, int V,
                      const void* temperature, const void* top_k,
                      const void* top_p, const void* seed, const void* offset,
                      void* out, hipStream_t stream);
void kt_token_logprobs(const void* logits, long row_stride, int B, int V,
                       const void* token, const void* temperature, int top_n,
                       void* logprob, void* rank, void* top_ids,
                       void* top_logprobs, hipStream_t stream);

// linear_w8.hip
int kt_linear_w8_plan(long N, long K);
void kt_linear_w8(const void* x, long x_stride, const void* wq,
                  const void* scale, void* y, void* part, int M, int N, int K,
                  int S, hipStream_t stream);
// more than 32 rows: 64-row tiles, the same plan and reduce
void kt_linear_w8_wide(const void* x, long x_stride, const void* wq,
                       const void* scale, void* y, void* part, int M, int N,
                       int K, int S, hipStream_t stream);

// moe.hip. kt_moe_route writes the routing table that kt_moe_mlp reads.
// fp8 != 0: the expert weights are e4m3 and the two scale arguments are
// [E, 2I] and [E, D] fp32 device arrays; otherwise bf16 weights, and the
// scales are not read.
int kt_moe_down_plan(long D, long I, int E, int top_k);
void kt_moe_route(const void* logits, int is_bf16, void* sel, void* weights,
                  void* expert_count, void* expert_rows, int T, int E,
                  int top_k, hipStream_t stream);
void kt_moe_mlp(const void* x, long x_stride, const void* w_gate_up,
                const void* w_down, const void* weights,
                const void* expert_count, const void* expert_rows, void* h,
                void* part, void* out, int T, int D, int I, int E, int top_k,
                int S, int fp8, const void* gate_up_scale,
                const void* down_scale, hipStream_t stream);
// out [T, D] bf16 = the sum over s, then j, of part [S, T, top_k, D] fp32
void kt_moe_combine(const void* part, void* out, int T, int D, int top_k,
                    int S, hipStream_t stream);

// moe_grouped.hip: the same MLP for more than 32 rows. The scratch arrays are
// sized by kt_moe_grouped_max_tiles (tiles of kt_moe_grouped_tile_rows rows).
int kt_moe_grouped_tile_rows(void);
int kt_moe_grouped_max_tiles(long T, int E, int top_k);
void kt_moe_grouped_mlp(const void* x, long x_stride, const void* logits,
                        int is_bf16, const void* w_gate_up,
                        const void* w_down, void* sel, void* weights,
                        void* expert_count, void* sorted_pairs,
                        void* tile_expert, void* tile_row0, void* n_tiles,
                        void* h, void* part, void* out, int T, int D, int I,
                        int E, int top_k, int fp8, const void* gate_up_scale,
                        const void* down_scale, hipStream_t stream);

}  // extern "C"
