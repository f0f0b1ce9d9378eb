// Paged KV cache kernels for the serving decode step (gfx950 / CDNA4).
//
// Pool layout, per layer: k_pages / v_pages [num_pages, n_kv, page_size, hd]
// bf16, so one (page, kv head) is one contiguous page_size*hd*2-byte run.
// The same layout with one-byte OCP e4m3 elements is the fp8 pool: a byte
// encodes x / scale with a static fp32 scale per kv head (k_scale, v_scale
// [n_kv], read from device memory). e4m3 -> fp32 is exact, so the fp8
// kernels are the bf16 kernels with another load and conversion (template
// parameter FP8): k_scale folds into the score scale, v_scale multiplies
// the merged fp32 accumulator once.
//
//  - paged_kv_write: scatters [T, n_kv, hd] rows into their pages by a flat
//    physical token index (page*page_size + offset); 16 B per lane.
//  - paged_attention_decode: single-token GQA attention over a block table.
//    One workgroup per (sequence, kv head, split). The decode step is a
//    memory-bound KV read, so K and V go straight from global memory to
//    VGPRs with 16 B loads (no LDS staging) and every loaded element serves
//    all Hq/Hkv query rows of the kv head. A token row (hd bf16) is spread
//    over hd/8 adjacent lanes; a wave load covers 64*8/hd whole tokens,
//    i.e. 1 KiB of one page. Each lane group keeps its own online-softmax
//    state (m, l, acc) in fp32 in the exp2 domain; the states are merged
//    once at the end (lanes by shuffle, waves through LDS).
//  - Split-KV: the grid is static (B x Hkv x num_splits); each workgroup
//    derives its page range from seq_lens[b] on the device. Partials are
//    fp32 (o, m, l); a second small kernel merges them. No atomics.
//
// Tokens at or past seq_lens[b], table entries outside [0, num_pages) and
// everything past max_blocks*page_size are skipped: never loaded, never
// multiplied by a zero probability.
//
// No torch headers here; bindings.cpp declares the extern "C" launchers.

#include <hip/hip_runtime.h>

typedef unsigned short u16;
typedef ushort vec8u __attribute__((ext_vector_type(8)));
typedef unsigned int vec2w __attribute__((ext_vector_type(2)));
typedef float vec2f __attribute__((ext_vector_type(2)));

#define PA_WAVES 4
#define PA_THREADS (PA_WAVES * 64)
#define PA_UNROLL 4

namespace {

__device__ __forceinline__ float bf2f(u16 x) {
  return __uint_as_float(((unsigned int)x) << 16);
}
__device__ __forceinline__ u16 f2bf(float f) {
  // round-to-nearest-even; NaN (from non-finite K/V data) stays NaN
  unsigned int u = __float_as_uint(f);
  if (f != f) return (u16)0x7fc0;
  u += 0x7fff + ((u >> 16) & 1);
  return (u16)(u >> 16);
}

// The 8 K/V elements a lane loads at once: 16 B of bf16 or 8 B of e4m3.
template <bool FP8>
struct KV8 {
  typedef u16 elem;
  typedef vec8u vec;
  static __device__ __forceinline__ void to_f32(vec v, float* f) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = bf2f(v[e]);
  }
};
template <>
struct KV8<true> {
  typedef unsigned char elem;
  typedef vec2w vec;
  static __device__ __forceinline__ void to_f32(vec v, float* f) {
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const vec2f lo = __builtin_amdgcn_cvt_pk_f32_fp8(v[w], false);
      const vec2f hi = __builtin_amdgcn_cvt_pk_f32_fp8(v[w], true);
      f[4 * w] = lo[0];
      f[4 * w + 1] = lo[1];
      f[4 * w + 2] = hi[0];
      f[4 * w + 3] = hi[1];
    }
  }
};

// fp32 -> the value the e4m3 conversion rounds: x * inv_scale clamped to
// the finite range +-448 (so +-inf saturate). fmin/fmax drop a NaN operand,
// so NaN is passed through explicitly and stays NaN in the pool.
__device__ __forceinline__ float fp8_prep(float x, float inv_scale) {
  const float y = x * inv_scale;
  return y != y ? y : fminf(fmaxf(y, -448.f), 448.f);
}

// 8 bf16 -> 8 e4m3 bytes (round to nearest even)
__device__ __forceinline__ vec2w quantize8(vec8u x, float inv_scale) {
  float y[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = fp8_prep(bf2f(x[e]), inv_scale);
  vec2w r;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w], y[4 * w + 1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w + 2], y[4 * w + 3], p, true);
    r[w] = (unsigned int)p;
  }
  return r;
}

// Sum over the LPT (8 or 16) adjacent lanes that hold one token row; every
// lane of the group gets the total. DPP controls: quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, row_mirror. All 64 lanes are
// active wherever this is called.
template <int LPT>
__device__ __forceinline__ float group_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(
      0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
  v += __int_as_float(__builtin_amdgcn_update_dpp(
      0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
  v += __int_as_float(__builtin_amdgcn_update_dpp(
      0, __float_as_int(v), 0x141, 0xF, 0xF, true));
  if (LPT == 16)
    v += __int_as_float(__builtin_amdgcn_update_dpp(
        0, __float_as_int(v), 0x140, 0xF, 0xF, true));
  return v;
}

// exp2(m - M) for merging a partial state with max m into one with max M
// (M >= m). An empty state has m = -inf; with M = -inf as well the plain
// difference is NaN, so empty states get weight 0 explicitly.
__device__ __forceinline__ float merge_weight(float m, float M) {
  return m == -INFINITY ? 0.f : exp2f(m - M);
}

// ---------------------------------------------------------------------------
// paged_kv_write
// ---------------------------------------------------------------------------
__global__ void paged_kv_write_kernel(const u16* __restrict__ k_new,
                                      const u16* __restrict__ v_new,
                                      u16* __restrict__ k_pages,
                                      u16* __restrict__ v_pages,
                                      const int* __restrict__ slot_mapping,
                                      long total_vecs, int Hkv, int hd,
                                      int page_size, long pool_tokens,
                                      long k_st, long k_sh, long v_st,
                                      long v_sh) {
  const int vpr = hd >> 3;  // 16 B vectors per head row
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total_vecs;
       i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i % vpr);
    const long th = i / vpr;
    const int h = (int)(th % Hkv);
    const long t = th / Hkv;
    const long slot = slot_mapping[t];
    if (slot < 0 || slot >= pool_tokens) continue;  // "write nothing"
    const long page = slot / page_size;
    const long off = slot - page * page_size;
    const size_t dst = (((size_t)page * Hkv + h) * page_size + off) * hd + j * 8;
    *reinterpret_cast<vec8u*>(k_pages + dst) =
        *reinterpret_cast<const vec8u*>(k_new + t * k_st + h * k_sh + j * 8);
    *reinterpret_cast<vec8u*>(v_pages + dst) =
        *reinterpret_cast<const vec8u*>(v_new + t * v_st + h * v_sh + j * 8);
  }
}

// The same scatter into fp8 pools: a lane loads 8 bf16 of K and of V,
// multiplies by the head's 1/scale (computed on the host side of the op),
// and stores 8 bytes of each.
__global__ void paged_kv_write_fp8_kernel(
    const u16* __restrict__ k_new, const u16* __restrict__ v_new,
    unsigned char* __restrict__ k_pages, unsigned char* __restrict__ v_pages,
    const int* __restrict__ slot_mapping, const float* __restrict__ k_inv,
    const float* __restrict__ v_inv, long total_vecs, int Hkv, int hd,
    int page_size, long pool_tokens, long k_st, long k_sh, long v_st,
    long v_sh) {
  const int vpr = hd >> 3;  // 8-element vectors per head row
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total_vecs;
       i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i % vpr);
    const long th = i / vpr;
    const int h = (int)(th % Hkv);
    const long t = th / Hkv;
    const long slot = slot_mapping[t];
    if (slot < 0 || slot >= pool_tokens) continue;  // "write nothing"
    const long page = slot / page_size;
    const long off = slot - page * page_size;
    const size_t dst = (((size_t)page * Hkv + h) * page_size + off) * hd + j * 8;
    *reinterpret_cast<vec2w*>(k_pages + dst) = quantize8(
        *reinterpret_cast<const vec8u*>(k_new + t * k_st + h * k_sh + j * 8),
        k_inv[h]);
    *reinterpret_cast<vec2w*>(v_pages + dst) = quantize8(
        *reinterpret_cast<const vec8u*>(v_new + t * v_st + h * v_sh + j * 8),
        v_inv[h]);
  }
}

// ---------------------------------------------------------------------------
// paged_attention_decode, first kernel
// ---------------------------------------------------------------------------
// q [B, Hq, HD] bf16; out [B, Hq, HD] bf16 (written when num_splits == 1);
// po [B, Hq, S, HD], pm / pl [B, Hq, S] fp32 partials otherwise. po is the
// unnormalised accumulator sum_t 2^(s_t - m) v_t, times v_scale[kvh] over
// fp8 pools (k_scale / v_scale are read only there).
template <int HD, int G, bool FP8>
__global__ __launch_bounds__(PA_THREADS) void paged_attn_decode_kernel(
    const u16* __restrict__ q,
    const typename KV8<FP8>::elem* __restrict__ k_pages,
    const typename KV8<FP8>::elem* __restrict__ v_pages,
    const int* __restrict__ block_table, const int* __restrict__ seq_lens,
    u16* __restrict__ out, float* __restrict__ po, float* __restrict__ pm,
    float* __restrict__ pl, int Hkv, int num_pages, int max_blocks,
    int page_shift, int num_splits, float qscale,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale) {
  typedef typename KV8<FP8>::vec kvec;
  constexpr int LPT = HD / 8;    // lanes per token row
  constexpr int NSLOT = 64 / LPT;  // tokens per wave load
  constexpr int CHUNK = PA_WAVES * PA_UNROLL * NSLOT;  // tokens per iteration

  const int split = blockIdx.x % num_splits;
  const int kvh = (blockIdx.x / num_splits) % Hkv;
  const int b = blockIdx.x / (num_splits * Hkv);
  const int Hq = Hkv * G;
  const int page_size = 1 << page_shift;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane % LPT;     // which 8 dims of the row
  const int slot = lane / LPT;  // which token of the wave load

  // token range of this split, from the sequence's own length
  int n = seq_lens[b];
  const int cap = max_blocks << page_shift;  // host checks this fits int32
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const int npages = (n + page_size - 1) >> page_shift;
  const int pps = (npages + num_splits - 1) / num_splits;
  const int p0 = split * pps;
  int p1 = p0 + pps;
  p1 = p1 > npages ? npages : p1;
  const int t0 = p0 << page_shift;
  int t1 = p1 << page_shift;
  t1 = t1 > n ? n : t1;  // t1 <= t0 when the split is empty

  // q rows of this kv head, scale*log2(e) (times the head's K scale over
  // fp8 pools) folded in, fp32
  if (FP8) qscale *= k_scale[kvh];
  float qf[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    vec8u qv = (vec8u)0;
    if (t0 < t1)
      qv = *reinterpret_cast<const vec8u*>(
          q + ((size_t)b * Hq + kvh * G + g) * HD + j * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[g][e] = bf2f(qv[e]) * qscale;
  }

  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  }

  const int* bt = block_table + (size_t)b * max_blocks;
  const size_t page_stride = (size_t)Hkv << page_shift;  // rows per page

  for (int base = t0; base < t1; base += CHUNK) {  // block-uniform trip count
    bool valid[PA_UNROLL];
    size_t row[PA_UNROLL];
#pragma unroll
    for (int u = 0; u < PA_UNROLL; ++u) {
      const int t = base + (u * PA_WAVES + wave) * NSLOT + slot;
      int pg = -1;
      if (t < t1) pg = bt[t >> page_shift];  // t < cap: inside the table row
      valid[u] = pg >= 0 && pg < num_pages;
      row[u] = (size_t)pg * page_stride + ((size_t)kvh << page_shift) +
               (t & (page_size - 1));
    }
    kvec kv[PA_UNROLL], vv[PA_UNROLL];
#pragma unroll
    for (int u = 0; u < PA_UNROLL; ++u) {
      kv[u] = (kvec)0;
      vv[u] = (kvec)0;
      if (valid[u]) {
        kv[u] = *reinterpret_cast<const kvec*>(k_pages + row[u] * HD + j * 8);
        vv[u] = *reinterpret_cast<const kvec*>(v_pages + row[u] * HD + j * 8);
      }
    }
    // scores of the chunk's tokens for all G rows (skipped tokens: -inf,
    // computed from zeros, never from memory)
    float s[PA_UNROLL][G];
#pragma unroll
    for (int u = 0; u < PA_UNROLL; ++u) {
      float kf[8];
      KV8<FP8>::to_f32(kv[u], kf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(qf[g][e], kf[e], d);
        d = group_sum<LPT>(d);
        s[u][g] = valid[u] ? d : -INFINITY;
      }
    }
    // one rescale per chunk, then p*v for every valid token
    float p[PA_UNROLL][G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < PA_UNROLL; ++u) mn = fmaxf(mn, s[u][g]);
      // mn == -inf only while this lane group has seen no valid token;
      // then l and acc are 0 and stay 0 (alpha 1, every p 0)
      const float alpha = mn == -INFINITY ? 1.f : exp2f(m[g] - mn);
      m[g] = mn;
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < PA_UNROLL; ++u) {
        p[u][g] = valid[u] ? exp2f(s[u][g] - mn) : 0.f;
        ps += p[u][g];
      }
      l[g] = l[g] * alpha + ps;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < PA_UNROLL; ++u) {
      if (valid[u]) {  // a skipped token adds nothing, not 0 * v
        float vf[8];
        KV8<FP8>::to_f32(vv[u], vf);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < 8; ++e)
            acc[g][e] = fmaf(p[u][g], vf[e], acc[g][e]);
      }
    }
  }

  // merge the NSLOT lane-group states of the wave (lanes j, j+LPT, ...)
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float M = m[g];
#pragma unroll
    for (int o = LPT; o < 64; o <<= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    const float w = merge_weight(m[g], M);
    float lg = l[g] * w;
#pragma unroll
    for (int o = LPT; o < 64; o <<= 1) lg += __shfl_xor(lg, o, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = acc[g][e] * w;
#pragma unroll
      for (int o = LPT; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
      acc[g][e] = a;
    }
    m[g] = M;
    l[g] = lg;
  }

  // merge the waves through LDS: PA_WAVES x G x (HD + m + l) fp32, 16.3 KiB
  // at HD 128, G 8
  __shared__ float s_acc[PA_WAVES][G][HD];
  __shared__ float s_m[PA_WAVES][G];
  __shared__ float s_l[PA_WAVES][G];
  if (slot == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int e = 0; e < 8; ++e) s_acc[wave][g][j * 8 + e] = acc[g][e];
      if (j == 0) {
        s_m[wave][g] = m[g];
        s_l[wave][g] = l[g];
      }
    }
  }
  __syncthreads();
  const float vs = FP8 ? v_scale[kvh] : 1.f;
  for (int idx = threadIdx.x; idx < G * HD; idx += PA_THREADS) {
    const int g = idx / HD;
    const int d = idx - g * HD;
    float M = s_m[0][g];
#pragma unroll
    for (int w = 1; w < PA_WAVES; ++w) M = fmaxf(M, s_m[w][g]);
    float a = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < PA_WAVES; ++w) {
      const float f = merge_weight(s_m[w][g], M);
      a += s_acc[w][g][d] * f;
      L += s_l[w][g] * f;
    }
    if (FP8) a *= vs;
    const size_t hrow = (size_t)b * Hq + kvh * G + g;
    if (num_splits == 1) {
      // L == 0 only for an empty sequence: an all-zero row
      out[hrow * HD + d] = L > 0.f ? f2bf(a / L) : (u16)0;
    } else {
      const size_t prow = hrow * num_splits + split;
      po[prow * HD + d] = a;
      if (d == 0) {
        pm[prow] = M;
        pl[prow] = L;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// second kernel: merge the splits' partials; one block per (b, q head)
// ---------------------------------------------------------------------------
__global__ void paged_attn_combine_kernel(const float* __restrict__ po,
                                          const float* __restrict__ pm,
                                          const float* __restrict__ pl,
                                          u16* __restrict__ out, int HD,
                                          int num_splits) {
  const size_t hrow = blockIdx.x;
  const int d = threadIdx.x;
  if (d >= HD) return;
  const float* m = pm + hrow * num_splits;
  const float* l = pl + hrow * num_splits;
  float M = -INFINITY;
  for (int s = 0; s < num_splits; ++s) M = fmaxf(M, m[s]);
  float a = 0.f, L = 0.f;
  for (int s = 0; s < num_splits; ++s) {
    const float f = merge_weight(m[s], M);
    a += po[(hrow * num_splits + s) * HD + d] * f;
    L += l[s] * f;
  }
  out[hrow * HD + d] = L > 0.f ? f2bf(a / L) : (u16)0;
}

template <int HD, int G, bool FP8>
void launch_decode(const void* q, const void* k_pages, const void* v_pages,
                   const int* block_table, const int* seq_lens, void* out,
                   float* po, float* pm, float* pl, int B, int Hkv,
                   int num_pages, int max_blocks, int page_shift,
                   int num_splits, float qscale, const float* k_scale,
                   const float* v_scale, hipStream_t stream) {
  typedef typename KV8<FP8>::elem elem;
  const unsigned grid = (unsigned)B * Hkv * num_splits;
  hipLaunchKernelGGL((paged_attn_decode_kernel<HD, G, FP8>), dim3(grid),
                     dim3(PA_THREADS), 0, stream, (const u16*)q,
                     (const elem*)k_pages, (const elem*)v_pages, block_table,
                     seq_lens, (u16*)out, po, pm, pl, Hkv, num_pages,
                     max_blocks, page_shift, num_splits, qscale, k_scale,
                     v_scale);
}

}  // namespace

extern "C" {

void kt_paged_kv_write(const void* k_new, const void* v_new, void* k_pages,
                       void* v_pages, const void* slot_mapping, long T,
                       int Hkv, int hd, int page_size, long num_pages,
                       long k_st, long k_sh, long v_st, long v_sh,
                       hipStream_t stream) {
  const long total = T * Hkv * (hd / 8);
  if (total == 0) return;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(paged_kv_write_kernel, dim3((unsigned)blocks), dim3(256),
                     0, stream, (const u16*)k_new, (const u16*)v_new,
                     (u16*)k_pages, (u16*)v_pages, (const int*)slot_mapping,
                     total, Hkv, hd, page_size, num_pages * page_size, k_st,
                     k_sh, v_st, v_sh);
}

// bf16 k_new / v_new rows into e4m3 pools; k_inv / v_inv [Hkv] fp32 device
// arrays hold 1/scale per kv head.
void kt_paged_kv_write_fp8(const void* k_new, const void* v_new,
                           void* k_pages, void* v_pages,
                           const void* slot_mapping, const void* k_inv,
                           const void* v_inv, long T, int Hkv, int hd,
                           int page_size, long num_pages, long k_st,
                           long k_sh, long v_st, long v_sh,
                           hipStream_t stream) {
  const long total = T * Hkv * (hd / 8);
  if (total == 0) return;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(paged_kv_write_fp8_kernel, dim3((unsigned)blocks),
                     dim3(256), 0, stream, (const u16*)k_new,
                     (const u16*)v_new, (unsigned char*)k_pages,
                     (unsigned char*)v_pages, (const int*)slot_mapping,
                     (const float*)k_inv, (const float*)v_inv, total, Hkv, hd,
                     page_size, num_pages * page_size, k_st, k_sh, v_st, v_sh);
}

// Returns 0, or -1 for a configuration with no instantiation (the binding
// checks the same set first and reports it). fp8 != 0: the pools are e4m3
// and k_scale / v_scale are [Hkv] fp32 device arrays; otherwise bf16 pools,
// and the scales are not read.
int kt_paged_attention_decode(const void* q, const void* k_pages,
                              const void* v_pages, const void* block_table,
                              const void* seq_lens, void* out, void* po,
                              void* pm, void* pl, int B, int Hq, int Hkv,
                              int hd, int page_size, int num_pages,
                              int max_blocks, int num_splits, float scale,
                              int fp8, const void* k_scale,
                              const void* v_scale, hipStream_t stream) {
  const int G = Hq / Hkv;
  int page_shift = 0;
  while ((1 << page_shift) < page_size) ++page_shift;
  const float qscale = scale * 1.4426950408889634f;
#define KT_PA_LAUNCH(HD_, G_, FP8_)                                        \
  launch_decode<HD_, G_, FP8_>(                                            \
      q, k_pages, v_pages, (const int*)block_table, (const int*)seq_lens,  \
      out, (float*)po, (float*)pm, (float*)pl, B, Hkv, num_pages,          \
      max_blocks, page_shift, num_splits, qscale, (const float*)k_scale,   \
      (const float*)v_scale, stream)
#define KT_PA_CASE(HD_, G_)           \
  if (hd == HD_ && G == G_) {         \
    if (fp8)                          \
      KT_PA_LAUNCH(HD_, G_, true);    \
    else                              \
      KT_PA_LAUNCH(HD_, G_, false);   \
  } else
  KT_PA_CASE(64, 1)
  KT_PA_CASE(64, 2)
  KT_PA_CASE(64, 4)
  KT_PA_CASE(64, 8)
  KT_PA_CASE(128, 1)
  KT_PA_CASE(128, 2)
  KT_PA_CASE(128, 4)
  KT_PA_CASE(128, 8)
  return -1;
#undef KT_PA_CASE
#undef KT_PA_LAUNCH
  if (num_splits > 1)
    hipLaunchKernelGGL(paged_attn_combine_kernel, dim3((unsigned)B * Hq),
                       dim3(hd), 0, stream, (const float*)po,
                       (const float*)pm, (const float*)pl, (u16*)out, hd,
                       num_splits);
  return 0;
}

}  // extern "C"
