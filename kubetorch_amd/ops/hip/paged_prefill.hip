// Paged prefill attention (gfx950 / CDNA4): causal GQA attention of a packed,
// variable-length batch of query tokens over the block-table KV pools of
// paged_attention.hip. Row b owns query tokens cu[b] .. cu[b+1]-1; with
// ctx = seq_lens[b] - qlen, token i sits at position ctx + i and attends
// keys [0, ctx + i] of the row's pages (their K/V are already in the pool).
//
// Structure, per workgroup (4 waves) = (query tile, kv head, row):
//  - The G = Hq/Hkv query heads of the kv head are stacked with the query
//    tokens into 128 "M rows" (m = token*G + g, 128/G tokens); each wave
//    owns 32 of them. A 64-key K/V tile is staged once in LDS through the
//    block table (16 B loads, next tile prefetched into registers during the
//    current tile's math) and serves all 128 M rows.
//  - S^T = K Q^T on mfma_f32_32x32x16_bf16: A = K rows from LDS
//    (ds_read_b128), B = Q, held in registers for the whole kernel. The
//    accumulator has the M row on the lane and the key in the registers, so
//    the online softmax (fp32, exp2 domain, scale*log2(e) applied to the fp32
//    scores) is lane-local up to one exchange with lane^32, and P^T, rounded
//    to bf16, is directly the B operand of O^T = V^T P^T. V^T fragments come
//    from the row-major V tile with ds_read_b64_tr_b16.
//  - m, l and O stay in fp32; l is summed from the unrounded p.
//  - Key tiles above the workgroup's causal horizon are never visited, and
//    a wave skips tiles above its own horizon; only diagonal tiles, tiles
//    with a key that was not loaded and waves with a token-less lane apply
//    the mask. No atomics, no split-KV: deterministic.
//
// Safety: a key at or beyond the workgroup's horizon (<= seq_lens[b] and
// <= max_blocks*page_size) or behind a table entry outside [0, num_pages) is
// not loaded: its LDS rows are zeros and its score is masked to -inf by a
// per-tile validity mask. A row with more query tokens than seq_lens[b],
// query tokens at a position >= max_blocks*page_size and tokens with a
// packed index outside [0, T) are not computed and not written (the binding
// zero-fills out). All index math on device-side int32 inputs is done in
// 64 bits. The host passes scale > 0 (the row max is taken before scaling).
//
// fp8 pools (template parameter FP8; OCP e4m3 bytes, static fp32 scales per
// kv head as in paged_attention.hip) differ at staging only: a thread loads
// 16 B = 16 elements of one key row, keeps the raw bytes in the prefetch
// registers, and converts to bf16 (exact) when it writes the same Ks / Vs
// tiles. k_scale folds into the score scale, v_scale into the epilogue's
// 1/l.
//
// No torch headers here; bindings.cpp declares the extern "C" launcher.

#include <hip/hip_runtime.h>

typedef unsigned short u16;
typedef ushort vec8u __attribute__((ext_vector_type(8)));
typedef unsigned int vec4w __attribute__((ext_vector_type(4)));
typedef float vec2f __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define PP_THREADS 256
#define PP_MROWS 128  // M rows (query token x group head) per workgroup
#define PP_KT 64      // keys per tile

namespace {

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// One 16 B chunk of a K/V row as it is loaded from the pool and held in the
// prefetch registers: 8 bf16 or 16 e4m3 bytes. to_lds writes it to the bf16
// LDS tile at `dst` (16 B aligned).
template <bool FP8>
struct Chunk {
  typedef u16 elem;
  typedef vec8u vec;
  static constexpr int N = 8;  // elements
  static __device__ __forceinline__ void to_lds(u16* dst, vec v) {
    *reinterpret_cast<vec8u*>(dst) = v;
  }
};
template <>
struct Chunk<true> {
  typedef unsigned char elem;
  typedef vec4w vec;
  static constexpr int N = 16;
  // e4m3 -> fp32 has at most 3 mantissa bits, so its high half is the
  // exact bf16
  static __device__ __forceinline__ unsigned bf16_pair(vec2f f) {
    return (__float_as_uint(f[0]) >> 16) |
           (__float_as_uint(f[1]) & 0xffff0000u);
  }
  static __device__ __forceinline__ void to_lds(u16* dst, vec v) {
    vec4w o[2];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      o[w >> 1][2 * (w & 1)] =
          bf16_pair(__builtin_amdgcn_cvt_pk_f32_fp8(v[w], false));
      o[w >> 1][2 * (w & 1) + 1] =
          bf16_pair(__builtin_amdgcn_cvt_pk_f32_fp8(v[w], true));
    }
    *reinterpret_cast<vec4w*>(dst) = o[0];
    *reinterpret_cast<vec4w*>(dst + 8) = o[1];
  }
};

template <int HD, int G, bool FP8>
__global__ __launch_bounds__(PP_THREADS, 2) void paged_prefill_kernel(
    const u16* __restrict__ q,
    const typename Chunk<FP8>::elem* __restrict__ k_pages,
    const typename Chunk<FP8>::elem* __restrict__ v_pages,
    const int* __restrict__ block_table, const int* __restrict__ cu_q_lens,
    const int* __restrict__ seq_lens, u16* __restrict__ out, long T,
    long q_st, long q_sh, int Hkv, int num_pages, int max_blocks,
    int page_shift, float qscale, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale) {
  typedef typename Chunk<FP8>::vec cvec;
  constexpr int CE = Chunk<FP8>::N;      // elements per 16 B chunk
  constexpr int TQ = PP_MROWS / G;       // query tokens per workgroup
  constexpr int TW = 32 / G;             // query tokens per wave
  constexpr int LDK = HD + 8;            // LDS row stride (elements), 16 B pad
  constexpr int CPR = HD / CE;           // 16 B chunks per K/V row
  constexpr int NLD = PP_KT * CPR / PP_THREADS;  // chunks per thread and tile
  constexpr int KS = HD / 16;            // k-steps of S^T = K Q^T
  constexpr int DB = HD / 32;            // 32-row blocks of O^T

  __shared__ __attribute__((aligned(16))) u16 Ks[PP_KT * LDK];
  __shared__ __attribute__((aligned(16))) u16 Vs[PP_KT * LDK];
  __shared__ unsigned s_valid[2];  // bit k: key k of the tile was loaded

  const int b = blockIdx.z;
  const int kvh = blockIdx.y;
  const long tq0 = (long)blockIdx.x * TQ;
  const long c0 = cu_q_lens[b];
  const long qlen = (long)cu_q_lens[b + 1] - c0;
  if (tq0 >= qlen) return;  // block-uniform, before any barrier
  const long ctx = (long)seq_lens[b] - qlen;
  if (ctx < 0) return;  // more query tokens than the row holds: zero row
  const long cap = (long)max_blocks << page_shift;  // host: fits int32
  // workgroup horizon: one past the last key any of its tokens may attend
  long hi = ctx + (qlen < tq0 + TQ ? qlen : tq0 + TQ);
  hi = hi > cap ? cap : hi;
  if (hi <= 0) return;
  const int n_hi = (int)hi;
  const int ntiles = (n_hi + PP_KT - 1) / PP_KT;
  if (FP8) qscale *= k_scale[kvh];  // scores come from the raw K bytes

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;  // MFMA row/column index of this lane
  const int h = lane >> 5;  // lane half

  // wave horizon (wave-uniform)
  const long wq0 = tq0 + (long)wave * TW;
  long whi_l = wq0 >= qlen ? 0 : ctx + (qlen < wq0 + TW ? qlen : wq0 + TW);
  whi_l = whi_l > cap ? cap : whi_l;
  const int whi = whi_l < 0 ? 0 : (int)whi_l;

  // this lane's M row: query token and head
  const int mrow = wave * 32 + r;
  const long tq = tq0 + mrow / G;
  const int head = kvh * G + mrow % G;
  const long pos_l = ctx + tq;
  const long tok = c0 + tq;
  const bool colok =
      tq < qlen && pos_l >= 0 && pos_l < cap && tok >= 0 && tok < T;
  const int pos = colok ? (int)pos_l : -1;
  // wave-uniform: every lane has a token; the wave's first token's position
  const bool wave_full = __builtin_amdgcn_ballot_w64(colok) == ~0ull;
  const long wmin_l = ctx + wq0;
  const int wmin = wmin_l > cap ? (int)cap : (int)wmin_l;

  // Q as the B operand of S^T = K Q^T: B[k = 8h + j][col r], k-step s
  bf16x8 qf[KS];
  {
    const u16* qp = q + (colok ? tok * q_st + head * q_sh : 0) + 8 * h;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      vec8u v = (vec8u)0;
      if (colok) v = *reinterpret_cast<const vec8u*>(qp + 16 * s);
      qf[s] = __builtin_bit_cast(bf16x8, v);
    }
  }

  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.f;
  float m = -INFINITY, l = 0.f;  // l: this lane half's part of the row sum

  const int* bt = block_table + (size_t)b * max_blocks;
  const int page_size = 1 << page_shift;
  const size_t page_stride = (size_t)Hkv << page_shift;  // rows per page

  // staging registers for one tile; chunk c = tid + u*256 is 16 B number
  // c % CPR of key c / CPR
  cvec kreg[NLD], vreg[NLD];
  bool kvalid = false;  // wave 0: key `lane` of the staged tile was loaded
  auto fetch = [&](int kt) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int c = tid + u * PP_THREADS;
      const int key = c / CPR, part = c % CPR;
      const int t = kt * PP_KT + key;
      int pg = -1;
      if (t < n_hi) pg = bt[t >> page_shift];  // t < cap: inside the row
      kreg[u] = (cvec)0;
      vreg[u] = (cvec)0;
      if (pg >= 0 && pg < num_pages) {
        const size_t row = (size_t)pg * page_stride +
                           ((size_t)kvh << page_shift) + (t & (page_size - 1));
        kreg[u] =
            *reinterpret_cast<const cvec*>(k_pages + row * HD + part * CE);
        vreg[u] =
            *reinterpret_cast<const cvec*>(v_pages + row * HD + part * CE);
      }
    }
    if (wave == 0) {
      const int t = kt * PP_KT + lane;
      int pg = -1;
      if (t < n_hi) pg = bt[t >> page_shift];
      kvalid = pg >= 0 && pg < num_pages;
    }
  };

  fetch(0);
  for (int kt = 0; kt < ntiles; ++kt) {  // block-uniform trip count
    __syncthreads();  // the previous tile's LDS reads are done
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int c = tid + u * PP_THREADS;
      const int key = c / CPR, part = c % CPR;
      Chunk<FP8>::to_lds(&Ks[key * LDK + part * CE], kreg[u]);
      Chunk<FP8>::to_lds(&Vs[key * LDK + part * CE], vreg[u]);
    }
    if (wave == 0) {
      const unsigned long long bal = __ballot(kvalid);
      if (lane == 0) {
        s_valid[0] = (unsigned)bal;
        s_valid[1] = (unsigned)(bal >> 32);
      }
    }
    __syncthreads();
    if (kt + 1 < ntiles) fetch(kt + 1);
    if (kt * PP_KT >= whi) continue;  // wave-uniform: above this wave's horizon

    // S^T tile: 2 blocks of 32 keys x 32 M rows; key on the registers
    f32x16 sacc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &Ks[(kb * 32 + r) * LDK + 16 * s + 8 * h]);
        sacc[kb] =
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], sacc[kb], 0, 0, 0);
      }
    }
    // Register i of block kb holds key kb*32 + (i&3) + 8*(i>>2) + 4h. Only
    // tiles that reach past the wave's first token (the diagonal), hold a
    // key that was not loaded, or meet a lane without a token need masking.
    const unsigned v0 = __builtin_amdgcn_readfirstlane(s_valid[0]);
    const unsigned v1 = __builtin_amdgcn_readfirstlane(s_valid[1]);
    if (!wave_full || kt * PP_KT + PP_KT - 1 > wmin || (v0 & v1) != ~0u) {
      const unsigned vm0 = v0 >> (4 * h);
      const unsigned vm1 = v1 >> (4 * h);
      const int lim = pos - kt * PP_KT - 4 * h;  // causal: key offset <= lim
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int off = (i & 3) + 8 * (i >> 2);
          const bool ok =
              kb * 32 + off <= lim && (((kb ? vm1 : vm0) >> off) & 1u);
          sacc[kb][i] = ok ? sacc[kb][i] : -INFINITY;
        }
      }
    }
    // qscale = scale*log2(e) > 0 is applied to the fp32 scores: to the row
    // max here, to each score inside the exp2 argument's fma below
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * qscale;
    const float mnew = fmaxf(m, mx);
    // mnew == -inf: this M row has seen no key yet; o and l are 0 and stay 0
    const float msafe = mnew == -INFINITY ? 0.f : mnew;
    const float alpha = __builtin_amdgcn_exp2f(m - msafe);
    m = mnew;
    float psum = 0.f;
    bf16x8 pf[2][2];  // P^T as the B operand: k-step s = registers 8s..8s+7
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p =
            __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], qscale, -msafe));
        psum += p;
        pf[kb][i >> 3][i & 7] = (__bf16)p;
      }
    }
    l = l * alpha + psum;
    if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {  // wave-uniform
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[d][i] *= alpha;
    }

    // O^T += V^T P^T. A = V^T: lane (r, h), element j of k-step s is
    // V[key 16s + 8(j>>2) + 4h + (j&3)][d = 32*db + r]: two transposed
    // reads of 4 keys x 16 columns per 16-lane group. Lane 4q+p of a group
    // supplies the address of key row q, columns 4p..4p+3.
    const int li = lane & 15;
    const int tr_row = 4 * h + (li >> 2);
    const int tr_col = 16 * ((lane >> 4) & 1) + 4 * (li & 3);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          const u16* p0 =
              &Vs[(kb * 32 + 16 * s + tr_row) * LDK + 32 * d + tr_col];
          const bf16x4 lo =
              __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p0);
          const bf16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(p0 + 8 * LDK));
          bf16x8 a;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            a[j] = lo[j];
            a[4 + j] = hi4[j];
          }
          o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pf[kb][s], o[d], 0,
                                                        0, 0);
        }
      }
    }
  }

  const float lt = l + __shfl_xor(l, 32, 64);
  if (!colok || !(lt > 0.f)) return;  // out is zero-filled by the binding
  const float inv = (FP8 ? v_scale[kvh] : 1.f) / lt;
  const size_t Hq = (size_t)Hkv * G;
  u16* op = out + ((size_t)tok * Hq + head) * HD + 4 * h;
  // registers 4g..4g+3 of block d are O[d*32 + 8g + 4h .. +3]: 8 B stores
#pragma unroll
  for (int d = 0; d < DB; ++d) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = (__bf16)(o[d][4 * g4 + e] * inv);
      *reinterpret_cast<bf16x4*>(op + 32 * d + 8 * g4) = w;
    }
  }
}

template <int HD, int G, bool FP8>
void launch_prefill(const void* q, const void* k_pages, const void* v_pages,
                    const int* block_table, const int* cu_q_lens,
                    const int* seq_lens, void* out, long T, long q_st,
                    long q_sh, int B, int Hkv, int num_pages, int max_blocks,
                    int page_shift, int max_q_len, float qscale,
                    const float* k_scale, const float* v_scale,
                    hipStream_t stream) {
  typedef typename Chunk<FP8>::elem elem;
  constexpr int TQ = PP_MROWS / G;
  const dim3 grid((unsigned)((max_q_len + TQ - 1) / TQ), (unsigned)Hkv,
                  (unsigned)B);
  hipLaunchKernelGGL((paged_prefill_kernel<HD, G, FP8>), grid,
                     dim3(PP_THREADS), 0, stream, (const u16*)q,
                     (const elem*)k_pages, (const elem*)v_pages, block_table,
                     cu_q_lens, seq_lens, (u16*)out, T, q_st, q_sh, Hkv,
                     num_pages, max_blocks, page_shift, qscale, k_scale,
                     v_scale);
}

}  // namespace

extern "C" {

// Returns 0, or -1 for a configuration with no instantiation (the binding
// checks the same set first and reports it). q rows may be strided (q_st,
// q_sh in elements); out is [T, Hq, hd] contiguous and zero-filled. fp8 != 0:
// the pools are e4m3 and k_scale / v_scale are [Hkv] fp32 device arrays;
// otherwise bf16 pools, and the scales are not read.
int kt_paged_attention_prefill(const void* q, const void* k_pages,
                               const void* v_pages, const void* block_table,
                               const void* cu_q_lens, const void* seq_lens,
                               void* out, long T, long q_st, long q_sh, int B,
                               int Hq, int Hkv, int hd, int page_size,
                               int num_pages, int max_blocks, int max_q_len,
                               float scale, int fp8, const void* k_scale,
                               const void* v_scale, hipStream_t stream) {
  const int G = Hq / Hkv;
  int page_shift = 0;
  while ((1 << page_shift) < page_size) ++page_shift;
  const float qscale = scale * 1.4426950408889634f;
#define KT_PP_LAUNCH(HD_, G_, FP8_)                                         \
  launch_prefill<HD_, G_, FP8_>(                                            \
      q, k_pages, v_pages, (const int*)block_table, (const int*)cu_q_lens,  \
      (const int*)seq_lens, out, T, q_st, q_sh, B, Hkv, num_pages,          \
      max_blocks, page_shift, max_q_len, qscale, (const float*)k_scale,     \
      (const float*)v_scale, stream)
#define KT_PP_CASE(HD_, G_)           \
  if (hd == HD_ && G == G_) {         \
    if (fp8)                          \
      KT_PP_LAUNCH(HD_, G_, true);    \
    else                              \
      KT_PP_LAUNCH(HD_, G_, false);   \
    return 0;                         \
  }
  KT_PP_CASE(64, 1)
  KT_PP_CASE(64, 2)
  KT_PP_CASE(64, 4)
  KT_PP_CASE(64, 8)
  KT_PP_CASE(128, 1)
  KT_PP_CASE(128, 2)
  KT_PP_CASE(128, 4)
  KT_PP_CASE(128, 8)
#undef KT_PP_CASE
#undef KT_PP_LAUNCH
  return -1;
}

}  // extern "C"
