// Routed expert MLP for decode (gfx950 / CDNA4): top-k routing, the experts'
// gate/up GEMM with a fused SwiGLU, the down GEMM and the top-k combine, for
// 1 <= T <= 32 tokens of bf16 x. Four launches, no atomics, no host sync:
//
//   moe_route           router logits [T, E] -> sel [T, k], weights [T, k]
//                       and the routing table expert_count [E],
//                       expert_rows [E, 32]
//   moe_gemm<true>      h[t, j, :]  = bf16(silu(x_t Wg_e^T) * (x_t Wu_e^T))
//   moe_gemm<false>     part[s, t, j, :] = w[t, j] * (h[t, j, Ks] Wd_e[:, Ks]^T)
//   moe_combine         out[t, :] = bf16(sum_s sum_j part[s, t, j, :])
//
// with e = sel[t, j]. A pair p = t * k + j names a (token, k-slot); h and the
// partials are indexed by it, and expert_rows[e] lists the pairs routed to
// expert e in token order.
//
// The two GEMMs are one kernel template. Per workgroup (4 waves) = (128
// output columns, expert, K slice):
//  - expert_count[e] == 0 returns before the first weight load: an expert
//    nobody picked costs no HBM traffic and its weights cannot reach the
//    output.
//  - Each token picks an expert at most once, so an expert has at most T <= 32
//    rows: one 32-row MFMA tile. The rows are gathered through the table into
//    an LDS image shared by the four waves, in chunks of four steps (256 or
//    512 k), double buffered, one barrier per chunk. Rows past the count are zeros and are
//    never loaded (a raw buffer load past its resource returns zeros without
//    a memory request).
//  - A wave owns 32 output columns = 32 weight rows. Lane (r, h) streams row
//    n0 + r: a 16 B load is 8 consecutive k, which is the lane's B fragment
//    of one mfma_f32_32x32x16_bf16 (k = 16 s + 8 h + j), so weights need no
//    permutation, go straight to VGPRs and never touch LDS. A step is 8 such
//    loads per lane: 64 k of the gate row and of the up row (two
//    accumulators), or 128 k of the down row. Three steps (24 loads per
//    lane) are in flight ahead of the one in use.
//  - The accumulator has the output column on the lane and the tile row in
//    the registers, so SwiGLU and the routing weight are lane-local.
//  - Only the down GEMM splits K (blockIdx.z): a split gate/up GEMM could not
//    apply SwiGLU in its epilogue. The split factor comes from the shapes
//    alone (kt_moe_down_plan), the partials are written with plain stores
//    and summed in index order: bit-identical run to run, and a token's
//    result does not depend on the batch it is computed in.
//
// FP8 expert weights (W8A16): the same template with a byte weight type.
// w_gate_up and w_down are OCP e4m3 with one power-of-two fp32 scale per
// expert and weight row; the work split, the early exit, the LDS image and
// the epilogue's layout are those above. What changes is the data path:
//  - A 16 B load is 16 consecutive k of the lane's row: its low 8 bytes are
//    the B fragment of one k-step and its high 8 bytes that of the next
//    (v_cvt_pk_f32_fp8 and the high half of each fp32: exact), so inside a
//    128-k tile k-step 2u + e holds, on lane half h, element j:
//        k = 32 u + 16 h + 8 e + j,
//    and the A fragments are read from the LDS image with that permutation.
//    The four loads of a tile are one 128 B line of the row.
//  - A step is still 8 loads per lane, now 128 k of the gate and up rows or
//    256 k of the down row, and the LDS chunks are 256 k for both (one
//    barrier per 256 k, 33,920 B). The unpacked fragments cost registers the
//    bf16 kernel does not need: gate/up keeps two steps (16 loads per lane)
//    ahead of the one in use, down three (24, as bf16).
//  - The down GEMM's K slices are counted in 128-k tiles for both weight
//    types, so kt_moe_down_plan means the same; a 256-k step whose second
//    tile lies past the slice loads zeros for it.
//  - The scale multiplies the fp32 accumulator once in the epilogue (exact):
//    gate and up before SwiGLU, down before the routing weight.
//
// Safety: every load of x, h and the weights goes through a buffer resource
// of the operand's exact size. Table entries are device data: a count is
// clamped to 32 and a pair outside [0, T k) is treated as an empty row, so
// no store leaves h or the partials. Every index that scales with E * N * K
// is 64-bit.
//
// No torch headers here; kt_launchers.h declares the extern "C" launchers.

#include <hip/hip_runtime.h>

#include "kt_launchers.h"
#include "moe_common.h"

#define MOE_THREADS 256
#define MOE_BN 128                  // output columns per workgroup
#define MOE_ROWS 32                 // rows of an expert's tile (max T)

namespace {

// ---------------------------------------------------------------------------
// Routing
// ---------------------------------------------------------------------------

// One workgroup. Pass 1, a wave per token and a lane per expert: rank the
// logits (descending, equal logits lowest index first, NaN as -inf), write
// the k best and their softmax (moe_route_token, shared with the grouped
// kernels). Pass 2, a wave per expert and a lane per token: a ballot of the
// tokens that picked the expert gives its count and, by prefix count, each
// pair's row in token order.
__global__ __launch_bounds__(MOE_THREADS) void moe_route_kernel(
    const void* __restrict__ logits, int is_bf16, int* __restrict__ sel,
    float* __restrict__ weights, int* __restrict__ expert_count,
    int* __restrict__ expert_rows, int T, int E, int top_k) {
  __shared__ signed char slot_of[MOE_ROWS][MOE_MAX_E];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  for (int t = wave; t < T; t += MOE_THREADS / 64) {  // wave-uniform
    const int slot =
        moe_route_token(logits, is_bf16, t, E, top_k, lane, sel, weights);
    if (lane < E) slot_of[t][lane] = (signed char)slot;
  }
  __syncthreads();

  for (int e = wave; e < E; e += MOE_THREADS / 64) {
    const int s = lane < T ? (int)slot_of[lane][e] : -1;
    const unsigned long long mask = __ballot(s >= 0);
    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
    if (s >= 0) expert_rows[e * MOE_ROWS + pos] = lane * top_k + s;
    if (lane == 0) expert_count[e] = __popcll(mask);
  }
}

// ---------------------------------------------------------------------------
// The routed GEMMs
// ---------------------------------------------------------------------------

struct WStep {
  vec4w v[8];
};

// The raw buffer loads (buf_load, MOE_OOB) are moe_common.h's.
//
// GU: a = x [a_rows, K] (row stride a_stride), w = w_gate_up [E, 2N, K],
//     writes h [npairs, N].
// !GU: a = h [npairs, K], w = w_down [E, N, K], writes part [S, npairs, N]
//     scaled by route_w [npairs].
// WT is the weight element: u16 (bf16) or unsigned char (e4m3, with one fp32
// scale per weight row in w_scale [E, 2N] or [E, N], applied in the
// epilogue). The K split is counted in units: a step, or for the e4m3 down
// GEMM a 128-k tile (half a step), so both weight types split alike.
template <bool GU, typename WT>
__global__ __launch_bounds__(MOE_THREADS, 2) void moe_gemm_kernel(
    const u16* __restrict__ a, long a_stride, int a_rows,
    const WT* __restrict__ w, const float* __restrict__ w_scale,
    const int* __restrict__ expert_count,
    const int* __restrict__ expert_rows, const float* __restrict__ route_w,
    u16* __restrict__ hout, float* __restrict__ part, int top_k, int N, int K,
    int npairs, int units_per_split) {
  constexpr bool W8 = sizeof(WT) == 1;
  constexpr int ES = (int)sizeof(WT);
  constexpr int NU = GU ? 4 : 8;      // 16 B loads per weight row and step
  constexpr int KS = NU * 32 / ES;    // k per step: 64 / 128, e4m3 128 / 256
  constexpr int UK = GU ? KS : 128;   // k per unit of the K split
  // Steps in the register ring (one in use, the others in flight), steps per
  // LDS chunk of the A rows and chunks per loop iteration: the unrolled
  // iteration is whole turns of the ring, so no register is copied.
  constexpr int R = W8 && GU ? 3 : 4;
  constexpr int SPC = W8 ? (GU ? 2 : 1) : 4;
  constexpr int CPI = W8 ? (GU ? 3 : 4) : 1;
  static_assert(CPI * SPC % R == 0, "an iteration is whole turns of the ring");
  constexpr int CK = SPC * KS;        // k per chunk
  constexpr int LDA = CK * 2 + 16;    // LDS row stride in bytes, 16 B pad
  constexpr int PP = CK / 8;          // 16 B pieces per row
  constexpr int RP = MOE_THREADS / PP;  // rows per staging pass
  constexpr int NI = MOE_ROWS / RP;     // staging passes
  __shared__ __attribute__((aligned(16))) unsigned char as[2 * MOE_ROWS * LDA];
  __shared__ int pair_s[MOE_ROWS];

  const int e = blockIdx.y;
  int count = expert_count[e];
  if (count <= 0) return;  // block-uniform, before the first weight load
  count = count > MOE_ROWS ? MOE_ROWS : count;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31;  // MFMA row/column index of this lane
  const int h = lane >> 5;  // lane half

  if (tid < MOE_ROWS) {
    int p = tid < count ? expert_rows[e * MOE_ROWS + tid] : -1;
    if (p < 0 || p >= npairs) p = -1;
    pair_s[tid] = p;
  }
  __syncthreads();

  // this workgroup's K slice, in units and in steps (block-uniform)
  const int t0 = (int)blockIdx.z * units_per_split;
  int nt = K / UK - t0;
  nt = nt > units_per_split ? units_per_split : nt;
  nt = nt < 0 ? 0 : nt;
  const long k0 = (long)(nt > 0 ? t0 : 0) * UK;  // inside the row
  const int klen = nt * UK;
  if constexpr (UK != KS) nt = (klen + KS - 1) / KS;  // units -> steps
  const int nchunks = (nt + SPC - 1) / SPC;

  // The wave's 32 weight rows from column k0 on as one resource (N is a
  // multiple of 128: every row exists). For gate/up a second resource holds
  // the 32 up rows, N rows further on.
  const long rows_e = GU ? 2L * N : (long)N;
  const long n0 = (long)blockIdx.x * MOE_BN + wave * 32;  // wave-uniform
  const WT* wb = w + ((size_t)e * rows_e + n0) * K + k0;
  const int wbytes = (int)((31L * K + (K - k0)) * ES);
  const rsrc_t wrs0 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<WT*>(wb), 0, wbytes, MOE_RSRC_FLAGS);
  const rsrc_t wrs1 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<WT*>(GU ? wb + (size_t)N * K : wb), 0, wbytes,
      MOE_RSRC_FLAGS);
  const unsigned woff = (unsigned)(r * (long)K * ES) + 16 * h;
  auto wstep = [&](int t) {  // step t of the slice, zeros past its end
    WStep o;
    if constexpr (W8 && !GU) {
      // two 128 B lines of the row; the slice may end after the first
      const unsigned off0 =
          t * KS < klen ? woff + (unsigned)t * KS : MOE_OOB;
      const unsigned off1 =
          t * KS + 128 < klen ? woff + (unsigned)t * KS + 128 : MOE_OOB;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        o.v[u] = buf_load(wrs0, off0 + 32 * u);
        o.v[4 + u] = buf_load(wrs0, off1 + 32 * u);
      }
    } else {
      const unsigned off =
          t < nt ? woff + (unsigned)t * (KS * ES) : MOE_OOB;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        o.v[u] = buf_load(wrs0, off + 32 * u);
        if constexpr (GU) o.v[4 + u] = buf_load(wrs1, off + 32 * u);
      }
    }
    return o;
  };

  // A staging: thread -> 16 B piece p of rows row0 + RP * i of a chunk,
  // gathered through the table. The resource is the whole operand; empty
  // rows and pieces past the slice come back as zeros.
  const int p = tid % PP;
  const int row0 = tid / PP;
  const rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(a), 0, (int)(((long)(a_rows - 1) * a_stride + K) * 2),
      MOE_RSRC_FLAGS);
  unsigned abase[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int pr = pair_s[row0 + RP * i];
    const long src = GU ? pr / top_k : pr;  // x row of the token, or h row
    abase[i] = pr >= 0 && src < a_rows
                   ? (unsigned)((src * a_stride + k0 + p * 8) * 2)
                   : MOE_OOB;
  }
  vec4w ar[NI];
  auto afetch = [&](int c) {
    const bool kok = c * CK + p * 8 < klen;  // the piece is in the slice
#pragma unroll
    for (int i = 0; i < NI; ++i)
      ar[i] = buf_load(ars, kok && abase[i] != MOE_OOB
                                ? abase[i] + (unsigned)c * (CK * 2)
                                : MOE_OOB);
  };
  auto awrite = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      *reinterpret_cast<vec4w*>(
          &as[(buf * MOE_ROWS + row0 + RP * i) * LDA + p * 16]) = ar[i];
  };

  // the row scales of this lane's output column (e4m3 weights only)
  float sc0 = 1.f, sc1 = 1.f;
  if constexpr (W8) {
    const float* sc = w_scale + (size_t)e * rows_e + n0 + r;
    sc0 = sc[0];
    if constexpr (GU) sc1 = sc[N];
  }

  f32x16 acc0, acc1;  // gate and up, or acc0 alone
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;

  // weight ring: wr[0] is the step in use, the others are in flight
  afetch(0);
  WStep wr[R];
#pragma unroll
  for (int i = 0; i < R; ++i) wr[i] = wstep(i);
  awrite(0);
  __syncthreads();

  // Every chunk runs all of its steps, and every iteration all of its
  // chunks: a step past the slice multiplies the zeros awrite left by the
  // zeros wstep returned.
  for (int c = 0; c < nchunks; c += CPI) {  // block-uniform trip count
#pragma unroll
    for (int ci = 0; ci < CPI; ++ci) {
      const int cc = c + ci;
      afetch(cc + 1);
      // bf16: k-step u of a step is k = 16 u + 8 h + j. e4m3: a 16 B load is
      // two k-steps, so k-step 2u + e is k = 32 u + 16 h + 8 e + j, and the
      // A fragments are read with the same permutation.
      const unsigned char* ab =
          &as[((cc & 1) * MOE_ROWS + r) * LDA + (W8 ? 32 : 16) * h];
#pragma unroll
      for (int tl = 0; tl < SPC; ++tl) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          if constexpr (W8) {
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
                ab + tl * (KS * 2) + 64 * u);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
                ab + tl * (KS * 2) + 64 * u + 16);
            const vec4w g = wr[0].v[u];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a0, frag_fp8(g[0], g[1]), acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a1, frag_fp8(g[2], g[3]), acc0, 0, 0, 0);
            if constexpr (GU) {
              const vec4w v = wr[0].v[4 + u];
              acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  a0, frag_fp8(v[0], v[1]), acc1, 0, 0, 0);
              acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  a1, frag_fp8(v[2], v[3]), acc1, 0, 0, 0);
            }
          } else {
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(
                ab + tl * (KS * 2) + 32 * u);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, frag(wr[0].v[u]),
                                                           acc0, 0, 0, 0);
            if constexpr (GU)
              acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  av, frag(wr[0].v[4 + u]), acc1, 0, 0, 0);
          }
        }
#pragma unroll
        for (int i = 0; i + 1 < R; ++i) wr[i] = wr[i + 1];
        wr[R - 1] = wstep(cc * SPC + tl + R);
      }
      awrite((cc + 1) & 1);
      __syncthreads();
    }
  }

  // register i holds tile row (i & 3) + 8 * (i >> 2) + 4h of column n. The
  // scales are powers of two: applying them to the fp32 sums is exact.
  const long n = n0 + r;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int pr = pair_s[(i & 3) + 8 * (i >> 2) + 4 * h];
    if (pr < 0) continue;
    if constexpr (GU) {
      const float g = acc0[i] * sc0;
      const float s = g / (1.f + expf(-g));
      const __bf16 b = (__bf16)(s * (acc1[i] * sc1));
      hout[(size_t)pr * N + n] = __builtin_bit_cast(u16, b);
    } else {
      part[((size_t)blockIdx.z * npairs + pr) * N + n] =
          acc0[i] * sc0 * route_w[pr];
    }
  }
}

// out[t, d] = bf16(sum over s, then j, of part[s, t, j, d]), in that order.
// Every (s, t, j) slab was written: each pair belongs to one expert's table.
__global__ __launch_bounds__(256) void moe_combine_kernel(
    const float* __restrict__ part, u16* __restrict__ out, int T, int D,
    int top_k, int S) {
  const int D4 = D / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)T * D4) return;
  const int t = (int)(i / D4);
  const int d = (int)(i % D4) * 4;
  float4 acc;
  for (int s = 0; s < S; ++s) {
    for (int j = 0; j < top_k; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(
          part + (((size_t)s * T + t) * top_k + j) * D + d);
      if (s == 0 && j == 0) {
        acc = v;
      } else {
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
    }
  }
  const __bf16 b0 = (__bf16)acc.x, b1 = (__bf16)acc.y, b2 = (__bf16)acc.z,
               b3 = (__bf16)acc.w;
  vec2w o;
  o[0] = (unsigned)__builtin_bit_cast(u16, b0) |
         ((unsigned)__builtin_bit_cast(u16, b1) << 16);
  o[1] = (unsigned)__builtin_bit_cast(u16, b2) |
         ((unsigned)__builtin_bit_cast(u16, b3) << 16);
  *reinterpret_cast<vec2w*>(out + (size_t)t * D + d) = o;
}

// The two routed GEMMs for weights of type WT. The gate/up GEMM takes all of
// K (a step is 64 k of bf16, 128 k of e4m3); the down GEMM's S slices are
// counted in 128-k tiles for both types.
template <typename WT>
void launch_gemms(const void* x, long x_stride, const void* w_gate_up,
                  const void* w_down, const void* gate_up_scale,
                  const void* down_scale, const void* weights,
                  const void* expert_count, const void* expert_rows, void* h,
                  void* part, int T, int D, int I, int E, int top_k, int S,
                  hipStream_t stream) {
  const int np = T * top_k;
  hipLaunchKernelGGL((moe_gemm_kernel<true, WT>),
                     dim3((unsigned)(I / MOE_BN), (unsigned)E, 1),
                     dim3(MOE_THREADS), 0, stream, (const u16*)x, x_stride, T,
                     (const WT*)w_gate_up, (const float*)gate_up_scale,
                     (const int*)expert_count, (const int*)expert_rows,
                     (const float*)nullptr, (u16*)h, (float*)nullptr, top_k, I,
                     D, np, D / (128 / (int)sizeof(WT)));
  const int kt = I / 128;
  hipLaunchKernelGGL((moe_gemm_kernel<false, WT>),
                     dim3((unsigned)(D / MOE_BN), (unsigned)E, (unsigned)S),
                     dim3(MOE_THREADS), 0, stream, (const u16*)h, (long)I, np,
                     (const WT*)w_down, (const float*)down_scale,
                     (const int*)expert_count, (const int*)expert_rows,
                     (const float*)weights, (u16*)nullptr, (float*)part, top_k,
                     D, I, np, (kt + S - 1) / S);
}

}  // namespace

extern "C" {

// The down GEMM's split-K factor. With T = 1 only top_k experts are active,
// so the smallest factor that still gives each of the chip's 256 CUs a
// workgroup is ceil(256 / (D/128 * top_k)); slices of at least four 128-k
// tiles, at most 8 slabs per pair to sum. A function of the shapes alone
// (E does not enter: idle experts' workgroups exit at once).
int kt_moe_down_plan(long D, long I, int E, int top_k) {
  (void)E;
  const long act = (D / MOE_BN) * top_k;
  const long kt = I / 128;
  long s = (256 + act - 1) / act;
  if (s > kt / 4) s = kt / 4;
  if (s > 8) s = 8;
  if (s < 1) s = 1;
  return (int)s;
}

// logits: [T, E] contiguous, bf16 (is_bf16 != 0) or fp32; sel, weights:
// [T, top_k] int32 / fp32; expert_count: [E] int32; expert_rows: [E, 32]
// int32. The binding has checked 1 <= T <= 32, 1 <= top_k <= E <= 64.
void kt_moe_route(const void* logits, int is_bf16, void* sel, void* weights,
                  void* expert_count, void* expert_rows, int T, int E,
                  int top_k, hipStream_t stream) {
  hipLaunchKernelGGL(moe_route_kernel, dim3(1), dim3(MOE_THREADS), 0, stream,
                     logits, is_bf16, (int*)sel, (float*)weights,
                     (int*)expert_count, (int*)expert_rows, T, E, top_k);
}

// x: [T, D] bf16, row stride x_stride elements; w_gate_up: [E, 2I, D] and
// w_down: [E, D, I] contiguous, bf16 or (fp8 != 0) e4m3 with the row scales
// gate_up_scale [E, 2I] and down_scale [E, D] fp32 (not read otherwise);
// weights, expert_count, expert_rows: as kt_moe_route wrote them;
// h: [T, top_k, I] bf16 and part: [S, T, top_k, D] fp32 scratch; out: [T, D]
// bf16. The binding has checked 1 <= T <= 32, D % 128 == I % 128 == 0, both
// <= 2^16, 1 <= S <= 64 and the alignments.
void kt_moe_mlp(const void* x, long x_stride, const void* w_gate_up,
                const void* w_down, const void* weights,
                const void* expert_count, const void* expert_rows, void* h,
                void* part, void* out, int T, int D, int I, int E, int top_k,
                int S, int fp8, const void* gate_up_scale,
                const void* down_scale, hipStream_t stream) {
  if (fp8)
    launch_gemms<unsigned char>(x, x_stride, w_gate_up, w_down, gate_up_scale,
                                down_scale, weights, expert_count, expert_rows,
                                h, part, T, D, I, E, top_k, S, stream);
  else
    launch_gemms<u16>(x, x_stride, w_gate_up, w_down, nullptr, nullptr,
                      weights, expert_count, expert_rows, h, part, T, D, I, E,
                      top_k, S, stream);
  kt_moe_combine(part, out, T, D, top_k, S, stream);
}

// part: [S, T, top_k, D] fp32, every slab written; out: [T, D] bf16.
void kt_moe_combine(const void* part, void* out, int T, int D, int top_k,
                    int S, hipStream_t stream) {
  const long n4 = (long)T * (D / 4);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n4 + 255) / 256)),
                     dim3(256), 0, stream, (const float*)part, (u16*)out, T, D,
                     top_k, S);
}

}  // extern "C"
