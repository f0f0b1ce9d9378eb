// Routed expert MLP for more than 32 tokens (gfx950 / CDNA4): a grouped GEMM
// over the experts' token groups. Five launches, no host sync, grids that are
// functions of the shapes alone:
//
//   moe_route_rows      router logits [T, E] -> sel [T, k], weights [T, k]
//                       (moe.hip's rule, a wave per token, any T)
//   moe_align           counting sort of the pairs p = t * k + j by expert:
//                       expert segments padded to 64 rows in sorted_pairs
//                       (-1 in the padding), one (expert, first row) entry
//                       per 64-row tile and the number of live tiles
//   grouped_gemm<true>  h[row, :] = bf16(silu(x_t Wg_e^T) * (x_t Wu_e^T)),
//                       row = the pair's place in sorted_pairs
//   grouped_gemm<false> part[p, :] = w[p] * (h[row, :] Wd_e^T)
//   moe_combine (moe.hip, S = 1)  out[t, :] = bf16(sum_j part[t k + j, :])
//
// The GEMM, one template for both roles and both weight types. A workgroup
// (4 waves) owns one M tile = 64 sorted rows of one expert by 128 output
// columns; the tile index is the fastest grid dimension, so the workgroups
// that stream the same 128 weight rows of an expert are dispatched together
// and all but the first find them in L2. The worst case ceil(T k / 64) + E
// tiles sizes the grid; a workgroup past the live count returns before its
// first load, and so an expert nobody picked has no tile, costs no weight
// traffic and cannot reach the output.
//  - A wave owns 32 output columns = 32 weight rows and all 64 tile rows
//    (two 32-row MFMA blocks): no other wave of the workgroup needs its
//    weights, so they skip LDS. Lane (r, h) streams row n0 + r: a 16 B load
//    is the lane's B fragment of one mfma_f32_32x32x16_bf16 (two of them for
//    e4m3) and feeds two MFMAs, one per row block; gate and up rows go to two
//    accumulator pairs, so SwiGLU is lane-local. Weights are loaded in chunks
//    of 128 B per row (64 k of bf16, 128 k of e4m3) into a register ring:
//    one chunk in use, two (gate/up) or three (down) in flight.
//  - The 64 A rows are what the waves share. They are staged through LDS in
//    the same chunks, double buffered, rows padded by 16 B, one barrier per
//    chunk. The gate/up GEMM gathers x rows through sorted_pairs; it writes
//    h in sorted order, so the down GEMM's rows are contiguous. Both go
//    through a buffer resource: a padding row and the prefetch past K read
//    zeros without a branch or a memory request.
//  - K is walked once, in order, by one workgroup: no split-K, no atomics on
//    floats. A row's sums depend on nothing but the row, so the result is
//    bit-identical run to run (the order moe_align's integer atomics place
//    the rows in does not matter) and independent of the other tokens.
//  - e4m3 weights stay bytes until the MFMA fragment (frag_fp8: exact); the
//    per-row power-of-two scale multiplies the fp32 sum once in the epilogue,
//    gate and up before SwiGLU, down before the routing weight, as in moe.hip.
//
// Safety: the table is device data. A tile whose expert or first row is out
// of range is skipped, a pair outside [0, T k) is a padding row, and stores
// go to h rows inside the tile and part rows of valid pairs only. Weight,
// h and part addresses are formed in 64 bits; x is one resource below 2 GiB
// (the binding checks its stride).
//
// No torch headers here; kt_launchers.h declares the extern "C" launchers.

#include <hip/hip_runtime.h>

#include "kt_launchers.h"
#include "moe_common.h"

#define MGG_THREADS 256
#define MGG_BM 64    // sorted rows per tile
#define MGG_BN 128   // output columns per workgroup
#define MGG_ALIGN_THREADS 1024

namespace {

__global__ __launch_bounds__(MGG_THREADS) void moe_route_rows_kernel(
    const void* __restrict__ logits, int is_bf16, int* __restrict__ sel,
    float* __restrict__ weights, int T, int E, int top_k) {
  const int t = (int)blockIdx.x * (MGG_THREADS / 64) +
                __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t < T)
    moe_route_token(logits, is_bf16, t, E, top_k, threadIdx.x & 63, sel,
                    weights);
}

// One workgroup. Count the pairs of every expert, lay the experts' segments
// out one after the other, each padded to whole tiles, then place the pairs.
// sum_e ceil(c_e / BM) <= ceil(npairs / BM) + E = max_tiles, so every segment
// lies inside sorted_pairs [max_tiles * BM].
__global__ __launch_bounds__(MGG_ALIGN_THREADS) void moe_align_kernel(
    const int* __restrict__ sel, int npairs, int E, int max_tiles,
    int* __restrict__ expert_count, int* __restrict__ sorted_pairs,
    int* __restrict__ tile_expert, int* __restrict__ tile_row0,
    int* __restrict__ n_tiles) {
  __shared__ int cnt[MOE_MAX_E], placed[MOE_MAX_E], tile0[MOE_MAX_E + 1];
  const int tid = threadIdx.x;
  if (tid < MOE_MAX_E) cnt[tid] = placed[tid] = 0;
  __syncthreads();
  for (int p = tid; p < npairs; p += MGG_ALIGN_THREADS) {
    const int e = sel[p];
    if (e >= 0 && e < E) atomicAdd(&cnt[e], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int nt = 0;
    for (int e = 0; e < E; ++e) {
      tile0[e] = nt;
      nt += (cnt[e] + MGG_BM - 1) / MGG_BM;
    }
    tile0[E] = nt;
    *n_tiles = nt < max_tiles ? nt : max_tiles;
  }
  __syncthreads();
  if (tid < E) {
    expert_count[tid] = cnt[tid];
    for (int i = tile0[tid]; i < tile0[tid + 1] && i < max_tiles; ++i) {
      tile_expert[i] = tid;
      tile_row0[i] = i * MGG_BM;
    }
  }
  for (int p = tid; p < npairs; p += MGG_ALIGN_THREADS) {
    const int e = sel[p];
    if (e < 0 || e >= E) continue;
    const int row = tile0[e] * MGG_BM + atomicAdd(&placed[e], 1);
    if (row < max_tiles * MGG_BM) sorted_pairs[row] = p;
  }
  // the padding of every segment: fewer than BM rows each
  for (int i = tid; i < E * MGG_BM; i += MGG_ALIGN_THREADS) {
    const int e = i / MGG_BM;
    const int row = tile0[e] * MGG_BM + cnt[e] + i % MGG_BM;
    if (row < tile0[e + 1] * MGG_BM && row < max_tiles * MGG_BM)
      sorted_pairs[row] = -1;
  }
}

template <bool GU>
struct WChunk {
  vec4w g[4];
  vec4w u[GU ? 4 : 1];
};

// GU: a = x [a_rows, K] (row stride a_stride), w = w_gate_up [E, 2N, K],
//     writes h [cap_rows, N] in sorted-row order.
// !GU: a = h [cap_rows, K], w = w_down [E, N, K], writes part [npairs, N]
//     scaled by route_w [npairs].
// WT is the weight element: u16 (bf16) or unsigned char (e4m3, with one fp32
// scale per weight row in w_scale [E, 2N] or [E, N]).
template <bool GU, typename WT>
__global__ __launch_bounds__(MGG_THREADS, 2) void moe_grouped_gemm_kernel(
    const u16* __restrict__ a, long a_stride, int a_rows,
    const WT* __restrict__ w, const float* __restrict__ w_scale,
    const int* __restrict__ n_tiles, const int* __restrict__ tile_expert,
    const int* __restrict__ tile_row0, const int* __restrict__ sorted_pairs,
    const float* __restrict__ route_w, u16* __restrict__ hout,
    float* __restrict__ part, int top_k, int N, int K, int E, int npairs,
    int cap_rows) {
  constexpr bool W8 = sizeof(WT) == 1;
  constexpr int ES = (int)sizeof(WT);
  constexpr int CK = 128 / ES;        // k per chunk: 128 B of a weight row
  constexpr int R = GU ? 3 : 4;       // chunks in the weight register ring
  constexpr int LDA = CK * 2 + 16;    // LDS row stride in bytes, 16 B pad
  constexpr int PP = CK / 8;          // 16 B pieces per A row and chunk
  constexpr int RP = MGG_THREADS / PP;  // rows per staging pass
  constexpr int NI = MGG_BM / RP;       // staging passes
  __shared__ __attribute__((aligned(16))) unsigned char as[2 * MGG_BM * LDA];
  __shared__ int pair_s[MGG_BM];

  const int tile = blockIdx.x;
  if (tile >= *n_tiles) return;  // block-uniform, before the first load
  const int e = tile_expert[tile];
  const int row0 = tile_row0[tile];
  if (e < 0 || e >= E || row0 < 0 || row0 > cap_rows - MGG_BM) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31;  // MFMA row/column index of this lane
  const int h = lane >> 5;  // lane half

  if (tid < MGG_BM) {
    int p = sorted_pairs[row0 + tid];
    if (p < 0 || p >= npairs) p = -1;
    pair_s[tid] = p;
  }
  __syncthreads();

  const int nchunks = K / CK;  // K is a multiple of 128

  // The wave's 32 weight rows as one resource (N is a multiple of 128: every
  // row exists). For gate/up a second resource holds the 32 up rows, N rows
  // further on.
  const long rows_e = GU ? 2L * N : (long)N;
  const long n0 = (long)blockIdx.y * MGG_BN + wave * 32;  // wave-uniform
  const WT* wb = w + ((size_t)e * rows_e + n0) * K;
  const int wbytes = (int)(32L * K * ES);
  const rsrc_t wrs0 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<WT*>(wb), 0, wbytes, MOE_RSRC_FLAGS);
  const rsrc_t wrs1 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<WT*>(GU ? wb + (size_t)N * K : wb), 0, wbytes,
      MOE_RSRC_FLAGS);
  const unsigned woff = (unsigned)(r * (long)K * ES) + 16 * h;
  auto wload = [&](int c) {  // chunk c of the lane's row, zeros past K
    WChunk<GU> o;
    const unsigned off = c < nchunks ? woff + (unsigned)c * 128 : MOE_OOB;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      o.g[u] = buf_load(wrs0, off + 32 * u);
      if constexpr (GU) o.u[u] = buf_load(wrs1, off + 32 * u);
    }
    return o;
  };

  // A staging: thread -> 16 B piece p of rows rw0 + RP * i of a chunk. The
  // gate/up GEMM gathers the tokens' x rows from the whole of x; the down
  // GEMM reads the tile's own 64 h rows. Padding rows are zeros.
  const int p = tid % PP;
  const int rw0 = tid / PP;
  const u16* abase_p = GU ? a : a + (size_t)row0 * a_stride;
  const long abytes =
      GU ? ((long)(a_rows - 1) * a_stride + K) * 2 : (long)MGG_BM * K * 2;
  const rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(abase_p), 0, (int)abytes, MOE_RSRC_FLAGS);
  unsigned abase[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = rw0 + RP * i;
    const int pr = pair_s[row];
    const long src = GU ? pr / top_k : row;  // x row of the token, or h row
    abase[i] = pr >= 0 && (!GU || src < a_rows)
                   ? (unsigned)((src * a_stride + p * 8) * 2)
                   : MOE_OOB;
  }
  vec4w ar[NI];
  auto afetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      ar[i] = buf_load(ars, c < nchunks && abase[i] != MOE_OOB
                                ? abase[i] + (unsigned)c * (CK * 2)
                                : MOE_OOB);
  };
  auto awrite = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      *reinterpret_cast<vec4w*>(
          &as[(buf * MGG_BM + rw0 + RP * i) * LDA + p * 16]) = ar[i];
  };

  // the row scales of this lane's output column (e4m3 weights only)
  float sc0 = 1.f, sc1 = 1.f;
  if constexpr (W8) {
    const float* sc = w_scale + (size_t)e * rows_e + n0 + r;
    sc0 = sc[0];
    if constexpr (GU) sc1 = sc[N];
  }

  // [row block]: gate and up, or acc0 alone
  f32x16 acc0[2], acc1[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[m][i] = acc1[m][i] = 0.f;

  // bf16: k-step u of a chunk is k = 16 u + 8 h + j. e4m3: a 16 B load is two
  // k-steps, so k-step 2u + s is k = 32 u + 16 h + 8 s + j, and the A
  // fragments are read with the same permutation.
  auto compute = [&](int buf, const WChunk<GU>& wc) {
    const unsigned char* ab =
        &as[(buf * MGG_BM + r) * LDA + (W8 ? 32 : 16) * h];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if constexpr (W8) {
        const vec4w g = wc.g[u];
        const bf16x8 g0 = frag_fp8(g[0], g[1]), g1 = frag_fp8(g[2], g[3]);
        bf16x8 u0, u1;
        if constexpr (GU) {
          const vec4w v = wc.u[u];
          u0 = frag_fp8(v[0], v[1]);
          u1 = frag_fp8(v[2], v[3]);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
              ab + m * 32 * LDA + 64 * u);
          const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
              ab + m * 32 * LDA + 64 * u + 16);
          acc0[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, g0, acc0[m],
                                                            0, 0, 0);
          acc0[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, g1, acc0[m],
                                                            0, 0, 0);
          if constexpr (GU) {
            acc1[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, u0, acc1[m],
                                                              0, 0, 0);
            acc1[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, u1, acc1[m],
                                                              0, 0, 0);
          }
        }
      } else {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const bf16x8 av = *reinterpret_cast<const bf16x8*>(
              ab + m * 32 * LDA + 32 * u);
          acc0[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              av, frag(wc.g[u]), acc0[m], 0, 0, 0);
          if constexpr (GU)
            acc1[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                av, frag(wc.u[u]), acc1[m], 0, 0, 0);
        }
      }
    }
  };

  // weight ring: chunk cc is in wr[cc % R], the next R - 1 are in flight
  afetch(0);
  WChunk<GU> wr[R];
#pragma unroll
  for (int i = 0; i + 1 < R; ++i) wr[i] = wload(i);
  awrite(0);
  __syncthreads();

  for (int c = 0; c < nchunks; c += R) {  // block-uniform trip count
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int cc = c + i;
      if (cc >= nchunks) break;
      afetch(cc + 1);
      wr[(i + R - 1) % R] = wload(cc + R - 1);
      compute(cc & 1, wr[i]);
      awrite((cc + 1) & 1);
      __syncthreads();
    }
  }

  // register i of block m holds tile row 32 m + (i & 3) + 8 * (i >> 2) + 4h
  // of column n. The scales are powers of two: applying them to the fp32
  // sums is exact.
  const long n = n0 + r;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 32 * m + (i & 3) + 8 * (i >> 2) + 4 * h;
      const int pr = pair_s[row];
      if (pr < 0) continue;
      if constexpr (GU) {
        const float g = acc0[m][i] * sc0;
        const float s = g / (1.f + expf(-g));
        const __bf16 b = (__bf16)(s * (acc1[m][i] * sc1));
        hout[(size_t)(row0 + row) * N + n] = __builtin_bit_cast(u16, b);
      } else {
        part[(size_t)pr * N + n] = acc0[m][i] * sc0 * route_w[pr];
      }
    }
  }
}

template <typename WT>
void launch_grouped(const void* x, long x_stride, const void* w_gate_up,
                    const void* w_down, const void* gate_up_scale,
                    const void* down_scale, const void* weights,
                    const void* n_tiles, const void* tile_expert,
                    const void* tile_row0, const void* sorted_pairs, void* h,
                    void* part, int T, int D, int I, int E, int top_k,
                    int max_tiles, hipStream_t stream) {
  const int np = T * top_k, cap = max_tiles * MGG_BM;
  hipLaunchKernelGGL((moe_grouped_gemm_kernel<true, WT>),
                     dim3((unsigned)max_tiles, (unsigned)(I / MGG_BN)),
                     dim3(MGG_THREADS), 0, stream, (const u16*)x, x_stride, T,
                     (const WT*)w_gate_up, (const float*)gate_up_scale,
                     (const int*)n_tiles, (const int*)tile_expert,
                     (const int*)tile_row0, (const int*)sorted_pairs,
                     (const float*)nullptr, (u16*)h, (float*)nullptr, top_k, I,
                     D, E, np, cap);
  hipLaunchKernelGGL((moe_grouped_gemm_kernel<false, WT>),
                     dim3((unsigned)max_tiles, (unsigned)(D / MGG_BN)),
                     dim3(MGG_THREADS), 0, stream, (const u16*)h, (long)I, cap,
                     (const WT*)w_down, (const float*)down_scale,
                     (const int*)n_tiles, (const int*)tile_expert,
                     (const int*)tile_row0, (const int*)sorted_pairs,
                     (const float*)weights, (u16*)nullptr, (float*)part, top_k,
                     D, I, E, np, cap);
}

}  // namespace

extern "C" {

// The rows of an M tile and the worst-case number of tiles of T tokens:
// every expert's last tile may be partial.
int kt_moe_grouped_tile_rows(void) { return MGG_BM; }

int kt_moe_grouped_max_tiles(long T, int E, int top_k) {
  return (int)((T * top_k + MGG_BM - 1) / MGG_BM) + E;
}

// x: [T, D] bf16, row stride x_stride elements, the whole of it below 2 GiB;
// logits: [T, E] contiguous, bf16 (is_bf16 != 0) or fp32; the weights and
// scales as kt_moe_mlp takes them. Scratch, with M = kt_moe_grouped_max_tiles:
// sel [T, top_k] int32, weights [T, top_k] fp32, expert_count [E],
// sorted_pairs [M * 64], tile_expert [M], tile_row0 [M], n_tiles [1] int32,
// h [M * 64, I] bf16, part [T, top_k, D] fp32. out: [T, D] bf16. The binding
// has checked 1 <= T <= 4096, 1 <= top_k <= min(E, 8), E <= 64, D % 128 ==
// I % 128 == 0, both <= 2^16, and the alignments.
void kt_moe_grouped_mlp(const void* x, long x_stride, const void* logits,
                        int is_bf16, const void* w_gate_up,
                        const void* w_down, void* sel, void* weights,
                        void* expert_count, void* sorted_pairs,
                        void* tile_expert, void* tile_row0, void* n_tiles,
                        void* h, void* part, void* out, int T, int D, int I,
                        int E, int top_k, int fp8, const void* gate_up_scale,
                        const void* down_scale, hipStream_t stream) {
  const int max_tiles = kt_moe_grouped_max_tiles(T, E, top_k);
  hipLaunchKernelGGL(moe_route_rows_kernel,
                     dim3((unsigned)((T + MGG_THREADS / 64 - 1) /
                                     (MGG_THREADS / 64))),
                     dim3(MGG_THREADS), 0, stream, logits, is_bf16, (int*)sel,
                     (float*)weights, T, E, top_k);
  hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(MGG_ALIGN_THREADS), 0,
                     stream, (const int*)sel, T * top_k, E, max_tiles,
                     (int*)expert_count, (int*)sorted_pairs, (int*)tile_expert,
                     (int*)tile_row0, (int*)n_tiles);
  if (fp8)
    launch_grouped<unsigned char>(x, x_stride, w_gate_up, w_down,
                                  gate_up_scale, down_scale, weights, n_tiles,
                                  tile_expert, tile_row0, sorted_pairs, h,
                                  part, T, D, I, E, top_k, max_tiles, stream);
  else
    launch_grouped<u16>(x, x_stride, w_gate_up, w_down, nullptr, nullptr,
                        weights, n_tiles, tile_expert, tile_row0, sorted_pairs,
                        h, part, T, D, I, E, top_k, max_tiles, stream);
  kt_moe_combine(part, out, T, D, top_k, 1, stream);
}

}  // extern "C"
