// Per-token log-probabilities for gfx950: for every row of a [B, V] bf16
// logits matrix, the log-probability and rank of one given token and the
// top_n most likely tokens with their log-probabilities, in one launch.
//
// One 1024-thread workgroup per row, as in sampler.hip, and the same 16-bit
// order-preserving bf16 keys (NaN counts as -inf, -0 as +0). The row (256 KB
// at V = 128,256) is re-read from L2 by every pass:
//
//   pass 1   maximum key, #keys above the token's key (the rank), #(+inf);
//            with top_n > 0 also the counts by high digit
//   pass 2   S = sum exp((x - max) / T): fp32 terms, fp64 accumulation
//   pass K2  counts by low digit in the bin of the top_n-th key  (top_n > 0)
//   pass G   gather the keys above the threshold and the lowest-index keys
//            equal to it, then one wave orders the <= 32 candidates
//
// Everything that decides an index is an integer: the rank is a sum of
// integer counts, the threshold is a radix select of two 8-bit digits over
// an LDS histogram, and which of the elements equal to the threshold are
// taken comes from an exclusive prefix count in index order. Pass G walks
// the row in chunks of 1024 vectors, thread t holding the 8 contiguous
// logits of vector chunk * 1024 + t, so (chunk, thread, lane of the vector)
// is index order and a workgroup scan of the per-thread counts numbers the
// equal elements by index. Elements above the threshold take their slot from
// an LDS counter; their order is arbitrary and the final ordering by
// (key descending, index ascending) removes it. S is reduced by a fixed
// tree (64-lane butterfly, then the 16 wave sums in order), so a row's four
// outputs are a pure function of the row, its token and its temperature.
//
// The histogram is kept in 32 copies, picked by lane & 31 and 257 words
// apart: logits crowd into a few high-digit bins, and 64 lanes adding to one
// LDS word serialise (in sampler.hip that is most of a 25 us pass).
//
// Global memory: reads of the row, token[row] and temperature[row]; plain
// stores of the row's outputs. No global atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int LP_THREADS = 1024;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_MAX_TOP = 32;
constexpr int HIST_COPIES = 32;
constexpr int HIST_PITCH = 257;  // copies land on different banks
constexpr unsigned KEY_NEG_INF = 0x007Fu;  // key of -inf (bits 0xFF80)
constexpr unsigned KEY_POS_INF = 0xFF80u;  // key of +inf (bits 0x7F80)

typedef unsigned long long u64;

// bf16 bits -> 16-bit key with key order == value order. NaN counts as
// -inf and -0 as +0, so equal keys are exactly equal logits. No key is 0.
__device__ __forceinline__ unsigned key_of(unsigned bits) {
  bits &= 0xFFFFu;
  if ((bits & 0x7FFFu) > 0x7F80u) bits = 0xFF80u;
  if (bits == 0x8000u) bits = 0u;
  return (bits & 0x8000u) ? (~bits & 0xFFFFu) : (bits | 0x8000u);
}

__device__ __forceinline__ float value_of(unsigned key) {
  const unsigned bits = (key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu);
  return __uint_as_float(bits << 16);
}

// The 8 keys of vector v into k[0..7].
__device__ __forceinline__ void load_keys(const uint16_t* row, int v,
                                          unsigned* k) {
  const uint4 q = reinterpret_cast<const uint4*>(row)[v];
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    k[2 * j] = key_of(w[j]);
    k[2 * j + 1] = key_of(w[j] >> 16);
  }
}

// f(key) for every element of the row: 16-byte loads of 8 logits, then the
// V % 8 tail one element per thread.
template <typename F>
__device__ __forceinline__ void for_each_key(const uint16_t* row, int V, F f) {
  const int nvec = V >> 3;
  for (int v = threadIdx.x; v < nvec; v += LP_THREADS) {
    unsigned k[8];
    load_keys(row, v, k);
#pragma unroll
    for (int j = 0; j < 8; ++j) f(k[j]);
  }
  const int t = nvec * 8 + (int)threadIdx.x;
  if (t < V) f(key_of(row[t]));
}

// Maximum (is_max) or sum of v over the workgroup, to every thread.
__device__ __forceinline__ unsigned block_reduce(unsigned v, bool is_max,
                                                 unsigned* red) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned o = __shfl_xor(v, m, 64);
    v = is_max ? (o > v ? o : v) : v + o;
  }
  __syncthreads();  // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned r = red[0];
#pragma unroll
  for (int w = 1; w < LP_WAVES; ++w)
    r = is_max ? (red[w] > r ? red[w] : r) : r + red[w];
  return r;
}

// Sum of v over the workgroup by a fixed tree, to every thread: a butterfly
// over the wave's lanes (both operands of every add are the same pair in
// every lane, so all lanes agree), then the wave sums in wave order.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < LP_WAVES; ++w) r += red[w];
  return r;
}

// Exclusive prefix of v over the threads in thread order; total to all.
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* wtot,
                                               unsigned& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  __syncthreads();  // wtot may still be read from the previous scan
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < LP_WAVES; ++i) {
    const unsigned t = wtot[i];
    before += i < w ? t : 0u;
    all += t;
  }
  total = all;
  return before + incl - v;
}

__device__ __forceinline__ void clear_hist(unsigned* hist) {
  __syncthreads();  // the previous fold has read it
  for (int i = threadIdx.x; i < HIST_COPIES * HIST_PITCH; i += LP_THREADS)
    hist[i] = 0;
  __syncthreads();
}

__device__ __forceinline__ void hist_add(unsigned* hist, unsigned bin) {
  atomicAdd(&hist[(threadIdx.x & (HIST_COPIES - 1)) * HIST_PITCH + bin], 1u);
}

// Fold the copies into bins[256]; then wave 0 walks the bins from the top
// (lane l owns bins 4l .. 4l+3, a suffix scan over the lanes gives each its
// count in all higher bins): sel[0] = the bin holding the need-th largest
// element, sel[1] = need minus the count above that bin. 1 <= need <= total.
__device__ __forceinline__ void select_bin(const unsigned* hist, unsigned need,
                                           unsigned* bins, unsigned* sel) {
  __syncthreads();  // every add has landed
  if (threadIdx.x < 256) {
    unsigned s = 0;
#pragma unroll 8
    for (int c = 0; c < HIST_COPIES; ++c)
      s += hist[c * HIST_PITCH + threadIdx.x];
    bins[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    unsigned c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = bins[4 * l + j];
    const unsigned own = c[0] + c[1] + c[2] + c[3];
    unsigned x = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_down(x, d, 64);
      if (l + d < 64) x += o;
    }
    unsigned above = x - own;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      if (above < need && above + c[j] >= need) {  // one bin only
        sel[0] = 4 * l + j;
        sel[1] = need - above;
      }
      above += c[j];
    }
  }
  __syncthreads();
}

// The row's log-probability of a key. Edge rows are decided by kmax.
struct RowDist {
  unsigned kmax;
  float xmax, T;
  double logS;  // log sum exp((x - max) / T); log(#(+inf)) on a +inf row

  __device__ __forceinline__ float operator()(unsigned key) const {
    if (kmax <= KEY_NEG_INF) return __uint_as_float(0x7FC00000u);  // NaN
    if (kmax >= KEY_POS_INF)
      return key >= KEY_POS_INF ? (float)(-logS) : -INFINITY;
    if (key <= KEY_NEG_INF) return -INFINITY;
    return (float)((double)((value_of(key) - xmax) / T) - logS);
  }
};

__global__ void __launch_bounds__(LP_THREADS)
token_logprobs_kernel(const uint16_t* __restrict__ logits, long row_stride,
                      int V, const long long* __restrict__ token,
                      const float* __restrict__ temperature, int top_n,
                      float* __restrict__ logprob, int* __restrict__ rank,
                      int* __restrict__ top_ids,
                      float* __restrict__ top_logprobs) {
  __shared__ unsigned hist[HIST_COPIES * HIST_PITCH];
  __shared__ unsigned bins[256];
  __shared__ double red64[LP_WAVES];
  __shared__ unsigned red[LP_WAVES];
  __shared__ unsigned sel[2];
  __shared__ unsigned cand_key[LP_MAX_TOP];
  __shared__ int cand_idx[LP_MAX_TOP];
  __shared__ unsigned n_above;

  const int b = blockIdx.x;
  const uint16_t* row = logits + (long)b * row_stride;
  const float Tin = temperature[b];
  const float T = Tin > 0.f ? Tin : 1.f;
  const long long tok = token[b];
  const bool tok_ok = tok >= 0 && tok < (long long)V;
  // an impossible key for a token outside the row: nothing is above it
  const unsigned ktok = tok_ok ? key_of(row[tok]) : 0xFFFFFFFFu;

  // pass 1
  unsigned kmax = 0, above = 0, ninf = 0;
  if (top_n > 0) {
    clear_hist(hist);
    for_each_key(row, V, [&](unsigned key) {
      kmax = key > kmax ? key : kmax;
      above += key > ktok;
      ninf += key == KEY_POS_INF;
      hist_add(hist, key >> 8);
    });
  } else {
    for_each_key(row, V, [&](unsigned key) {
      kmax = key > kmax ? key : kmax;
      above += key > ktok;
      ninf += key == KEY_POS_INF;
    });
  }
  kmax = block_reduce(kmax, true, red);
  above = block_reduce(above, false, red);

  RowDist lp;
  lp.kmax = kmax;
  lp.xmax = value_of(kmax);
  lp.T = T;
  if (kmax >= KEY_POS_INF) {
    ninf = block_reduce(ninf, false, red);
    lp.logS = log((double)ninf);
  } else if (kmax > KEY_NEG_INF) {
    // pass 2
    const float xmax = lp.xmax;
    double part = 0.0;
    for_each_key(row, V, [&](unsigned key) {
      part += (double)expf((value_of(key) - xmax) / T);
    });
    lp.logS = log(block_sum_f64(part, red64));
  } else {
    lp.logS = 0.0;
  }

  if (threadIdx.x == 0) {
    logprob[b] = tok_ok ? lp(ktok) : __uint_as_float(0x7FC00000u);
    rank[b] = tok_ok ? (int)above + 1 : 0;
  }
  if (top_n <= 0) return;

  // the top_n-th largest key: high digit from pass 1's counts, then low
  const int nvec = V >> 3;
  const unsigned n_eff = top_n < V ? top_n : V;
  select_bin(hist, n_eff, bins, sel);
  const unsigned hi = sel[0];
  const unsigned need_hi = sel[1];
  clear_hist(hist);
  for_each_key(row, V, [&](unsigned key) {
    if ((key >> 8) == hi) hist_add(hist, key & 255u);
  });
  select_bin(hist, need_hi, bins, sel);
  const unsigned thr = (hi << 8) | sel[0];
  const unsigned need = sel[1];        // elements equal to thr to take
  const unsigned n_gt = n_eff - need;  // elements above thr, all taken

  if (threadIdx.x < LP_MAX_TOP) {
    cand_key[threadIdx.x] = 0;
    cand_idx[threadIdx.x] = -1;
  }
  if (threadIdx.x == 0) n_above = 0;
  __syncthreads();

  // pass G: chunk c < nchunks is vectors c * 1024 + t; the last round is
  // the V % 8 tail, one element per thread
  const int nchunks = (nvec + LP_THREADS - 1) / LP_THREADS;
  const int rounds = nchunks + ((V & 7) ? 1 : 0);
  unsigned taken = 0;  // elements equal to thr seen in lower rounds
  for (int c = 0; c < rounds; ++c) {
    unsigned k[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // 0 is no key
    int first = 0;
    if (c < nchunks) {
      const int v = c * LP_THREADS + (int)threadIdx.x;
      if (v < nvec) load_keys(row, v, k);
      first = v * 8;
    } else {
      first = nvec * 8 + (int)threadIdx.x;
      if (first < V) k[0] = key_of(row[first]);
    }
    unsigned eq = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (k[j] > thr) {
        const unsigned slot = atomicAdd(&n_above, 1u);
        if (slot < n_gt) {
          cand_key[slot] = k[j];
          cand_idx[slot] = first + j;
        }
      }
      eq += k[j] == thr;
    }
    if (taken < need) {  // workgroup-uniform
      unsigned total;
      unsigned pos = taken + block_scan(eq, red, total);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (k[j] == thr) {
          if (pos < need) {
            cand_key[n_gt + pos] = thr;
            cand_idx[n_gt + pos] = first + j;
          }
          ++pos;
        }
      }
      taken += total;
    }
  }
  __syncthreads();

  // order by (key descending, index ascending): a candidate's place is the
  // number of candidates ahead of it; (key, ~index) are all different
  if (threadIdx.x < 64) {
    const unsigned l = threadIdx.x;
    const long out = (long)b * top_n;
    if (l < n_eff) {
      const unsigned key = cand_key[l];
      const int idx = cand_idx[l];
      const u64 mine = ((u64)key << 32) | (unsigned)~idx;
      unsigned place = 0;
      for (unsigned j = 0; j < n_eff; ++j) {
        const u64 o = ((u64)cand_key[j] << 32) | (unsigned)~cand_idx[j];
        place += o > mine;
      }
      if (place < n_eff) {
        top_ids[out + place] = idx;
        top_logprobs[out + place] = lp(key);
      }
    } else if (l < (unsigned)top_n) {
      top_ids[out + l] = -1;
      top_logprobs[out + l] = -INFINITY;
    }
  }
}

}  // namespace

extern "C" void kt_token_logprobs(const void* logits, long row_stride, int B,
                                  int V, const void* token,
                                  const void* temperature, int top_n,
                                  void* logprob, void* rank, void* top_ids,
                                  void* top_logprobs, hipStream_t stream) {
  hipLaunchKernelGGL(token_logprobs_kernel, dim3(B), dim3(LP_THREADS), 0,
                     stream, (const uint16_t*)logits, row_stride, V,
                     (const long long*)token, (const float*)temperature, top_n,
                     (float*)logprob, (int*)rank, (int*)top_ids,
                     (float*)top_logprobs);
}
