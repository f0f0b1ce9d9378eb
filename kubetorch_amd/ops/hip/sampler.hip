// Batched token sampler for gfx950: temperature, top-k, top-p and a seeded
// draw for every row of a [B, V] bf16 logits matrix in one launch.
//
// One 1024-thread workgroup per row. bf16 has 16-bit order-preserving keys,
// so both filters are thresholds on the key and each threshold is a radix
// select of two 8-bit digits over a 256-bin LDS histogram: top-k counts
// tokens per bin, top-p adds their softmax weight per bin. No sort. The row
// (256 KB at V = 128,256) is re-read from L2 by every pass; a row only runs
// the passes its parameters need (the branches are workgroup-uniform).
//
//   pass A   arg-max (key, lowest index)      every row; all a greedy row needs
//   pass K1  counts by high digit             0 < top_k < V
//   pass K2  counts by low digit in that bin
//   pass P1  weights by high digit            top_p < 1
//   pass P2  weights by low digit in that bin
//   pass F   Philox + race score + arg-max    temperature > 0
//
// The result is a pure function of the row and its parameters: bin mass is
// summed in 64-bit fixed point (integer LDS adds commute, float adds do
// not), every comparison that picks a bin is on integers or on a double
// derived from them, and ties resolve to the lowest index. The kernel reads
// the row and the five parameter vectors and stores out[row]; nothing else.
//
// The draw is an exponential race (Gumbel-max): token i gets
//   score_i = x_i / T - log(E_i),  E_i = -log1p(-v_i),  v_i = (r_i + .5) 2^-23
// with r_i the top 23 bits of word i & 3 of Philox4x32-10 under the key
// (seed lo, seed hi) and the counter (i >> 2, offset lo, offset hi, 0). v and
// 1 - v are exact in fp32; log1pf and logf keep E's relative accuracy for the
// small v that win.

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int SAMPLER_THREADS = 1024;
constexpr int SAMPLER_WAVES = SAMPLER_THREADS / 64;
constexpr unsigned KEY_NEG_INF = 0x007Fu;  // key of -inf (bits 0xFF80)
constexpr unsigned KEY_POS_INF = 0xFF80u;  // key of +inf (bits 0x7F80)
constexpr float MASS_ONE = 17592186044416.f;  // 2^44: V <= 2^18 sums < 2^63

typedef unsigned long long u64;

// bf16 bits -> 16-bit key with key order == value order. NaN counts as
// -inf and -0 as +0, so equal keys are exactly equal logits.
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

// fp32 (never NaN here) -> 32-bit key with key order == value order
__device__ __forceinline__ unsigned score_key(float s) {
  const unsigned b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ u64 shfl_xor64(u64 v, int mask) {
  const unsigned lo = __shfl_xor((unsigned)v, mask, 64);
  const unsigned hi = __shfl_xor((unsigned)(v >> 32), mask, 64);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 shfl_down64(u64 v, int delta) {
  const unsigned lo = __shfl_down((unsigned)v, delta, 64);
  const unsigned hi = __shfl_down((unsigned)(v >> 32), delta, 64);
  return ((u64)hi << 32) | lo;
}

// max over the workgroup, returned to every thread; red holds SAMPLER_WAVES
__device__ __forceinline__ u64 block_max64(u64 v, u64* red) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const u64 o = shfl_xor64(v, m);
    v = o > v ? o : v;
  }
  __syncthreads();  // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = red[0];
#pragma unroll
  for (int w = 1; w < SAMPLER_WAVES; ++w) r = red[w] > r ? red[w] : r;
  return r;
}

// f(index, key) for every element of the row: 16-byte loads of 8 logits,
// then the V % 8 tail one element per thread.
template <typename F>
__device__ __forceinline__ void for_each_key(const uint16_t* row, int V, F f) {
  const int nvec = V >> 3;
  const uint4* rv = reinterpret_cast<const uint4*>(row);
  for (int v = threadIdx.x; v < nvec; v += SAMPLER_THREADS) {
    const uint4 q = rv[v];
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f(v * 8 + 2 * j, key_of(w[j]));
      f(v * 8 + 2 * j + 1, key_of(w[j] >> 16));
    }
  }
  const int t = nvec * 8 + (int)threadIdx.x;
  if (t < V) f(t, key_of(row[t]));
}

__device__ __forceinline__ void clear_hist(u64* hist) {
  __syncthreads();  // the previous scan has read it
  if (threadIdx.x < 256) hist[threadIdx.x] = 0;
  __syncthreads();
}

// Sum of the 256 bins, to every thread (integer adds: any order is exact).
__device__ __forceinline__ u64 hist_total(const u64* hist, u64* red) {
  __syncthreads();  // every add has landed; red is free
  if (threadIdx.x < 256) {
    u64 v = hist[threadIdx.x];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += shfl_xor64(v, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  }
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// Wave 0 walks the 256 bins from the top. Lane l owns bins 4l .. 4l+3; a
// suffix scan over the lanes gives each its sum of all higher bins.
// Counting form (mass == false): the bin holding the need-th largest
// element, sel[1] = need minus the count above that bin.
// Mass form: the lowest bin b with base + (sum of bins above b) < limit,
// sel[1] = that sum including base; sel[0] = 256 when no bin qualifies.
__device__ __forceinline__ void select_bin(const u64* hist, bool mass, u64 need,
                                           u64 base, double limit, u64* sel) {
  __syncthreads();  // every add has landed
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    u64 c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = hist[4 * l + j];
    const u64 own = c[0] + c[1] + c[2] + c[3];
    u64 x = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 o = shfl_down64(x, d);
      if (l + d < 64) x += o;
    }
    u64 above = base + (x - own);
    unsigned found = 256;
    u64 found_above = 0;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      const bool hit = mass ? ((double)above < limit)
                            : (above < need && above + c[j] >= need);
      if (hit) {  // mass: keeps the lowest; counting: one bin only
        found = 4 * l + j;
        found_above = above;
      }
      above += c[j];
    }
    unsigned best = found;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const unsigned o = __shfl_xor(best, m, 64);
      best = o < best ? o : best;
    }
    if (l == 0 && best == 256) {
      sel[0] = 256;
      sel[1] = 0;
    }
    if (best != 256 && found == best) {
      sel[0] = best;
      sel[1] = mass ? found_above : need - found_above;
    }
  }
  __syncthreads();
}

struct Philox {
  unsigned w[4];
};

__device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1,
                                                unsigned c2, unsigned c3,
                                                unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ float race_score(float x, float T, unsigned word) {
  const float v = ((float)(word >> 9) + 0.5f) * 1.1920928955078125e-07f;
  const float E = -log1pf(-v);
  return x / T - logf(E);
}

// A cheap upper bound of race_score: E = v + v^2/2 + .. >= v, so
// -log(E) <= -log(v). The hardware log and the multiply by 1/T are a few
// instructions where the accurate score is a few hundred (measured: the
// race over 128,256 tokens took 140 us with the accurate score for every
// token). Their errors, 2e-6 on |log v| <= 17 and 2^-23 relative on x / T,
// are covered by the margin, so a token whose bound is below a score already
// seen can neither beat nor tie it, and skipping it changes no result.
__device__ __forceinline__ float race_bound(float x, float invT,
                                            unsigned word) {
  const float v = ((float)(word >> 9) + 0.5f) * 1.1920928955078125e-07f;
  const float xt = x * invT;
  return xt - __logf(v) + (1e-4f + 1e-6f * fabsf(xt));
}

// One candidate of the race: `win` packs (score key, ~index), `best` is the
// thread's highest accurate score so far.
__device__ __forceinline__ void race_step(float x, float T, float invT,
                                          unsigned word, int i, float& best,
                                          u64& win) {
  if (race_bound(x, invT, word) < best) return;
  const float s = race_score(x, T, word);
  const u64 c = ((u64)score_key(s) << 32) | (unsigned)~i;
  win = c > win ? c : win;
  best = s > best ? s : best;
}

__global__ void __launch_bounds__(SAMPLER_THREADS)
sample_tokens_kernel(const uint16_t* __restrict__ logits, long row_stride,
                     int V, const float* __restrict__ temperature,
                     const int* __restrict__ top_k,
                     const float* __restrict__ top_p,
                     const long long* __restrict__ seed,
                     const long long* __restrict__ offset,
                     long long* __restrict__ out) {
  __shared__ u64 hist[256];
  __shared__ u64 red[SAMPLER_WAVES];
  __shared__ u64 sel[2];

  const int b = blockIdx.x;
  const uint16_t* row = logits + (long)b * row_stride;
  const float T = temperature[b];
  const int k = top_k[b];
  const float p = top_p[b];

  // pass A: the maximum and its lowest index. ~index in the low word makes
  // the 64-bit maximum prefer the lowest index; the start value is index 0.
  u64 best = 0xFFFFFFFFull;
  for_each_key(row, V, [&](int i, unsigned key) {
    const u64 c = ((u64)key << 32) | (unsigned)~i;
    best = c > best ? c : best;
  });
  best = block_max64(best, red);
  const unsigned kmax = (unsigned)(best >> 32);
  unsigned token = ~(unsigned)best;

  const bool greedy = !(T > 0.f);
  if (kmax <= KEY_NEG_INF) token = 0;  // no logit above -inf
  // a +inf outweighs everything: its lowest index, like a greedy row
  if (!greedy && kmax > KEY_NEG_INF && kmax < KEY_POS_INF) {
    unsigned kept = 0;  // tokens with key >= kept survive the filters
    if (k > 0 && k < V) {
      clear_hist(hist);
      for_each_key(row, V, [&](int, unsigned key) {
        atomicAdd(&hist[key >> 8], 1ull);
      });
      select_bin(hist, false, (u64)k, 0, 0.0, sel);
      const unsigned hi = (unsigned)sel[0];
      const u64 need = sel[1];
      clear_hist(hist);
      for_each_key(row, V, [&](int, unsigned key) {
        if ((key >> 8) == hi) atomicAdd(&hist[key & 255u], 1ull);
      });
      select_bin(hist, false, need, 0, 0.0, sel);
      kept = (hi << 8) | (unsigned)sel[0];
    }
    if (p < 1.f) {
      const float xmax = value_of(kmax);
      const unsigned kk = kept;
      clear_hist(hist);
      for_each_key(row, V, [&](int, unsigned key) {
        if (key >= kk && key > KEY_NEG_INF) {
          const float w = expf((value_of(key) - xmax) / T);
          atomicAdd(&hist[key >> 8], (u64)(w * MASS_ONE));
        }
      });
      const u64 Z = hist_total(hist, red);
      const double limit = (double)p * (double)Z;
      select_bin(hist, true, 0, 0, limit, sel);
      unsigned kp = kmax;  // the maximum always stays
      if (sel[0] != 256) {
        const unsigned hi = (unsigned)sel[0];
        const u64 base = sel[1];
        clear_hist(hist);
        for_each_key(row, V, [&](int, unsigned key) {
          if (key >= kk && (key >> 8) == hi && key > KEY_NEG_INF) {
            const float w = expf((value_of(key) - xmax) / T);
            atomicAdd(&hist[key & 255u], (u64)(w * MASS_ONE));
          }
        });
        select_bin(hist, true, 0, base, limit, sel);
        if (sel[0] != 256) kp = (hi << 8) | (unsigned)sel[0];
      }
      kp = kp > kmax ? kmax : kp;
      kept = kp > kept ? kp : kept;
    }

    // pass F: the race among the kept tokens
    const long long sd = seed[b], off = offset[b];
    const unsigned k0 = (unsigned)(u64)sd, k1 = (unsigned)((u64)sd >> 32);
    const unsigned o0 = (unsigned)(u64)off, o1 = (unsigned)((u64)off >> 32);
    u64 win = 0xFFFFFFFFull;
    float seen = -INFINITY;  // this thread's best score so far
    const float invT = 1.f / T;
    const int nvec = V >> 3;
    const uint4* rv = reinterpret_cast<const uint4*>(row);
    for (int v = threadIdx.x; v < nvec; v += SAMPLER_THREADS) {
      const uint4 q = rv[v];
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // four tokens share one Philox block
        unsigned key[4];
        key[0] = key_of(w[2 * h]);
        key[1] = key_of(w[2 * h] >> 16);
        key[2] = key_of(w[2 * h + 1]);
        key[3] = key_of(w[2 * h + 1] >> 16);
        if (key[0] < kept && key[1] < kept && key[2] < kept && key[3] < kept)
          continue;
        const Philox r = philox4x32_10((unsigned)(v * 2 + h), o0, o1, 0, k0, k1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (key[j] < kept) continue;
          race_step(value_of(key[j]), T, invT, r.w[j], v * 8 + h * 4 + j,
                    seen, win);
        }
      }
    }
    const int t = nvec * 8 + (int)threadIdx.x;
    if (t < V) {
      const unsigned key = key_of(row[t]);
      if (key >= kept) {
        const Philox r = philox4x32_10((unsigned)(t >> 2), o0, o1, 0, k0, k1);
        // selects, not r.w[t & 3]: a dynamically indexed array would be
        // moved to LDS, 16 B for each of the 1024 threads
        const int j = t & 3;
        const unsigned word = j == 0 ? r.w[0] : j == 1 ? r.w[1]
                            : j == 2 ? r.w[2] : r.w[3];
        race_step(value_of(key), T, invT, word, t, seen, win);
      }
    }
    win = block_max64(win, red);
    token = ~(unsigned)win;
  }
  if (threadIdx.x == 0) out[b] = token < (unsigned)V ? (long long)token : 0;
}

}  // namespace

extern "C" void kt_sample_tokens(const void* logits, long row_stride, int B,
                                 int V, const void* temperature,
                                 const void* top_k, const void* top_p,
                                 const void* seed, const void* offset,
                                 void* out, hipStream_t stream) {
  hipLaunchKernelGGL(sample_tokens_kernel, dim3(B), dim3(SAMPLER_THREADS), 0,
                     stream, (const uint16_t*)logits, row_stride, V,
                     (const float*)temperature, (const int*)top_k,
                     (const float*)top_p, (const long long*)seed,
                     (const long long*)offset, (long long*)out);
}
