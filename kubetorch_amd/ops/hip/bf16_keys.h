// Order-preserving 16-bit keys of bf16 logits and the walk of a vocabulary
// row by a workgroup, shared by sampler.hip and logprobs.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr unsigned KEY_NEG_INF = 0x007Fu;  // key of -inf (bits 0xFF80)
constexpr unsigned KEY_POS_INF = 0xFF80u;  // key of +inf (bits 0x7F80)

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

// The 8 keys of vector v (one 16-byte load) into k[0..7].
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

// f(index, key) for every element of the row by a workgroup of THREADS:
// 16-byte loads of 8 logits, then the V % 8 tail one element per thread.
template <int THREADS, typename F>
__device__ __forceinline__ void for_each_key(const uint16_t* row, int V, F f) {
  const int nvec = V >> 3;
  for (int v = threadIdx.x; v < nvec; v += THREADS) {
    unsigned k[8];
    load_keys(row, v, k);
#pragma unroll
    for (int j = 0; j < 8; ++j) f(v * 8 + j, k[j]);
  }
  const int t = nvec * 8 + (int)threadIdx.x;
  if (t < V) f(t, key_of(row[t]));
}
