// Device code shared by the routed expert MLP kernels (moe.hip for up to 32
// rows, moe_grouped.hip above that): the routing rule of one token and the
// raw buffer loads both GEMMs gather their rows with.
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.h"

#define MOE_MAX_E 64

// exp(v - m) for v <= m in fp32. v == m is 1 (infinities included); the
// rounding error of v - m is recovered (TwoSum) and applied to first order,
// so the result is as accurate as expf itself for any spread of the logits.
__device__ __forceinline__ float exp_diff(float v, float m) {
  if (v == m) return 1.f;
  const float d = v - m;
  if (d == -INFINITY) return 0.f;
  const float b = -m;
  const float bb = d - v;
  const float err = (v - (d - bb)) + (b - bb);
  return expf(d) * (1.f + err);
}

// Routing of token t by one whole wave, a lane per expert: rank the logits
// (descending, equal logits lowest index first, NaN as -inf) and write the k
// best and their softmax to sel[t, :] and weights[t, :]. Returns the lane's
// k-slot, or -1 where its expert was not picked. t is wave-uniform.
__device__ __forceinline__ int moe_route_token(
    const void* __restrict__ logits, int is_bf16, int t, int E, int top_k,
    int lane, int* __restrict__ sel, float* __restrict__ weights) {
  float v = -INFINITY;
  if (lane < E) {
    v = is_bf16 ? bf2f(((const u16*)logits)[t * E + lane])
                : ((const float*)logits)[t * E + lane];
    if (v != v) v = -INFINITY;
  }
  int rank = 0;
  for (int o = 0; o < E; ++o) {
    const float vo = __shfl(v, o);
    rank += (vo > v || (vo == v && o < lane)) ? 1 : 0;
  }
  const bool picked = lane < E && rank < top_k;
  // the picked logits in slot order: every lane sums them the same way
  float m = 0.f, sum = 0.f;
  for (int j = 0; j < top_k; ++j) {
    const unsigned long long b = __ballot(lane < E && rank == j);
    const float vj = __shfl(v, __ffsll((long long)b) - 1);
    if (j == 0) m = vj;
    sum += exp_diff(vj, m);
  }
  if (picked) {
    sel[t * top_k + rank] = lane;
    weights[t * top_k + rank] = exp_diff(v, m) / sum;
  }
  return picked ? rank : -1;
}

// Raw buffer loads: a lane whose offset is at or past the resource's size
// gets zeros and makes no memory request, so empty rows, the tail of a K
// slice and the prefetch past its end need no branch.
#define MOE_RSRC_FLAGS 0x00020000  // gfx9 raw buffer, 32-bit data format
#define MOE_OOB 0x80000000u        // every resource here is < 2 GiB

typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ vec4w buf_load(rsrc_t rs, unsigned off) {
  return __builtin_bit_cast(
      vec4w, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
}

__device__ __forceinline__ bf16x8 frag(vec4w v) {
  return __builtin_bit_cast(bf16x8, v);
}
