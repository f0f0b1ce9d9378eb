// Device helpers shared by the hand-written kernels: vector types, bf16
// conversion and e4m3 unpacking.
#pragma once

#include <hip/hip_runtime.h>

typedef unsigned short u16;
typedef ushort vec8u __attribute__((ext_vector_type(8)));
typedef unsigned int vec2w __attribute__((ext_vector_type(2)));
typedef unsigned int vec4w __attribute__((ext_vector_type(4)));
typedef float vec2f __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float bf2f(u16 x) {
  return __uint_as_float(((unsigned int)x) << 16);
}

// fp32 -> bf16, round to nearest even. The rounding bias is added to a NaN's
// bits too: a NaN may come out as another NaN, as an infinity or as zero.
__device__ __forceinline__ u16 f2bf(float f) {
  unsigned int u = __float_as_uint(f);
  u += 0x7fff + ((u >> 16) & 1);
  return (u16)(u >> 16);
}

// fp32 -> bf16, round to nearest even; NaN stays NaN (0x7fc0)
__device__ __forceinline__ u16 f2bf_nan(float f) {
  unsigned int u = __float_as_uint(f);
  if (f != f) return (u16)0x7fc0;
  u += 0x7fff + ((u >> 16) & 1);
  return (u16)(u >> 16);
}

// The 4 OCP e4m3 bytes of a word -> 4 fp32, in byte order (exact)
__device__ __forceinline__ void e4m3x4_to_f32(unsigned int w, float* f) {
  const vec2f lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  const vec2f hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}

// Two fp32 that came from e4m3 -> their two bf16 in one word, exact: e4m3
// has 3 mantissa bits, so the high half of the fp32 is the bf16.
__device__ __forceinline__ unsigned int bf16_pair(vec2f f) {
  return (__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xffff0000u);
}

// The same 4 bytes as 4 bf16 in two words. Each half is converted and packed
// before the next is converted, not through e4m3x4_to_f32: the compiler
// schedules the MFMA loops that use this from the order written here.
__device__ __forceinline__ vec2w e4m3x4_to_bf16(unsigned int w) {
  vec2w o;
  o[0] = bf16_pair(__builtin_amdgcn_cvt_pk_f32_fp8(w, false));
  o[1] = bf16_pair(__builtin_amdgcn_cvt_pk_f32_fp8(w, true));
  return o;
}

// 8 e4m3 bytes (two dwords) -> one bf16x8 MFMA fragment
__device__ __forceinline__ bf16x8 frag_fp8(unsigned lo, unsigned hi) {
  const vec2w a = e4m3x4_to_bf16(lo), b = e4m3x4_to_bf16(hi);
  const vec4w o = {a[0], a[1], b[0], b[1]};
  return __builtin_bit_cast(bf16x8, o);
}
