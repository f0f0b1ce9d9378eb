// Weight-only FP8 linear for decode (gfx950 / CDNA4), W8A16:
//   y[m, n] = bf16( scale[n] * sum_k x[m, k] * e4m3(wq[n, k]) ),  1 <= M <= 32
// x is bf16 [M, K] (rows may be strided), wq is OCP e4m3 [N, K] row-major,
// scale is fp32 [N] and a power of two (the host validates it), so the one
// multiply of the fp32 accumulator in the epilogue is exact.
//
// Structure, per workgroup (4 waves) = (128 output columns, K slice):
//  - A wave owns 32 output columns = 32 rows of wq. Lane (r, h) streams row
//    n0 + r: one 16 B load is 16 consecutive k of that row, a wave
//    instruction covers 32 B of each of its 32 rows and the four loads of a
//    128-k tile a full 128 B line per row. The loads go straight to VGPRs
//    and run three tiles (12 loads per lane) ahead of their use; wq is read
//    exactly once and never touches LDS.
//  - fp8 -> bf16 is v_cvt_pk_f32_fp8 and the high half of each fp32 (e4m3
//    has 3 mantissa bits: exact). A load's low 8 bytes are the B fragment of
//    one mfma_f32_32x32x16_bf16 k-step and its high 8 bytes that of the
//    next, so k-step 2u+e of a tile holds, on lane half h, element j:
//        k = 128*tile + 32u + 16h + 8e + j.
//    x is the A operand and reads its fragments with the same permutation.
//  - x (at most 32 rows) is shared by the four waves through LDS: chunks of
//    256 k are loaded in full rows (512 B per row, 16 B per thread), double
//    buffered, one barrier per chunk. Rows >= M are never loaded (a raw
//    buffer load past its resource returns zeros without a memory
//    request): their LDS rows are zeros. The accumulator has the output
//    column on the lane and the x row in the registers.
//  - Split-K: blockIdx.y owns a contiguous range of 128-k tiles. With one
//    split the epilogue writes bf16 y; otherwise it writes its fp32 partial
//    [S, M, N] with plain stores and linear_w8_reduce sums the S slabs in
//    index order: no atomics, bit-identical run to run. The split factor
//    comes from (N, K) alone (kt_linear_w8_plan), so a row's result does not
//    depend on the batch it is computed in.
//
// Safety: columns n >= N read row N-1 again and are not stored; an empty K
// slice writes zeros. Every index that scales with N*K is 64-bit.
//
// No torch headers here; bindings.cpp declares the extern "C" launchers.

#include <hip/hip_runtime.h>

typedef unsigned short u16;
typedef unsigned int vec4w __attribute__((ext_vector_type(4)));
typedef float vec2f __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define LW_THREADS 256
#define LW_BN 128                    // output columns per workgroup
#define LW_KT 128                    // k per tile: 4 x 16 B per lane
#define LW_CT 2                      // tiles per x chunk
#define LW_LDX (LW_CT * LW_KT * 2 + 16)  // LDS row stride in bytes, 16 B pad
#define LW_MAX_M 32

namespace {

// the exact bf16 of two e4m3 values: high halves of their fp32
__device__ __forceinline__ unsigned bf16_pair(vec2f f) {
  return (__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xffff0000u);
}

// 8 e4m3 bytes (two dwords) -> one bf16x8 MFMA fragment
__device__ __forceinline__ bf16x8 frag_fp8(unsigned lo, unsigned hi) {
  vec4w o;
  o[0] = bf16_pair(__builtin_amdgcn_cvt_pk_f32_fp8(lo, false));
  o[1] = bf16_pair(__builtin_amdgcn_cvt_pk_f32_fp8(lo, true));
  o[2] = bf16_pair(__builtin_amdgcn_cvt_pk_f32_fp8(hi, false));
  o[3] = bf16_pair(__builtin_amdgcn_cvt_pk_f32_fp8(hi, true));
  return __builtin_bit_cast(bf16x8, o);
}

struct WTile {
  vec4w v[4];
};

// Raw buffer loads: a lane whose offset is at or past the resource's size
// gets zeros and makes no memory request, so rows >= M, the tail of a K
// slice and the prefetch past its end need no branch (a branch around a
// load makes the compiler drain every load in flight at the join).
#define LW_RSRC_FLAGS 0x00020000  // gfx9 raw buffer, 32-bit data format
#define LW_OOB 0x80000000u        // every resource here is < 2 GiB

typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ vec4w buf_load(rsrc_t rs, unsigned off) {
  return __builtin_bit_cast(
      vec4w, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
}

__device__ __forceinline__ WTile load_tile(rsrc_t rs, unsigned off) {
  WTile t;
#pragma unroll
  for (int u = 0; u < 4; ++u) t.v[u] = buf_load(rs, off + 32 * u);
  return t;
}

__global__ __launch_bounds__(LW_THREADS, 2) void linear_w8_kernel(
    const u16* __restrict__ x, long x_stride,
    const unsigned char* __restrict__ wq, const float* __restrict__ scale,
    u16* __restrict__ y, float* __restrict__ part, int M, int N, int K,
    int tiles_per_split) {
  __shared__ __attribute__((aligned(16))) unsigned char
      xs[2 * LW_MAX_M * LW_LDX];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31;  // MFMA row/column index of this lane
  const int h = lane >> 5;  // lane half

  // this workgroup's K slice, in tiles (block-uniform)
  const int t0 = (int)blockIdx.y * tiles_per_split;
  int nt = K / LW_KT - t0;
  nt = nt > tiles_per_split ? tiles_per_split : nt;
  nt = nt < 0 ? 0 : nt;
  const int nchunks = (nt + LW_CT - 1) / LW_CT;
  const size_t k0 = (size_t)(nt > 0 ? t0 : 0) * LW_KT;  // inside the row

  // wq: the wave's 32 rows from column k0 on as one resource (32 * K bytes
  // at most; the binding bounds K). Columns n >= N read row N-1 again.
  const long n0 = (long)blockIdx.x * LW_BN + wave * 32;  // wave-uniform
  const long nb = n0 < N ? n0 : (long)N - 1;
  const long n = n0 + r;
  const long nrows = (long)N - nb < 32 ? (long)N - nb : 32;
  const rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(wq) + (size_t)nb * K + k0, 0,
      (int)((nrows - 1) * K + (K - (long)k0)), LW_RSRC_FLAGS);
  const unsigned woff =
      (unsigned)((r < nrows ? r : nrows - 1) * (long)K) + 16 * h;
  auto wtile = [&](int t) {  // tile t of the slice, zeros past its end
    return load_tile(wrs, t < nt ? woff + (unsigned)t * LW_KT : LW_OOB);
  };

  // x staging: thread -> 16 B piece p of rows (tid >> 5) + 8i of a chunk.
  // The resource spans rows 0 .. M-1 from column k0 on (the binding bounds
  // the row stride); rows >= M and tiles past the slice come back as zeros.
  const int p = tid & 31;
  const int row0 = tid >> 5;
  const rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u16*>(x) + k0, 0,
      (int)(((long)(M - 1) * x_stride + (K - (long)k0)) * 2), LW_RSRC_FLAGS);
  vec4w xr[4];
  auto xfetch = [&](int c) {
    const bool kok = c * LW_CT + (p >> 4) < nt;  // the piece's tile exists
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 8 * i;
      const unsigned off = (unsigned)(((long)row * x_stride +
                                       (long)c * (LW_CT * LW_KT) + p * 8) * 2);
      xr[i] = buf_load(xrs, kok && row < M ? off : LW_OOB);
    }
  };
  auto xwrite = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<vec4w*>(
          &xs[(buf * LW_MAX_M + row0 + 8 * i) * LW_LDX + p * 16]) = xr[i];
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  // wq ring: w0 is the tile in use, w1..w3 are in flight
  xfetch(0);
  WTile w0 = wtile(0), w1 = wtile(1), w2 = wtile(2), w3 = wtile(3);
  xwrite(0);
  __syncthreads();

  // Every chunk runs both of its tiles: the second tile of an odd slice's
  // last chunk multiplies the zeros xwrite left by the zeros wtile returned.
  for (int c = 0; c < nchunks; ++c) {  // block-uniform trip count
    xfetch(c + 1);
    const unsigned char* xb =
        &xs[((c & 1) * LW_MAX_M + r) * LW_LDX + 32 * h];
#pragma unroll
    for (int tl = 0; tl < LW_CT; ++tl) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
            xb + tl * (LW_KT * 2) + 64 * u);
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
            xb + tl * (LW_KT * 2) + 64 * u + 16);
        const bf16x8 b0 = frag_fp8(w0.v[u][0], w0.v[u][1]);
        const bf16x8 b1 = frag_fp8(w0.v[u][2], w0.v[u][3]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
      }
      w0 = w1;
      w1 = w2;
      w2 = w3;
      w3 = wtile(c * LW_CT + tl + 4);
    }
    xwrite((c + 1) & 1);
    __syncthreads();
  }

  if (n >= N) return;
  const float sc = scale[n];
  // register i holds x row (i & 3) + 8 * (i >> 2) + 4h of column n
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = (i & 3) + 8 * (i >> 2) + 4 * h;
    if (m < M) {
      const float v = acc[i] * sc;
      if (part != nullptr) {
        part[((size_t)blockIdx.y * M + m) * N + n] = v;
      } else {
        const __bf16 b = (__bf16)v;
        y[(size_t)m * N + n] = __builtin_bit_cast(u16, b);
      }
    }
  }
}

// y[i] = bf16(part[0][i] + part[1][i] + ... ), slabs of MN floats, in order
__global__ __launch_bounds__(256) void linear_w8_reduce(
    const float* __restrict__ part, u16* __restrict__ y, long MN, int S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= MN) return;
  float a = part[i];
  for (int s = 1; s < S; ++s) a += part[(size_t)s * MN + i];
  const __bf16 b = (__bf16)a;
  y[i] = __builtin_bit_cast(u16, b);
}

}  // namespace

extern "C" {

// The split-K factor for an [N, K] weight: the smallest that gives each of
// the chip's 256 CUs a workgroup (more slabs only add partial traffic: the
// sweep in profiles/linear_w8.md), slices of at least four tiles, at most 8
// slabs to reduce. A function of (N, K) alone.
int kt_linear_w8_plan(long N, long K) {
  const long ct = (N + LW_BN - 1) / LW_BN;
  const long kt = K / LW_KT;
  long s = (256 + ct - 1) / ct;
  if (s > kt / 4) s = kt / 4;
  if (s > 8) s = 8;
  if (s < 1) s = 1;
  return (int)s;
}

// x: [M, K] bf16, row stride x_stride elements; wq: [N, K] e4m3 contiguous;
// scale: [N] fp32; y: [M, N] bf16 contiguous; part: [S, M, N] fp32 scratch
// when S > 1 (not read or written when S == 1). The binding has checked
// 1 <= M <= 32, K % 128 == 0, 1 <= S <= 64 and the alignments.
void kt_linear_w8(const void* x, long x_stride, const void* wq,
                  const void* scale, void* y, void* part, int M, int N, int K,
                  int S, hipStream_t stream) {
  const int kt = K / LW_KT;
  const int tps = (kt + S - 1) / S;
  const dim3 grid((unsigned)((N + LW_BN - 1) / LW_BN), (unsigned)S);
  hipLaunchKernelGGL(linear_w8_kernel, grid, dim3(LW_THREADS), 0, stream,
                     (const u16*)x, x_stride, (const unsigned char*)wq,
                     (const float*)scale, (u16*)y,
                     S > 1 ? (float*)part : (float*)nullptr, M, N, K, tps);
  if (S > 1) {
    const long MN = (long)M * N;
    hipLaunchKernelGGL(linear_w8_reduce, dim3((unsigned)((MN + 255) / 256)),
                       dim3(256), 0, stream, (const float*)part, (u16*)y, MN,
                       S);
  }
}

}  // extern "C"
