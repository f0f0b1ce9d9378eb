// CK-tile FMHA forward instantiation for the Llama training shape:
// bf16, head_dim 128, causal, batch mode, GQA, LSE output (training).
//
// composable_kernel's ck_tile FMHA is AMD's optimized attention (the
// header-only form of the AITER kernels); like hipBLASLt for GEMM this is
// the library path — we instantiate the exact variant the model needs and
// pair it with torch's AITER backward in ops.flash_attention.
// (Upstream dispatch `fmha_fwd()` is codegen at CK build time and is not
// shipped in /opt/rocm, so we instantiate the kernel template directly.)
#include <cstdlib>
#include <cstring>
#include <ck_tile/core.hpp>
#include <ck_tile/host/kernel_launch.hpp>
#include <ck_tile/ops/epilogue.hpp>
#include <ck_tile/ops/fmha.hpp>
#include <ck_tile/ops/fmha_fwd_v3_impl.hpp>

#include "kt_launchers.h"

namespace {

using qkv_t = ck_tile::bf16_t;

// hdim-128 bf16 tile config (CK codegen default for this head dim):
// M0=128 N0=128 K0=32 N1=128 K1=32 K0L=128; 4 warps; 32x32x16 warp gemm.
using FmhaShape = ck_tile::TileFmhaShape<
    ck_tile::sequence<128, 128, 32, 128, 32, 128>,
    ck_tile::sequence<4, 1, 1>, ck_tile::sequence<32, 32, 16>,
    ck_tile::sequence<4, 1, 1>, ck_tile::sequence<32, 32, 16>,
    true /* V row-major */>;

using FmhaTraits = ck_tile::TileFmhaTraits<
    true /* kPadSeqLenQ (async pipeline requires the padded views) */,
    true /* kPadSeqLenK */,
    true /* kPadHeadDimQ */,
    true /* kPadHeadDimV */,
    false /* kHasLogitsSoftCap */,
    ck_tile::BlockAttentionBiasEnum::NO_BIAS,
    false /* kHasBiasGrad */,
    true /* kStoreLSE: training */,
    false /* kHasDropout */,
    false /* kDoFp8StaticQuant */>;

using FmhaMask = ck_tile::SimplifiedGenericAttentionMask<true /* masking */>;

using FmhaPipelineProblem = ck_tile::BlockFmhaPipelineProblem<
    qkv_t /* Q */, qkv_t /* K */, qkv_t /* V */,
    float /* Sacc */, float /* SMPLCompute */,
    qkv_t /* Bias */, uint8_t /* RandValOutput */,
    float /* LSE */, qkv_t /* P */, float /* Oacc */, qkv_t /* O */,
    FmhaShape,
    false /* kIsGroupMode */,
    ck_tile::StandardAttention,
    FmhaMask,
    false /* kUseTrLoad */,
    FmhaTraits>;

using FmhaPipeline = ck_tile::BlockFmhaPipelineQRKSVSAsync<FmhaPipelineProblem>;

using FmhaEpilogue = ck_tile::Default2DEpilogue<
    ck_tile::Default2DEpilogueProblem<float, qkv_t, false /* kPadM */,
                                      false /* kPadN */>>;

using Kernel = ck_tile::FmhaFwdKernel<FmhaPipeline, FmhaEpilogue>;

using FmhaPipelineProblemTr = ck_tile::BlockFmhaPipelineProblem<
    qkv_t, qkv_t, qkv_t, float, float, qkv_t, uint8_t, float, qkv_t, float,
    qkv_t, FmhaShape, false, ck_tile::StandardAttention, FmhaMask,
    true /* kUseTrLoad: gfx950 ds_read_tr path */, FmhaTraits>;
using FmhaPipelineTr = ck_tile::BlockFmhaPipelineQRKSVSAsync<FmhaPipelineProblemTr>;
using KernelTr = ck_tile::FmhaFwdKernel<FmhaPipelineTr, FmhaEpilogue>;

struct FmhaStrides {
  // element strides along (seqlen, head, batch) per tensor
  long q_s, q_h, q_b;
  long k_s, k_h, k_b;
  long v_s, v_h, v_b;
  long o_s, o_h, o_b;
};

template <typename K>
void run_fmha(const void* q, const void* k, const void* v, void* o,
              void* lse, int B, int Hq, int Hkv, int S, float scale,
              const FmhaStrides& st, hipStream_t stream) {
  const ck_tile::index_t D = 128;
  auto kargs = K::MakeKargs(
      q, k, v, nullptr, nullptr, lse, o, S, S, D, D, Hq, Hq / Hkv, scale,
      1.0f, 1.0f, 0.0f,
      (ck_tile::index_t)st.q_s, (ck_tile::index_t)st.k_s,
      (ck_tile::index_t)st.v_s, 0, 0, (ck_tile::index_t)st.o_s,
      (ck_tile::index_t)st.q_h, (ck_tile::index_t)st.k_h,
      (ck_tile::index_t)st.v_h, 0, 0, S, (ck_tile::index_t)st.o_h,
      (ck_tile::index_t)st.q_b, (ck_tile::index_t)st.k_b,
      (ck_tile::index_t)st.v_b, 0, 0, (ck_tile::index_t)Hq * S,
      (ck_tile::index_t)st.o_b, -1, 0,
      (ck_tile::index_t)ck_tile::GenericAttentionMaskEnum::MASK_FROM_TOP_LEFT,
      0.0f, false, std::make_tuple<uint64_t, uint64_t>(0, 0));
  dim3 grid = K::GridSize(B, Hq, S, D, false);
  ck_tile::stream_config cfg{};
  cfg.stream_id_ = stream;
  cfg.cold_niters_ = 0;
  cfg.nrepeat_ = 1;
  ck_tile::launch_kernel(cfg, ck_tile::make_kernel<K::kBlockPerCu>(
                                  K{}, grid, K::kBlockSize, 0, kargs));
}

// --- fmha v3 (the AITER schedule: 8 warps, M0=256, bf16) with LSE -------
// the public fmha_fwd_v3() API hard-codes lse_ptr = nullptr; the kernel
// itself supports kStoreLSE, so instantiate it directly for training.
using V3Shape = ck_tile::TileFmhaShape<
    ck_tile::sequence<256, 32, 128, 128, 32, 128>,
    ck_tile::sequence<8, 1, 1>, ck_tile::sequence<32, 32, 16>,
    ck_tile::sequence<8, 1, 1>, ck_tile::sequence<32, 32, 16>, true>;
using V3Traits = ck_tile::TileFmhaFwdV3Traits<true,  // kPadSeqLenQ
                                              true,  // kPadSeqLenK
                                              false, // kPadHeadDimQ
                                              false, // kPadHeadDimV
                                              true,  // kStoreLSE (training)
                                              -1>;
using V3Mask = ck_tile::GenericAttentionMask<true, false>;
using V3Problem = ck_tile::BlockFmhaFwdV3PipelineProblem<
    qkv_t, qkv_t, qkv_t, float, float, float /* lse */, qkv_t /* P */,
    float /* Oacc */, qkv_t /* O */, V3Shape, false /* varlen */, V3Mask,
    V3Traits>;
using V3Pipeline = ck_tile::BlockFmhaFwdV3Pipeline<V3Problem>;
using V3Epilogue = ck_tile::Default2DEpilogue<
    ck_tile::Default2DEpilogueProblem<float, qkv_t, true, true, true>>;
using V3Kernel = ck_tile::FmhaFwdV3Kernel<V3Pipeline, V3Epilogue>;

}  // namespace

extern "C" void kt_attn_fwd_v3(const void* q, const void* k, const void* v,
                               void* o, void* lse, int B, int Hq, int Hkv,
                               int S, float scale, const long* strides,
                               hipStream_t stream) {
  FmhaStrides st;
  memcpy(&st, strides, sizeof(st));
  const ck_tile::index_t D = 128;
  auto kargs = V3Kernel::MakeKargs(
      q, k, v, lse, o, S, S, D, D, Hq, Hq / Hkv, scale,
      (ck_tile::index_t)st.q_s, (ck_tile::index_t)st.k_s,
      (ck_tile::index_t)st.v_s, (ck_tile::index_t)st.o_s,
      (ck_tile::index_t)st.q_h, (ck_tile::index_t)st.k_h,
      (ck_tile::index_t)st.v_h, S /* nhead_stride_lse */,
      (ck_tile::index_t)st.o_h, (ck_tile::index_t)st.q_b,
      (ck_tile::index_t)st.k_b, (ck_tile::index_t)st.v_b,
      (ck_tile::index_t)Hq * S /* batch_stride_lse */,
      (ck_tile::index_t)st.o_b, -1 /* window_left */, 0 /* window_right */,
      (ck_tile::index_t)ck_tile::GenericAttentionMaskEnum::MASK_FROM_TOP_LEFT,
      [] {  // XCD-aware tile remapping (0=none, 1/2=swizzles); 2 is the
           // aiter default for this shape — KT_V3_REMAP overrides for
           // on-box sweeps without a recompile
        const char* r = std::getenv("KT_V3_REMAP");
        return (ck_tile::index_t)(r ? atoi(r) : 2);
      }(),
      nullptr, nullptr);
  dim3 grid = V3Kernel::GridSize(B, Hq, S, D);
  constexpr dim3 blocks = V3Kernel::BlockSize();
  ck_tile::stream_config cfg{};
  cfg.stream_id_ = stream;
  cfg.cold_niters_ = 0;
  cfg.nrepeat_ = 1;
  ck_tile::launch_kernel(cfg,
                         ck_tile::make_kernel<V3Kernel::kBlockPerCu>(
                             V3Kernel{}, grid, blocks, 0, kargs));
}

extern "C" void kt_attn_fwd_ck_tr(const void* q, const void* k,
                                  const void* v, void* o, void* lse, int B,
                                  int Hq, int Hkv, int S, float scale,
                                  const long* strides, hipStream_t stream) {
  FmhaStrides st;
  memcpy(&st, strides, sizeof(st));
  run_fmha<KernelTr>(q, k, v, o, lse, B, Hq, Hkv, S, scale, st, stream);
}

extern "C" void kt_attn_fwd_ck(const void* q, const void* k, const void* v,
                               void* o, void* lse, int B, int Hq, int Hkv,
                               int S, float scale, const long* strides,
                               hipStream_t stream) {
  FmhaStrides st;
  memcpy(&st, strides, sizeof(st));
  run_fmha<Kernel>(q, k, v, o, lse, B, Hq, Hkv, S, scale, st, stream);
}
