// Profiled GEMM launches of the learners (dqn.hip, impala.hip, r2d2_learner.hip, torso.hip,
// d4pg.hip): a profiler section around the launch of one engine, or the caller returns
// ACME_ERR_HIP.  The macros expand in a function that returns an acme_status and whose stream
// is `st`; the caller includes the header of the engine it launches (gemm_x6.h, gemm_p3.h,
// gemm_p3i.h, gemm_direct.h).
#pragma once

#include "common.h"
#include "profiler.h"

namespace acme {

// Split-K chunk size (a multiple of 32, every engine's deepest reduction stage) for `splits`
// splits of K.
inline int chunk_for(int K, int splits) {
  int c = (int)ceil_div(K, splits);
  return (int)ceil_div(c, 32) * 32;
}

}  // namespace acme

// Algorithmic FLOPs of a problem with M, N, K (2 x MACs).
#define ACME_MNK_FLOPS(prob) (2.0 * (double)(prob).M * (double)(prob).N * (double)(prob).K)

// Section `name` (flops, the engine's TFLOP/s peak) around `launch`, a hipError_t expression.
#define ACME_LAUNCH_GEMM(name, flops, peak, launch)                                           \
  do {                                                                                        \
    ACME_PROF_PEAK(name, st, flops, 0.0, peak);                                               \
    hipError_t _e = (launch);                                                                 \
    if (_e != hipSuccess) {                                                                   \
      ::acme::set_error("gemm launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__,    \
                        __LINE__);                                                            \
      return ACME_ERR_HIP;                                                                    \
    }                                                                                         \
  } while (0)

// f32 engines (gemm_x6.h launch_matmul): BM x BN tiles of WM x WN waves, reduction stage
// depth BKV, WK waves splitting the reduction.  _F: the caller's own FLOP count.
#define ACME_GEMM_F(name, flops, BM, BN, WM, WN, BKV, WK, prob, splits)                       \
  ACME_LAUNCH_GEMM(name, flops, (gemm::matmul_peak_tflops<WK, decltype(prob)>()),             \
                   (gemm::launch_matmul<BM, BN, WM, WN, BKV, WK>(prob, splits, st)))
#define ACME_GEMM(name, BM, BN, WM, WN, BKV, WK, prob, splits)                                \
  ACME_GEMM_F(name, ACME_MNK_FLOPS(prob), BM, BN, WM, WN, BKV, WK, prob, splits)

// Plane engine (gemm_p3.h): single-role, warp-specialised (producer and consumer waves,
// fragment reads one k16 step ahead) and LDS-DMA with ST stages.
#define ACME_P3_GEMM_F(name, flops, BM, BN, WM, WN, BKV, prob, splits)                        \
  ACME_LAUNCH_GEMM(name, flops, gemm::p3_peak_tflops<decltype(prob)>(),                       \
                   (gemm::launch_gemm_p3<BM, BN, WM, WN, BKV>(prob, splits, st)))
#define ACME_P3_GEMM(name, BM, BN, WM, WN, BKV, prob, splits)                                 \
  ACME_P3_GEMM_F(name, ACME_MNK_FLOPS(prob), BM, BN, WM, WN, BKV, prob, splits)
#define ACME_P3WS_GEMM(name, BM, BN, WM, WN, BKV, prob, splits)                               \
  ACME_LAUNCH_GEMM(name, ACME_MNK_FLOPS(prob), gemm::p3_peak_tflops<decltype(prob)>(),        \
                   (gemm::launch_gemm_p3ws<BM, BN, WM, WN, BKV, true>(prob, splits, st)))
#define ACME_P3G_GEMM(name, BM, BN, WM, WN, BKV, ST, prob, splits)                            \
  ACME_LAUNCH_GEMM(name, ACME_MNK_FLOPS(prob), gemm::p3_peak_tflops<decltype(prob)>(),        \
                   (gemm::launch_gemm_p3g<BM, BN, WM, WN, BKV, ST>(prob, splits, st)))

// Register-operand engine for small f32 layers (gemm_direct.h: 32 x 32 tiles, 8 waves
// splitting the reduction, each lane's k run in one load burst).
#define ACME_DIRECT_GEMM(name, prob)                                                          \
  ACME_LAUNCH_GEMM(name, ACME_MNK_FLOPS(prob), kPeakF32MfmaTflops,                            \
                   gemm::launch_direct(prob, 1, (prob).K, st))
