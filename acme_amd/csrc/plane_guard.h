// Step guard and plane-scale state of a learner on the f16 plane engine (dqn.hip, impala.hip,
// r2d2_learner.hip): the StepGuard (kernels.h) with the pinned mirror of its skipped count,
// the scale records (gemm_p3.h PScale) of the plane tensors with their sticky overflow flag,
// and the bodies of the exports that read or restore them.  A learner derives from
// PlaneGuard; the template helpers allocate through its `allocs` (learner_common.h).
// Also the views of a plane tensor (torso.h Plane) as the engines take them, for the
// learners and torso.hip.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "common.h"
#include "gemm_p3.h"
#include "kernels.h"
#include "learner_common.h"
#include "torso.h"

namespace acme {

// Views of a plane tensor as the engines take them: a kernel's read-only / writable planes,
// an operand source over the first `elems` elements of each plane, the rows from `row` on.
inline gemm::CPlanes CP(const torso::Plane& x) { return gemm::CPlanes{x.p, x.stride, x.sc}; }
inline gemm::Planes PP(const torso::Plane& x) { return gemm::Planes{x.p, x.stride, x.sc}; }
inline gemm::PlaneSrc SRC(const torso::Plane& x, int64_t elems) {
  return gemm::PlaneSrc{x.p, x.stride, (int32_t)(2 * elems), x.sc};
}
inline torso::Plane rows_from(const torso::Plane& x, int64_t row, int64_t per_row) {
  return torso::Plane{x.p + row * per_row, x.stride, x.sc};
}

struct PlaneGuard {
  StepGuard* guard = nullptr;
  int64_t* host_skipped = nullptr;  // pinned mirror of guard->skipped (read without a sync)
  gemm::PScale* scales = nullptr;   // n_scales records (null: the learner has no plane path)
  int* overflow = nullptr;          // sticky: a plane write overflowed f16
  bool scales_ok = false;           // the records are calibrated for the bound parameters
  int n_scales = 0;
};

// The zeroed guard and its pinned host mirror.  vseq starts at "no verdict" (all ones, as the
// host ring's entries): zero reads as "verdict 0: applied", and the first step's priority
// write-back, which waits for verdict 0, would take it for its own before the rescale
// workgroup has decided.
template <class L>
int guard_create(L* l) {
  int rc = dev_alloc(l, &l->guard, 1);
  if (rc != ACME_OK) return rc;
  if (hipMemset(l->guard, 0, sizeof(StepGuard)) != hipSuccess ||
      hipMemset(&l->guard->vseq, 0xFF, sizeof(uint32_t)) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&l->host_skipped), sizeof(int64_t),
                    hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
    return (set_error("step guard allocation failed"), ACME_ERR_HIP);
  *l->host_skipped = 0;
  return ACME_OK;
}

inline void guard_destroy(PlaneGuard* g) {
  if (g->host_skipped) (void)hipHostFree(g->host_skipped);
  g->host_skipped = nullptr;
}

// n scale records at w = r = wi = rl = 1 with zero amax slots, record i raising the guard
// word flag_of(i); the overflow flag cleared.  The first call allocates them.
template <class L, class F>
int scales_init(L* l, int n, F flag_of) {
  int rc;
  if (!l->scales && ((rc = dev_alloc(l, &l->scales, n)) || (rc = dev_alloc(l, &l->overflow, 1))))
    return rc;
  l->n_scales = n;
  std::vector<gemm::PScale> init(n);
  std::memset(init.data(), 0, init.size() * sizeof(gemm::PScale));
  for (int i = 0; i < n; ++i) {
    gemm::PScale& r = init[i];
    r.w = r.r = r.wi = r.rl = 1.f;
    r.flag = flag_of(i);
  }
  if (hipMemcpy(l->scales, init.data(), init.size() * sizeof(gemm::PScale),
                hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(l->overflow, 0, sizeof(int)) != hipSuccess)
    return (set_error("scale record init failed"), ACME_ERR_HIP);
  return ACME_OK;
}
// Every record on the online step's word.
template <class L>
int scales_init(L* l, int n) {
  return scales_init(l, n, [l](int) { return &l->guard->on; });
}

// A two-plane tensor of `count` elements bound to scale record rec.
template <class L>
int plane_alloc(L* l, torso::Plane* x, int64_t count, int rec) {
  const int64_t stride = align64(count);
  uint16_t* p = nullptr;
  int rc = dev_alloc(l, &p, gemm::kPlanes * stride);
  if (rc != ACME_OK) return rc;
  *x = torso::Plane{p, stride, l->scales + rec};
  return ACME_OK;
}

// Scale state = (w, r, wi, rl) of every record, host floats (the *_scale_state exports).
inline int scale_state(const PlaneGuard* g, float* out, int32_t capacity, int32_t* count) {
  ACME_CHECK_ARG(g && count, "null argument");
  *count = g->scales ? 4 * g->n_scales : 0;
  if (!g->scales || !out) return ACME_OK;
  ACME_CHECK_ARG(capacity >= 4 * g->n_scales, "scale state needs %d floats", 4 * g->n_scales);
  ACME_HIP_TRY(hipDeviceSynchronize());
  for (int i = 0; i < g->n_scales; ++i)
    ACME_HIP_TRY(hipMemcpy(out + 4 * i, g->scales + i, 4 * sizeof(float), hipMemcpyDeviceToHost));
  return ACME_OK;
}

inline int set_scale_state(PlaneGuard* g, const float* in, int32_t count) {
  ACME_CHECK_ARG(g && in, "null argument");
  ACME_CHECK_ARG(g->scales && count == 4 * g->n_scales, "scale state of %d floats expected, got %d",
                 g->scales ? 4 * g->n_scales : 0, count);
  for (int i = 0; i < 4 * g->n_scales; ++i) {
    int e;
    const float m = std::frexp(in[i], &e);
    ACME_CHECK_ARG(m == 0.5f, "scale state entries must be powers of two");
  }
  ACME_HIP_TRY(hipDeviceSynchronize());
  for (int i = 0; i < g->n_scales; ++i)
    ACME_HIP_TRY(hipMemcpy(g->scales + i, in + 4 * i, 4 * sizeof(float), hipMemcpyHostToDevice));
  g->scales_ok = true;
  return ACME_OK;
}

inline int plane_overflow(PlaneGuard* g, int32_t* overflow, int32_t reset) {
  ACME_CHECK_ARG(g && overflow, "null argument");
  *overflow = 0;
  if (!g->overflow) return ACME_OK;
  ACME_HIP_TRY(hipDeviceSynchronize());
  int v = 0;
  ACME_HIP_TRY(hipMemcpy(&v, g->overflow, sizeof(int), hipMemcpyDeviceToHost));
  *overflow = v != 0;
  if (reset) ACME_HIP_TRY(hipMemset(g->overflow, 0, sizeof(int)));
  return ACME_OK;
}

inline int64_t skipped_steps(const PlaneGuard* g) {
  if (!g || !g->host_skipped) return 0;
  return *reinterpret_cast<volatile const int64_t*>(g->host_skipped);
}

// The guard as the device holds it once all queued work is done.
inline int read_guard(const PlaneGuard* g, StepGuard* out) {
  ACME_HIP_TRY(hipDeviceSynchronize());
  ACME_HIP_TRY(hipMemcpy(out, g->guard, sizeof(*out), hipMemcpyDeviceToHost));
  return ACME_OK;
}

// Adam's count of applied updates (a restored checkpoint's).
inline int set_applied(PlaneGuard* g, int64_t n) {
  ACME_HIP_TRY(hipDeviceSynchronize());
  ACME_HIP_TRY(hipMemcpy(&g->guard->applied, &n, sizeof(n), hipMemcpyHostToDevice));
  return ACME_OK;
}

// A calibration finished: the overflows and guard flags its passes raised at the initial
// scales are expected and cleared (the guard's counts are kept).
inline int calibration_done(PlaneGuard* g, hipStream_t st) {
  ACME_HIP_TRY(hipMemsetAsync(g->overflow, 0, sizeof(int), st));
  ACME_HIP_TRY(hipMemsetAsync(g->guard, 0, offsetof(StepGuard, applied), st));
  g->scales_ok = true;
  return ACME_OK;
}

}  // namespace acme
