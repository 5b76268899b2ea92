// The per-row selection rule of acme_epsilon_greedy (include/acme_hip.h), shared by the kernels
// that pick an action from a row they hold in registers: kernels.hip (epsilon_greedy_kernel,
// duel_head_act_kernel) and bc.hip (bc_act_fused_kernel).  One definition, so every caller draws
// the same action from the same (row, seed, step_counter) and the same values.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "detmath.h"

namespace acme {

// ---- epsilon-greedy selection of the acting paths (include/acme_hip.h acme_epsilon_greedy)
constexpr uint32_t kActTag = 0x52324143u;  // "R2AC"
constexpr int kActSlots = 16;              // A <= 1024: action lane + 64 i in slot i

// max(a, b) with NaNs ignored (NaN only when both are).
__device__ __forceinline__ float nanmax(float a, float b) {
  return b != b ? a : (a != a || b > a ? b : a);
}

// One row's action, by the wave that holds the row: lane l has q[l + 64 i] in qv[i].  All 64
// lanes call it (ballots) and get the same result.  One Philox call per row:
// explore iff u01_53(r.x, r.y) < epsilon, then (r.z A) >> 32; else the ((r.w n) >> 32)-th of
// the n actions equal to the row's maximum (NaNs ignored), ascending; no maximum: action 0.
__device__ __forceinline__ int select_action(const float (&qv)[kActSlots], int A, int lane,
                                             uint32_t row, double epsilon, uint64_t seed,
                                             uint64_t step) {
  const u32x4 r = philox4x32_10(u32x4{row, (uint32_t)step, (uint32_t)(step >> 32), kActTag},
                                (uint32_t)seed, (uint32_t)(seed >> 32));
  if (u01_53(r.x, r.y) < epsilon) return (int)(((uint64_t)r.z * (uint64_t)A) >> 32);
  const int slots = (A + 63) >> 6;
  float m = NAN;
#pragma unroll
  for (int i = 0; i < kActSlots; ++i)
    if (i < slots && lane + 64 * i < A) m = nanmax(m, qv[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o, 64));
  int n = 0;
#pragma unroll
  for (int i = 0; i < kActSlots; ++i)
    if (i < slots) n += __popcll(__ballot(lane + 64 * i < A && qv[i] == m));
  if (n == 0) return 0;
  int k = (int)(((uint64_t)r.w * (uint64_t)n) >> 32);
  int a = 0;
  bool found = false;
#pragma unroll
  for (int i = 0; i < kActSlots; ++i)
    if (i < slots && !found) {
      unsigned long long mask = __ballot(lane + 64 * i < A && qv[i] == m);
      const int c = __popcll(mask);
      if (k < c) {
        for (int s = 0; s < k; ++s) mask &= mask - 1;  // drop the k lowest members
        a = 64 * i + __ffsll((long long)mask) - 1;
        found = true;
      } else {
        k -= c;
      }
    }
  return a;
}

}  // namespace acme
