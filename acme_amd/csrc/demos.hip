// Demonstrations mixed into replay batches (DQfD, acme/agents/tf/dqfd/agent.py).
//
// The reference maps every demonstration episode to one n-step transition on the host
// (_n_step_transition_from_episode, agent.py:160-217) and lets tf.data choose, element by
// element, between the Reverb stream and that mapped dataset (sample_from_datasets,
// agent.py:116-118).  Here the episodes are device arrays (acme_demo_store) and the choice,
// the episode / first-step draw, the n-step return and the row copies of a whole batch are
// one launch (acme_demo_mix) issued behind the table's own sample + gather on the dataset's
// stream: a demonstration row overwrites the replay row the table put there, a replay row
// is not touched.
//
// Kernel shape: one workgroup per batch row (one wave when every copied row is small).
// Lane 0 makes the row's single Philox call, walks the at most n_step rewards and discounts
// of the n-step return and writes the row's scalars; the choice and the two step indices go
// to the other lanes through LDS.  A replay row's workgroup leaves before any store to the
// batch.  The three row copies (o_tm1, a_tm1, o_t) use 16-byte accesses when the row bytes
// and both base pointers allow, else 4-byte accesses (row bytes are multiples of 4).
//
// The return is f32 arithmetic in a fixed order with FP contraction off (the order is in
// include/acme_hip.h), so a numpy f32 restatement (tests/dqfd_oracle.py) gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.h"
#include "detmath.h"
#include "profiler.h"

using namespace acme;

struct acme_demo_store {
  int64_t num_episodes = 0;
  int64_t total = 0;
  int64_t obs_bytes = 0;
  int64_t act_bytes = 0;
  std::vector<int64_t> offsets;  // host copy, [E + 1]
  uint8_t* obs = nullptr;
  uint8_t* act = nullptr;
  float* rewards = nullptr;
  float* discounts = nullptr;
  int64_t* d_offsets = nullptr;
  bool uploaded = false;
};

namespace {

constexpr uint32_t kDemoTag = 0x44454D4Fu;  // "DEMO"

struct MixArgs {
  const uint8_t* obs;
  const uint8_t* act;
  const float* rewards;
  const float* discounts;
  const int64_t* offsets;
  int64_t num_episodes;
  int64_t obs_bytes, act_bytes;
  double ratio;
  int32_t n_step;
  float discount;
  uint32_t k0, k1, step_lo, step_hi;
  int64_t batch;
  uint8_t* o_tm1;
  uint8_t* a_tm1;
  float* r_t;
  float* d_t;
  uint8_t* o_t;
  uint64_t* keys;
  double* probabilities;
  int64_t* table_size;
  double* priorities;
  uint8_t* is_demo;
  int32_t obs_vec16, act_vec16;
};

template <typename V>
__device__ __forceinline__ void copy_row(const uint8_t* __restrict__ src,
                                         uint8_t* __restrict__ dst, int64_t bytes) {
  const V* s = reinterpret_cast<const V*>(src);
  V* d = reinterpret_cast<V*>(dst);
  const int64_t n = bytes / (int64_t)sizeof(V);
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
}

__device__ __forceinline__ void copy_row_any(const uint8_t* src, uint8_t* dst, int64_t bytes,
                                             int vec16) {
  if (vec16)
    copy_row<uint4>(src, dst, bytes);
  else
    copy_row<uint32_t>(src, dst, bytes);
}

// grid = batch, block = 64 or 256.
__global__ void __launch_bounds__(256) demo_mix_kernel(const MixArgs a) {
#pragma clang fp contract(off)
  __shared__ int64_t s_first, s_last;
  __shared__ int32_t s_demo;
  const int64_t j = blockIdx.x;
  if (threadIdx.x == 0) {
    const u32x4 ctr = {(uint32_t)j, a.step_lo, a.step_hi, kDemoTag};
    const u32x4 r = philox4x32_10(ctr, a.k0, a.k1);
    const int demo = u01_53(r.x, r.y) < a.ratio;
    s_demo = demo;
    if (a.is_demo) a.is_demo[j] = (uint8_t)demo;
    if (demo) {
      const int64_t e = (int64_t)(((uint64_t)r.z * (uint64_t)a.num_episodes) >> 32);
      const int64_t base = a.offsets[e];
      const int64_t L = a.offsets[e + 1] - base;  // >= 3 (checked at create)
      const int64_t first = (int64_t)(((uint64_t)r.w * (uint64_t)(L - 2)) >> 32);
      const int64_t to = first + (int64_t)a.n_step;
      const int64_t last = to < L - 1 ? to : L - 1;
      const int64_t m = last - first;  // >= 1
      const float* rew = a.rewards + base + first + 1;
      const float* dis = a.discounts + base + first;
      float g = 1.0f, c = 1.0f, disc = 1.0f, acc = 0.0f;
      for (int64_t k = 0; k < m; ++k) {
        if (k > 0) {
          g = g * a.discount;
          c = c * dis[k - 1];
        }
        disc = c * g;
        const float term = rew[k] * disc;
        acc = acc + term;
      }
      a.r_t[j] = acc;
      a.d_t[j] = disc;
      if (a.keys) a.keys[j] = ACME_DEMO_KEY;
      if (a.probabilities) a.probabilities[j] = 1.0;
      if (a.table_size) a.table_size[j] = 1;
      if (a.priorities) a.priorities[j] = 1.0;
      s_first = base + first;
      s_last = base + last;
    }
  }
  __syncthreads();
  if (!s_demo) return;  // a replay row: untouched
  const int64_t first = s_first, last = s_last;
  copy_row_any(a.obs + first * a.obs_bytes, a.o_tm1 + j * a.obs_bytes, a.obs_bytes, a.obs_vec16);
  copy_row_any(a.obs + last * a.obs_bytes, a.o_t + j * a.obs_bytes, a.obs_bytes, a.obs_vec16);
  copy_row_any(a.act + first * a.act_bytes, a.a_tm1 + j * a.act_bytes, a.act_bytes, a.act_vec16);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

void free_device(acme_demo_store* s) {
  if (s->obs) (void)hipFree(s->obs);
  if (s->act) (void)hipFree(s->act);
  if (s->rewards) (void)hipFree(s->rewards);
  if (s->discounts) (void)hipFree(s->discounts);
  if (s->d_offsets) (void)hipFree(s->d_offsets);
  s->obs = s->act = nullptr;
  s->rewards = s->discounts = nullptr;
  s->d_offsets = nullptr;
  s->uploaded = false;
}

}  // namespace

extern "C" {

int acme_demo_store_create(int64_t num_episodes, const int64_t* offsets, int64_t obs_row_bytes,
                           int64_t action_row_bytes, acme_demo_store** out) {
  ACME_CHECK_ARG(offsets && out, "null argument");
  ACME_CHECK_ARG(num_episodes >= 1, "a demonstration store needs at least one episode");
  ACME_CHECK_ARG(num_episodes <= (int64_t)1 << 31, "too many demonstration episodes");
  ACME_CHECK_ARG(obs_row_bytes >= 4 && obs_row_bytes % 4 == 0 && action_row_bytes >= 4 &&
                     action_row_bytes % 4 == 0,
                 "demonstration row bytes must be positive multiples of 4 (got %lld and %lld)",
                 (long long)obs_row_bytes, (long long)action_row_bytes);
  ACME_CHECK_ARG(offsets[0] == 0, "episode offsets must start at 0");
  for (int64_t e = 0; e < num_episodes; ++e) {
    const int64_t len = offsets[e + 1] - offsets[e];
    ACME_CHECK_ARG(len >= 3,
                   "demonstration episode %lld has %lld steps; at least 3 are needed (the "
                   "first step is drawn from [0, L - 2))",
                   (long long)e, (long long)len);
  }
  acme_demo_store* s = new acme_demo_store();
  s->num_episodes = num_episodes;
  s->total = offsets[num_episodes];
  s->obs_bytes = obs_row_bytes;
  s->act_bytes = action_row_bytes;
  s->offsets.assign(offsets, offsets + num_episodes + 1);
  *out = s;
  return ACME_OK;
}

int acme_demo_store_destroy(acme_demo_store* s) {
  if (!s) return ACME_OK;
  free_device(s);
  delete s;
  return ACME_OK;
}

int acme_demo_store_upload(acme_demo_store* s, const void* observations, const void* actions,
                           const float* rewards, const float* discounts) {
  ACME_CHECK_ARG(s && observations && actions && rewards && discounts, "null argument");
  ACME_CHECK_ARG(!s->uploaded, "the demonstration store is immutable once uploaded");
  const size_t n = (size_t)s->total;
  struct Part {
    void** dst;
    const void* src;
    size_t bytes;
  } parts[] = {{(void**)&s->obs, observations, n * (size_t)s->obs_bytes},
               {(void**)&s->act, actions, n * (size_t)s->act_bytes},
               {(void**)&s->rewards, rewards, n * sizeof(float)},
               {(void**)&s->discounts, discounts, n * sizeof(float)},
               {(void**)&s->d_offsets, s->offsets.data(), s->offsets.size() * sizeof(int64_t)}};
  for (const Part& p : parts) {
    hipError_t e = hipMalloc(p.dst, p.bytes);
    if (e == hipSuccess) e = hipMemcpy(*p.dst, p.src, p.bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      set_error("demonstration store upload of %zu bytes failed: %s", p.bytes,
                hipGetErrorString(e));
      free_device(s);
      return e == hipErrorOutOfMemory ? ACME_ERR_OOM : ACME_ERR_HIP;
    }
  }
  s->uploaded = true;
  return ACME_OK;
}

int acme_demo_mix(const acme_demo_store* s, double ratio, int32_t n_step, float discount,
                  uint64_t seed, uint64_t step_counter, int64_t batch, void* const* out_fields,
                  uint64_t* keys, double* probabilities, int64_t* table_size,
                  double* priorities, uint8_t* is_demo, void* stream) {
  ACME_CHECK_ARG(s && out_fields, "null argument");
  ACME_CHECK_ARG(s->uploaded, "the demonstration store has not been uploaded");
  ACME_CHECK_ARG(ratio >= 0.0 && ratio <= 1.0, "demonstration ratio %g is outside [0, 1]", ratio);
  ACME_CHECK_ARG(n_step >= 1, "n_step must be >= 1");
  ACME_CHECK_ARG(batch >= 1 && batch <= 0x7fffffff, "bad batch size");
  for (int f = 0; f < 5; ++f)
    ACME_CHECK_ARG(out_fields[f] && aligned4(out_fields[f]), "field %d: null or unaligned", f);
  MixArgs a;
  a.obs = s->obs;
  a.act = s->act;
  a.rewards = s->rewards;
  a.discounts = s->discounts;
  a.offsets = s->d_offsets;
  a.num_episodes = s->num_episodes;
  a.obs_bytes = s->obs_bytes;
  a.act_bytes = s->act_bytes;
  a.ratio = ratio;
  a.n_step = n_step;
  a.discount = discount;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.step_lo = (uint32_t)step_counter;
  a.step_hi = (uint32_t)(step_counter >> 32);
  a.batch = batch;
  a.o_tm1 = static_cast<uint8_t*>(out_fields[0]);
  a.a_tm1 = static_cast<uint8_t*>(out_fields[1]);
  a.r_t = static_cast<float*>(out_fields[2]);
  a.d_t = static_cast<float*>(out_fields[3]);
  a.o_t = static_cast<uint8_t*>(out_fields[4]);
  a.keys = keys;
  a.probabilities = probabilities;
  a.table_size = table_size;
  a.priorities = priorities;
  a.is_demo = is_demo;
  a.obs_vec16 = s->obs_bytes % 16 == 0 && aligned16(s->obs) && aligned16(a.o_tm1) &&
                aligned16(a.o_t);
  a.act_vec16 = s->act_bytes % 16 == 0 && aligned16(s->act) && aligned16(a.a_tm1);
  hipStream_t st = as_stream(stream);
  // Expected traffic: ratio * batch rows of two observations and an action, read and written.
  ACME_PROF("demo_mix", st, 0.0,
            2.0 * ratio * (double)batch * (double)(2 * s->obs_bytes + s->act_bytes));
  const int64_t big = s->obs_bytes > s->act_bytes ? s->obs_bytes : s->act_bytes;
  const unsigned block = big <= 1024 ? 64 : 256;
  demo_mix_kernel<<<(unsigned)batch, block, 0, st>>>(a);
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

}  // extern "C"
