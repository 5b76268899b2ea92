// Demonstrations mixed into replay batches: transitions (DQfD, acme/agents/tf/dqfd/agent.py)
// and sequences (R2D3, acme/agents/tf/r2d3/agent.py).
//
// The reference maps every demonstration episode on the host, to one n-step transition
// (_n_step_transition_from_episode, dqfd/agent.py:160-217) or to one zero-padded window of
// sequence_length steps (_sequence_from_episode, r2d3/agent.py:163-235), and lets tf.data
// choose, element by element, between the Reverb stream and that mapped dataset
// (sample_from_datasets, dqfd/agent.py:116-118, r2d3/agent.py:104-106).  Here the episodes are
// device arrays (acme_demo_store: K per-step fields, densely packed) and the choice, the
// episode / step draw and the row writes of a whole batch are one launch (acme_demo_mix,
// acme_seq_demo_mix) issued behind the table's own sample + gather on the dataset's stream: a
// demonstration row overwrites the replay row the table put there, a replay row is not
// touched.  Both kernels share the row's draw, the episode lookup and the SampleInfo stores
// (row_draw, episode_of, write_demo_info over MixCommon); who calls them differs.
//
// Kernel shape, transitions: one workgroup per batch row (one wave when every copied row is
// small).  Lane 0 makes the row's single Philox call, walks the at most n_step rewards and
// discounts of the n-step return and writes the row's scalars; the choice and the two step
// indices go to the other lanes through LDS.  A replay row's workgroup leaves before any
// store to the batch.  The three row copies (o_tm1, a_tm1, o_t) use 16-byte accesses when the
// row bytes and both base pointers allow, else 4-byte accesses (row bytes are multiples of 4).
//
// The return is f32 arithmetic in a fixed order with FP contraction off (the order is in
// include/acme_hip.h), so a numpy f32 restatement (tests/dqfd_oracle.py) gives the same bits.
//
// Kernel shape, sequences: a sequence row is large (121 steps of 28,224 bytes are 3.4 MB) and
// only a few rows of a batch are demonstrations, so the grid is (chunks, batch): workgroup
// (c, j) owns bytes [c * kChunk, (c + 1) * kChunk) of every field of row j, and `chunks`
// covers the largest field.  Every workgroup makes its row's Philox call itself (it is the
// same in every lane, so no LDS, no barrier, no communication between workgroups and no
// dependence on launch order); the workgroups of a replay row leave before any store to the
// batch.  Fields of at most kChunk bytes, the flag field and the scalars are thereby chunk
// 0's alone.
//
// Within its chunk a workgroup writes, per field, the window's source bytes and zeros behind
// them (copied fields), the start_of_episode byte (the flag field) or zeros (extras), in
// 16-, 4- or 1-byte accesses: the widest that divides the field's step bytes (its logical
// bytes for the flag and the extras), the row stride and every base pointer.  The source of
// a window starts at first * step_bytes, so a 3-byte step takes the byte path.
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
  int32_t num_fields = 0;
  int64_t step_bytes[ACME_DEMO_MAX_FIELDS] = {};
  uint8_t* fields[ACME_DEMO_MAX_FIELDS] = {};
  std::vector<int64_t> offsets;  // host copy, [E + 1]
  int64_t* d_offsets = nullptr;
  int64_t min_episode_steps = 1;
  bool uploaded = false;
};

namespace {

constexpr uint32_t kDemoTag = 0x44454D4Fu;     // "DEMO"
constexpr uint32_t kSeqDemoTag = 0x53455144u;  // "SEQD"
constexpr int64_t kChunk = 16384;              // bytes of a field one workgroup writes
constexpr int kBlock = 256;

// What both kernels take: the episodes, the draw's key and counter, the SampleInfo outputs.
struct MixCommon {
  const int64_t* offsets;
  int64_t num_episodes;
  double ratio;
  uint32_t k0, k1, step_lo, step_hi;
  uint64_t* keys;
  double* probabilities;
  int64_t* table_size;
  double* priorities;
  uint8_t* is_demo;
};

struct Draw {
  u32x4 r;
  bool demo;
};

// Row j's single Philox call and its choice between replay and demonstration.
__device__ __forceinline__ Draw row_draw(const MixCommon& m, int64_t j, uint32_t tag) {
  const u32x4 ctr = {(uint32_t)j, m.step_lo, m.step_hi, tag};
  const u32x4 r = philox4x32_10(ctr, m.k0, m.k1);
  return {r, u01_53(r.x, r.y) < m.ratio};
}

// The first step and the length (in [min_episode_steps, 2^31], checked at create) of the
// episode the draw's third word selects.
__device__ __forceinline__ void episode_of(const MixCommon& m, uint32_t z, int64_t* base,
                                           int64_t* L) {
  const int64_t e = (int64_t)(((uint64_t)z * (uint64_t)m.num_episodes) >> 32);
  *base = m.offsets[e];
  *L = m.offsets[e + 1] - *base;
}

__device__ __forceinline__ void write_demo_info(const MixCommon& m, int64_t j) {
  if (m.keys) m.keys[j] = ACME_DEMO_KEY;
  if (m.probabilities) m.probabilities[j] = 1.0;
  if (m.table_size) m.table_size[j] = 1;
  if (m.priorities) m.priorities[j] = 1.0;
}

// ------------------------------------------------------------------ transitions

struct MixArgs {
  MixCommon m;
  const uint8_t* obs;
  const uint8_t* act;
  const float* rewards;
  const float* discounts;
  int64_t obs_bytes, act_bytes;
  int32_t n_step;
  float discount;
  uint8_t* o_tm1;
  uint8_t* a_tm1;
  float* r_t;
  float* d_t;
  uint8_t* o_t;
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
    const Draw d = row_draw(a.m, j, kDemoTag);
    s_demo = d.demo;
    if (a.m.is_demo) a.m.is_demo[j] = (uint8_t)d.demo;
    if (d.demo) {
      int64_t base, L;  // L >= 3 (checked at the mix)
      episode_of(a.m, d.r.z, &base, &L);
      const int64_t first = (int64_t)(((uint64_t)d.r.w * (uint64_t)(L - 2)) >> 32);
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
      write_demo_info(a.m, j);
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

// -------------------------------------------------------------------- sequences

enum : int32_t { kCopy = 0, kFlag = 1, kZero = 2 };

struct OutField {
  uint8_t* dst;        // [batch][stride]
  const uint8_t* src;  // kCopy: [total][step_bytes]
  int64_t stride;      // stored bytes of a row
  int64_t logical;     // bytes of a row that are written
  int64_t step_bytes;  // kCopy only
  int32_t width;       // 16, 4 or 1
  int32_t kind;
};

struct SeqMixArgs {
  OutField f[ACME_SEQ_DEMO_MAX_OUT_FIELDS];
  int32_t num_out;
  MixCommon m;
  int64_t period, T;
};

// Bytes [lo, hi) of a row: src[i] for i < n_src, `fill` behind.  lo, hi and n_src are
// multiples of sizeof(V); four accesses per lane are in flight.
template <typename V>
__device__ __forceinline__ void put_chunk(const uint8_t* __restrict__ src, int64_t n_src,
                                          uint8_t* __restrict__ dst, int64_t lo, int64_t hi,
                                          V fill) {
  constexpr int64_t W = (int64_t)sizeof(V);
  constexpr int64_t stride = (int64_t)kBlock * W;
  for (int64_t i = lo + (int64_t)threadIdx.x * W; i < hi; i += 4 * stride) {
    V v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t at = i + u * stride;
      v[u] = fill;
      if (at < hi && at < n_src) v[u] = *reinterpret_cast<const V*>(src + at);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t at = i + u * stride;
      if (at < hi) *reinterpret_cast<V*>(dst + at) = v[u];
    }
  }
}

// grid = (chunks, batch), block = kBlock.
__global__ void __launch_bounds__(kBlock) seq_demo_mix_kernel(const SeqMixArgs a) {
  const int64_t j = blockIdx.y;
  const int64_t c = blockIdx.x;
  const Draw d = row_draw(a.m, j, kSeqDemoTag);
  const bool lead = c == 0 && threadIdx.x == 0;
  if (lead && a.m.is_demo) a.m.is_demo[j] = (uint8_t)d.demo;
  if (!d.demo) return;  // a replay row: untouched
  int64_t base, L;
  episode_of(a.m, d.r.z, &base, &L);
  const int64_t pos = (int64_t)(((uint64_t)d.r.w * (uint64_t)L) >> 32);
  const int64_t first = pos / a.period * a.period;
  const int64_t to = first + a.T < L ? first + a.T : L;
  if (lead) write_demo_info(a.m, j);
  const uint32_t flag = first == 0 ? 0x01010101u : 0u;
  const int64_t lo = c * kChunk;
  for (int32_t k = 0; k < a.num_out; ++k) {
    const OutField& f = a.f[k];
    if (lo >= f.logical) continue;
    const int64_t hi = lo + kChunk < f.logical ? lo + kChunk : f.logical;
    uint8_t* dst = f.dst + j * f.stride;
    const uint8_t* src = nullptr;
    int64_t n_src = 0;
    uint32_t fill = 0;
    if (f.kind == kCopy) {
      src = f.src + (base + first) * f.step_bytes;
      n_src = (to - first) * f.step_bytes;
    } else if (f.kind == kFlag) {
      fill = flag;
    }
    if (f.width == 16)
      put_chunk<uint4>(src, n_src, dst, lo, hi, make_uint4(fill, fill, fill, fill));
    else if (f.width == 4)
      put_chunk<uint32_t>(src, n_src, dst, lo, hi, fill);
    else
      put_chunk<uint8_t>(src, n_src, dst, lo, hi, (uint8_t)fill);
  }
}

// ------------------------------------------------------------------------- host

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// The widest of 16, 4, 1 that divides `unit` and `stride` and that every pointer allows.
int32_t access_width(int64_t unit, int64_t stride, const void* dst, const void* src,
                     const void* dst2 = nullptr) {
  const uintptr_t bits =
      (uintptr_t)unit | (uintptr_t)stride | addr(dst) | addr(src) | addr(dst2);
  return bits % 16 == 0 ? 16 : bits % 4 == 0 ? 4 : 1;
}

void free_device(acme_demo_store* s) {
  for (int32_t f = 0; f < ACME_DEMO_MAX_FIELDS; ++f) {
    if (s->fields[f]) (void)hipFree(s->fields[f]);
    s->fields[f] = nullptr;
  }
  if (s->d_offsets) (void)hipFree(s->d_offsets);
  s->d_offsets = nullptr;
  s->uploaded = false;
}

// The checks both mixes share, and the arguments both kernels take.
int mix_common(const acme_demo_store* s, double ratio, uint64_t seed, uint64_t step_counter,
               void* const* out_fields, uint64_t* keys, double* probabilities,
               int64_t* table_size, double* priorities, uint8_t* is_demo, MixCommon* m) {
  ACME_CHECK_ARG(s && out_fields, "null argument");
  ACME_CHECK_ARG(s->uploaded, "the demonstration store has not been uploaded");
  ACME_CHECK_ARG(ratio >= 0.0 && ratio <= 1.0, "demonstration ratio %g is outside [0, 1]", ratio);
  m->offsets = s->d_offsets;
  m->num_episodes = s->num_episodes;
  m->ratio = ratio;
  m->k0 = (uint32_t)seed;
  m->k1 = (uint32_t)(seed >> 32);
  m->step_lo = (uint32_t)step_counter;
  m->step_hi = (uint32_t)(step_counter >> 32);
  m->keys = keys;
  m->probabilities = probabilities;
  m->table_size = table_size;
  m->priorities = priorities;
  m->is_demo = is_demo;
  return ACME_OK;
}

}  // namespace

extern "C" {

int acme_demo_store_create(int64_t num_episodes, const int64_t* offsets, int32_t num_fields,
                           const int64_t* step_bytes, int64_t min_episode_steps,
                           acme_demo_store** out) {
  ACME_CHECK_ARG(offsets && step_bytes && out, "null argument");
  ACME_CHECK_ARG(num_episodes >= 1, "a demonstration store needs at least one episode");
  ACME_CHECK_ARG(num_episodes <= (int64_t)1 << 31, "too many demonstration episodes");
  ACME_CHECK_ARG(num_fields >= 1 && num_fields <= ACME_DEMO_MAX_FIELDS,
                 "a demonstration store holds 1 to %d per-step fields (got %d)",
                 ACME_DEMO_MAX_FIELDS, (int)num_fields);
  for (int32_t f = 0; f < num_fields; ++f)
    ACME_CHECK_ARG(step_bytes[f] >= 1 && step_bytes[f] <= (int64_t)1 << 40,
                   "field %d: step bytes must be >= 1 (got %lld)", (int)f,
                   (long long)step_bytes[f]);
  ACME_CHECK_ARG(min_episode_steps >= 1 && min_episode_steps <= (int64_t)1 << 31,
                 "min_episode_steps must be >= 1 (got %lld)", (long long)min_episode_steps);
  ACME_CHECK_ARG(offsets[0] == 0, "episode offsets must start at 0");
  for (int64_t e = 0; e < num_episodes; ++e) {
    const int64_t len = offsets[e + 1] - offsets[e];
    ACME_CHECK_ARG(len >= min_episode_steps && len <= (int64_t)1 << 31,
                   "demonstration episode %lld has %lld steps; at least %lld and at most 2^31 "
                   "are needed",
                   (long long)e, (long long)len, (long long)min_episode_steps);
  }
  acme_demo_store* s = new acme_demo_store();
  s->num_episodes = num_episodes;
  s->total = offsets[num_episodes];
  s->num_fields = num_fields;
  for (int32_t f = 0; f < num_fields; ++f) s->step_bytes[f] = step_bytes[f];
  s->offsets.assign(offsets, offsets + num_episodes + 1);
  s->min_episode_steps = min_episode_steps;
  *out = s;
  return ACME_OK;
}

int acme_demo_store_destroy(acme_demo_store* s) {
  if (!s) return ACME_OK;
  free_device(s);
  delete s;
  return ACME_OK;
}

int acme_demo_store_upload(acme_demo_store* s, const void* const* fields) {
  ACME_CHECK_ARG(s && fields, "null argument");
  ACME_CHECK_ARG(!s->uploaded, "the demonstration store is immutable once uploaded");
  const int32_t K = s->num_fields;
  for (int32_t f = 0; f < K; ++f) ACME_CHECK_ARG(fields[f], "field %d: null", (int)f);
  for (int32_t f = 0; f <= K; ++f) {  // the K fields, then the offsets
    void** dst = f < K ? (void**)&s->fields[f] : (void**)&s->d_offsets;
    const void* src = f < K ? fields[f] : s->offsets.data();
    const size_t bytes = f < K ? (size_t)s->total * (size_t)s->step_bytes[f]
                               : s->offsets.size() * sizeof(int64_t);
    hipError_t e = hipMalloc(dst, bytes);
    if (e == hipSuccess) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      set_error("demonstration store upload of %zu bytes failed: %s", bytes,
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
  ACME_CHECK_ARG(s, "null argument");
  // What this mix asks of the store's layout (no device call before these).
  const int64_t ob = s->step_bytes[0], ab = s->step_bytes[1];
  ACME_CHECK_ARG(s->num_fields == 4 && s->step_bytes[2] == 4 && s->step_bytes[3] == 4,
                 "a transition mix needs a store of four fields (observation rows, action "
                 "rows, f32 rewards, f32 discounts)");
  ACME_CHECK_ARG(ob % 4 == 0 && ab % 4 == 0,
                 "demonstration row bytes must be positive multiples of 4 (got %lld and %lld)",
                 (long long)ob, (long long)ab);
  ACME_CHECK_ARG(s->min_episode_steps >= 3,
                 "a transition mix needs a store created with min_episode_steps of at least 3 "
                 "(the first step is drawn from [0, L - 2)); this one has %lld",
                 (long long)s->min_episode_steps);
  MixArgs a;
  if (int rc = mix_common(s, ratio, seed, step_counter, out_fields, keys, probabilities,
                          table_size, priorities, is_demo, &a.m))
    return rc;
  ACME_CHECK_ARG(n_step >= 1, "n_step must be >= 1");
  ACME_CHECK_ARG(batch >= 1 && batch <= 0x7fffffff, "bad batch size");
  for (int f = 0; f < 5; ++f)
    ACME_CHECK_ARG(out_fields[f] && access_width(4, 4, out_fields[f], nullptr) >= 4,
                   "field %d: null or unaligned", f);
  a.obs = s->fields[0];
  a.act = s->fields[1];
  a.rewards = reinterpret_cast<const float*>(s->fields[2]);
  a.discounts = reinterpret_cast<const float*>(s->fields[3]);
  a.obs_bytes = ob;
  a.act_bytes = ab;
  a.n_step = n_step;
  a.discount = discount;
  a.o_tm1 = static_cast<uint8_t*>(out_fields[0]);
  a.a_tm1 = static_cast<uint8_t*>(out_fields[1]);
  a.r_t = static_cast<float*>(out_fields[2]);
  a.d_t = static_cast<float*>(out_fields[3]);
  a.o_t = static_cast<uint8_t*>(out_fields[4]);
  a.obs_vec16 = access_width(ob, ob, a.o_tm1, a.obs, a.o_t) == 16;
  a.act_vec16 = access_width(ab, ab, a.a_tm1, a.act) == 16;
  hipStream_t st = as_stream(stream);
  // Expected traffic: ratio * batch rows of two observations and an action, read and written.
  ACME_PROF("demo_mix", st, 0.0, 2.0 * ratio * (double)batch * (double)(2 * ob + ab));
  const unsigned block = (ob > ab ? ob : ab) <= 1024 ? 64 : 256;
  demo_mix_kernel<<<(unsigned)batch, block, 0, st>>>(a);
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

int acme_seq_demo_mix(const acme_demo_store* s, double ratio, int64_t period,
                      int64_t sequence_length, uint64_t seed, uint64_t step_counter,
                      int64_t batch, void* const* out_fields, int32_t num_out_fields,
                      const int64_t* out_row_bytes, const int64_t* out_logical_bytes,
                      uint64_t* keys, double* probabilities, int64_t* table_size,
                      double* priorities, uint8_t* is_demo, void* stream) {
  SeqMixArgs a;
  if (int rc = mix_common(s, ratio, seed, step_counter, out_fields, keys, probabilities,
                          table_size, priorities, is_demo, &a.m))
    return rc;
  ACME_CHECK_ARG(out_row_bytes && out_logical_bytes, "null argument");
  ACME_CHECK_ARG(period >= 1, "period must be >= 1");
  ACME_CHECK_ARG(sequence_length >= 1 && sequence_length <= (int64_t)1 << 20,
                 "bad sequence length");
  ACME_CHECK_ARG(batch >= 1 && batch <= 65535, "bad batch size (1 to 65535 rows)");
  const int32_t K = s->num_fields;
  ACME_CHECK_ARG(num_out_fields > K && num_out_fields <= ACME_SEQ_DEMO_MAX_OUT_FIELDS,
                 "a sequence batch has the store's %d fields, start_of_episode and at most %d "
                 "fields in all (got %d)",
                 (int)K, ACME_SEQ_DEMO_MAX_OUT_FIELDS, (int)num_out_fields);
  const int64_t T = sequence_length;
  int64_t largest = 0;
  double written = 0.0, read = 0.0;
  for (int32_t f = 0; f < num_out_fields; ++f) {
    const int64_t want = f < K ? T * s->step_bytes[f] : f == K ? T : out_logical_bytes[f];
    ACME_CHECK_ARG(out_fields[f], "field %d: null", (int)f);
    ACME_CHECK_ARG(out_logical_bytes[f] == want && want >= 0 && want <= out_row_bytes[f],
                   "field %d: %lld logical bytes in rows of %lld, expected %lld", (int)f,
                   (long long)out_logical_bytes[f], (long long)out_row_bytes[f],
                   (long long)want);
    OutField& o = a.f[f];
    o.dst = static_cast<uint8_t*>(out_fields[f]);
    o.src = f < K ? s->fields[f] : nullptr;
    o.stride = out_row_bytes[f];
    o.logical = want;
    o.step_bytes = f < K ? s->step_bytes[f] : 0;
    o.kind = f < K ? kCopy : f == K ? kFlag : kZero;
    o.width = access_width(f < K ? o.step_bytes : want, o.stride, o.dst, o.src);
    if (want > largest) largest = want;
    written += (double)want;
    if (f < K) read += (double)want;
  }
  for (int32_t f = num_out_fields; f < ACME_SEQ_DEMO_MAX_OUT_FIELDS; ++f) a.f[f] = OutField{};
  a.num_out = num_out_fields;
  a.period = period;
  a.T = T;
  hipStream_t st = as_stream(stream);
  // Expected traffic: ratio * batch rows, every field written and the copied ones read (an
  // upper bound: a padded window reads less).
  ACME_PROF("seq_demo_mix", st, 0.0, ratio * (double)batch * (written + read));
  const int64_t chunks = largest > kChunk ? (largest + kChunk - 1) / kChunk : 1;
  ACME_CHECK_ARG(chunks <= 0x7fffffff, "row too large");
  seq_demo_mix_kernel<<<dim3((unsigned)chunks, (unsigned)batch), kBlock, 0, st>>>(a);
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

}  // extern "C"
