// Demonstration sequences mixed into sequence batches (R2D3, acme/agents/tf/r2d3/agent.py).
//
// The reference maps every demonstration episode to one zero-padded window of
// sequence_length steps on the host (_sequence_from_episode, agent.py:163-235) and lets
// tf.data choose, element by element, between the Reverb stream and that mapped dataset
// (sample_from_datasets, agent.py:104-106).  Here the episodes are device arrays
// (acme_seq_demo_store: K per-step fields, densely packed) and the choice, the episode /
// window draw and the row writes of a whole batch are one launch (acme_seq_demo_mix) issued
// behind the table's own sample + gather on the dataset's stream: a demonstration row
// overwrites the replay row the table put there, a replay row is not touched.
//
// Kernel shape: a sequence row is large (121 steps of 28,224 bytes are 3.4 MB) and only a
// few rows of a batch are demonstrations, so the grid is (chunks, batch): workgroup (c, j)
// owns bytes [c * kChunk, (c + 1) * kChunk) of every field of row j, and `chunks` covers the
// largest field.  Every workgroup makes its row's Philox call itself (it is the same in every
// lane, so no LDS, no barrier, no communication between workgroups and no dependence on
// launch order); the workgroups of a replay row leave before any store to the batch.  Fields
// of at most kChunk bytes, the flag field and the scalars are thereby chunk 0's alone.
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

struct acme_seq_demo_store {
  int64_t num_episodes = 0;
  int64_t total = 0;
  int32_t num_fields = 0;
  int64_t step_bytes[ACME_SEQ_DEMO_MAX_FIELDS] = {};
  uint8_t* fields[ACME_SEQ_DEMO_MAX_FIELDS] = {};
  std::vector<int64_t> offsets;  // host copy, [E + 1]
  int64_t* d_offsets = nullptr;
  bool uploaded = false;
};

namespace {

constexpr uint32_t kSeqDemoTag = 0x53455144u;  // "SEQD"
constexpr int64_t kChunk = 16384;              // bytes of a field one workgroup writes
constexpr int kBlock = 256;

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
  const int64_t* offsets;
  int64_t num_episodes;
  double ratio;
  int64_t period, T;
  uint32_t k0, k1, step_lo, step_hi;
  uint64_t* keys;
  double* probabilities;
  int64_t* table_size;
  double* priorities;
  uint8_t* is_demo;
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
  const u32x4 ctr = {(uint32_t)j, a.step_lo, a.step_hi, kSeqDemoTag};
  const u32x4 r = philox4x32_10(ctr, a.k0, a.k1);
  const bool demo = u01_53(r.x, r.y) < a.ratio;
  const bool lead = c == 0 && threadIdx.x == 0;
  if (lead && a.is_demo) a.is_demo[j] = (uint8_t)demo;
  if (!demo) return;  // a replay row: untouched
  const int64_t e = (int64_t)(((uint64_t)r.z * (uint64_t)a.num_episodes) >> 32);
  const int64_t base = a.offsets[e];
  const int64_t L = a.offsets[e + 1] - base;  // in [1, 2^31] (checked at create)
  const int64_t pos = (int64_t)(((uint64_t)r.w * (uint64_t)L) >> 32);
  const int64_t first = pos / a.period * a.period;
  const int64_t to = first + a.T < L ? first + a.T : L;
  if (lead) {
    if (a.keys) a.keys[j] = ACME_DEMO_KEY;
    if (a.probabilities) a.probabilities[j] = 1.0;
    if (a.table_size) a.table_size[j] = 1;
    if (a.priorities) a.priorities[j] = 1.0;
  }
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

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// The widest of 16, 4, 1 that divides `unit` and `stride` and that both pointers allow.
int32_t access_width(int64_t unit, int64_t stride, const void* dst, const void* src) {
  const uintptr_t bits = (uintptr_t)unit | (uintptr_t)stride | addr(dst) | addr(src);
  return bits % 16 == 0 ? 16 : bits % 4 == 0 ? 4 : 1;
}

void free_device(acme_seq_demo_store* s) {
  for (int32_t f = 0; f < ACME_SEQ_DEMO_MAX_FIELDS; ++f) {
    if (s->fields[f]) (void)hipFree(s->fields[f]);
    s->fields[f] = nullptr;
  }
  if (s->d_offsets) (void)hipFree(s->d_offsets);
  s->d_offsets = nullptr;
  s->uploaded = false;
}

}  // namespace

extern "C" {

int acme_seq_demo_store_create(int64_t num_episodes, const int64_t* offsets, int32_t num_fields,
                               const int64_t* step_bytes, acme_seq_demo_store** out) {
  ACME_CHECK_ARG(offsets && step_bytes && out, "null argument");
  ACME_CHECK_ARG(num_episodes >= 1, "a demonstration store needs at least one episode");
  ACME_CHECK_ARG(num_episodes <= (int64_t)1 << 31, "too many demonstration episodes");
  ACME_CHECK_ARG(num_fields >= 1 && num_fields <= ACME_SEQ_DEMO_MAX_FIELDS,
                 "a sequence demonstration store holds 1 to %d per-step fields (got %d)",
                 ACME_SEQ_DEMO_MAX_FIELDS, (int)num_fields);
  for (int32_t f = 0; f < num_fields; ++f)
    ACME_CHECK_ARG(step_bytes[f] >= 1 && step_bytes[f] <= (int64_t)1 << 40,
                   "field %d: step bytes must be >= 1 (got %lld)", (int)f,
                   (long long)step_bytes[f]);
  ACME_CHECK_ARG(offsets[0] == 0, "episode offsets must start at 0");
  for (int64_t e = 0; e < num_episodes; ++e) {
    const int64_t len = offsets[e + 1] - offsets[e];
    ACME_CHECK_ARG(len >= 1 && len <= (int64_t)1 << 31,
                   "demonstration episode %lld has %lld steps; at least 1 is needed",
                   (long long)e, (long long)len);
  }
  acme_seq_demo_store* s = new acme_seq_demo_store();
  s->num_episodes = num_episodes;
  s->total = offsets[num_episodes];
  s->num_fields = num_fields;
  for (int32_t f = 0; f < num_fields; ++f) s->step_bytes[f] = step_bytes[f];
  s->offsets.assign(offsets, offsets + num_episodes + 1);
  *out = s;
  return ACME_OK;
}

int acme_seq_demo_store_destroy(acme_seq_demo_store* s) {
  if (!s) return ACME_OK;
  free_device(s);
  delete s;
  return ACME_OK;
}

int acme_seq_demo_store_upload(acme_seq_demo_store* s, const void* const* fields) {
  ACME_CHECK_ARG(s && fields, "null argument");
  ACME_CHECK_ARG(!s->uploaded, "the demonstration store is immutable once uploaded");
  for (int32_t f = 0; f < s->num_fields; ++f) ACME_CHECK_ARG(fields[f], "field %d: null", (int)f);
  hipError_t e = hipSuccess;
  size_t bytes = 0;
  for (int32_t f = 0; f < s->num_fields && e == hipSuccess; ++f) {
    bytes = (size_t)s->total * (size_t)s->step_bytes[f];
    e = hipMalloc((void**)&s->fields[f], bytes);
    if (e == hipSuccess) e = hipMemcpy(s->fields[f], fields[f], bytes, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    bytes = s->offsets.size() * sizeof(int64_t);
    e = hipMalloc((void**)&s->d_offsets, bytes);
    if (e == hipSuccess)
      e = hipMemcpy(s->d_offsets, s->offsets.data(), bytes, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    set_error("sequence demonstration store upload of %zu bytes failed: %s", bytes,
              hipGetErrorString(e));
    free_device(s);
    return e == hipErrorOutOfMemory ? ACME_ERR_OOM : ACME_ERR_HIP;
  }
  s->uploaded = true;
  return ACME_OK;
}

int acme_seq_demo_mix(const acme_seq_demo_store* s, double ratio, int64_t period,
                      int64_t sequence_length, uint64_t seed, uint64_t step_counter,
                      int64_t batch, void* const* out_fields, int32_t num_out_fields,
                      const int64_t* out_row_bytes, const int64_t* out_logical_bytes,
                      uint64_t* keys, double* probabilities, int64_t* table_size,
                      double* priorities, uint8_t* is_demo, void* stream) {
  ACME_CHECK_ARG(s && out_fields && out_row_bytes && out_logical_bytes, "null argument");
  ACME_CHECK_ARG(s->uploaded, "the demonstration store has not been uploaded");
  ACME_CHECK_ARG(ratio >= 0.0 && ratio <= 1.0, "demonstration ratio %g is outside [0, 1]", ratio);
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
  SeqMixArgs a;
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
  a.offsets = s->d_offsets;
  a.num_episodes = s->num_episodes;
  a.ratio = ratio;
  a.period = period;
  a.T = T;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.step_lo = (uint32_t)step_counter;
  a.step_hi = (uint32_t)(step_counter >> 32);
  a.keys = keys;
  a.probabilities = probabilities;
  a.table_size = table_size;
  a.priorities = priorities;
  a.is_demo = is_demo;
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
