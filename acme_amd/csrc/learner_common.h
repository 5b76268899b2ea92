// What every native learner (dqn.hip, impala.hip, r2d2_learner.hip, d4pg.hip) keeps the same
// way: the tensor table of its flat parameter buffer, its device workspace allocations, and
// the lookups behind *_tensor_info and *_debug_buffer.  The helpers are templates over the
// learner type L, which has `std::vector<Tensor> tensors`, `int64_t flat` and
// `std::vector<void*> allocs`.  Beside it: launch.h (the profiled GEMM launch macros and
// chunk_for), plane_guard.h (the step guard and plane-scale state of the learners on the f16
// plane engine: dqn.hip, impala.hip, r2d2_learner.hip) and recurrent_common.h (the OAR
// embedding -> LSTM part impala.hip and r2d2_learner.hip share).
#pragma once

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "common.h"

namespace acme {

// One named tensor of the flat parameter buffer (offsets in floats, 64-float aligned).
struct Tensor {
  std::string name;
  int64_t offset = 0, numel = 0;
  int ndim = 0;
  int64_t shape[4] = {1, 1, 1, 1};
};

inline int64_t align64(int64_t x) { return (x + 63) & ~int64_t(63); }

// Appends a tensor at the end of the flat buffer; returns its index.
template <class L>
int add_tensor(L* l, const std::string& name, std::initializer_list<int64_t> shape) {
  Tensor t;
  t.name = name;
  t.ndim = (int)shape.size();
  t.numel = 1;
  int i = 0;
  for (int64_t s : shape) {
    t.shape[i++] = s;
    t.numel *= s;
  }
  t.offset = l->flat;
  l->flat = align64(l->flat + t.numel);
  l->tensors.push_back(t);
  return (int)l->tensors.size() - 1;
}

// Device workspace owned by the learner (freed from l->allocs when it is destroyed).
template <class L, class T>
int dev_alloc(L* l, T** p, int64_t count) {
  void* q = nullptr;
  if (hipMalloc(&q, std::max<int64_t>(count, 1) * sizeof(T)) != hipSuccess) {
    set_error("hipMalloc of %lld bytes failed", (long long)(count * sizeof(T)));
    return ACME_ERR_OOM;
  }
  l->allocs.push_back(q);
  *p = static_cast<T*>(q);
  return ACME_OK;
}

// Tensor t inside a flat buffer (params, target, grads, ...).
template <class L>
inline const float* P(const L* l, const float* base, int t) {
  return base + l->tensors[t].offset;
}
template <class L>
inline float* Pm(const L* l, float* base, int t) {
  return base + l->tensors[t].offset;
}

// The body of every *_tensor_info export.
template <class L>
int tensor_info(const L* l, int32_t i, int64_t* offset, int64_t* numel, int32_t* ndim,
                int64_t* shape4, const char** name) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(i >= 0 && i < (int32_t)l->tensors.size(), "tensor index %d out of range", i);
  const Tensor& t = l->tensors[i];
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (ndim) *ndim = t.ndim;
  if (shape4)
    for (int k = 0; k < 4; ++k) shape4[k] = t.shape[k];
  if (name) *name = t.name.c_str();
  return ACME_OK;
}

// One row of a *_debug_buffer table: a workspace buffer and its float count.
struct DebugItem {
  const char* name;
  const float* ptr;
  int64_t count;
};

template <size_t N>
int find_debug_buffer(const DebugItem (&items)[N], const char* name, const float** out,
                      int64_t* count) {
  for (const DebugItem& it : items)
    if (strcmp(it.name, name) == 0) {
      *out = it.ptr;
      *count = it.count;
      return ACME_OK;
    }
  set_error("unknown debug buffer '%s'", name);
  return ACME_ERR_INVALID;
}

}  // namespace acme
