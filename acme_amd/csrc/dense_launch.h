// Host-side launches of the dense layers on the register-operand engine (gemm_direct.h), shared
// by the learners built from plain dense layers (d4pg.hip: D4PG, DDPG, MPO, DMPO, CRR; az.hip):
// the forward of one layer, and the backward launches that run a layer's input gradient together
// with the weight gradients whose dZ is already written.  Every function returns an acme_status
// and records its profiler section.
#pragma once

#include <algorithm>
#include <vector>

#include "common.h"
#include "conv.h"
#include "gemm.h"
#include "gemm_direct.h"
#include "launch.h"
#include "profiler.h"

namespace acme {
namespace dense {

using conv::DenseDgrad;
using conv::DenseFwd;
using conv::DenseWgrad;

// Small GEMMs: 32x32 output tiles, 8 waves per block splitting the reduction, so a
// 512 x 512 x 512 layer runs 2048 waves: the register-operand engine (gemm_direct.h, one
// load burst per wave; round 5: 0.196 -> 0.164 ms per step against the staged f32 engine of
// gemm.h, profiles/r05/ab/d4pg_direct_*.log).
#define D4_LAUNCH(prob, nz) gemm::launch_direct(prob, nz, (prob).K, st)

// Dense layer forward y = act(x @ W + b) over `rows` rows.
inline int dense_fwd(const char* name, const float* x, int rows, int K, const float* w,
                     const float* b, int N, int act, float* y, hipStream_t st) {
  if (K % 4 == 0 && N % 4 == 0) {
    DenseFwd<true> p;
    p.M = rows; p.N = N; p.K = K; p.k_chunk = K;
    p.x = x; p.x2 = x; p.split_b = rows; p.ldx = K;
    p.w = w; p.bias = b; p.y = y; p.act = act; p.slab = nullptr;
    ACME_DIRECT_GEMM(name, p);
  } else {
    DenseFwd<false> p;
    p.M = rows; p.N = N; p.K = K; p.k_chunk = K;
    p.x = x; p.x2 = x; p.split_b = rows; p.ldx = K;
    p.w = w; p.bias = b; p.y = y; p.act = act; p.slab = nullptr;
    ACME_DIRECT_GEMM(name, p);
  }
  return ACME_OK;
}

// The same layer of two evaluations (rows0 / rows1 rows, weights w0 / w1, outputs y0 / y1) as
// the two sub-problems of one launch; each output row is computed as by dense_fwd.
template <bool VEC>
inline int dense_fwd_pair_impl(const char* name, const float* x0, int rows0, const float* w0,
                               const float* b0, float* y0, const float* x1, int rows1,
                               const float* w1, const float* b1, float* y1, int K, int N, int act,
                               hipStream_t st) {
  DenseFwd<VEC> q[2];
  const float* xs[2] = {x0, x1};
  const float* ws[2] = {w0, w1};
  const float* bs[2] = {b0, b1};
  float* ys[2] = {y0, y1};
  const int rs[2] = {rows0, rows1};
  for (int i = 0; i < 2; ++i) {
    q[i].M = rs[i]; q[i].N = N; q[i].K = K; q[i].k_chunk = K;
    q[i].x = xs[i]; q[i].x2 = xs[i]; q[i].split_b = rs[i]; q[i].ldx = K;
    q[i].w = ws[i]; q[i].bias = bs[i]; q[i].y = ys[i]; q[i].act = act; q[i].slab = nullptr;
  }
  auto p = gemm::make_zset(q);
  ACME_PROF_PEAK(name, st, 2.0 * (double)(rows0 + rows1) * N * K, 0.0, 157.3);
  hipError_t e = D4_LAUNCH(p, 2);
  if (e != hipSuccess) {
    set_error("gemm launch failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    return ACME_ERR_HIP;
  }
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

// One layer over two row sources that share its weights: y[0, rows0) from x0 and
// y[rows0, rows0 + rows1) from x1, without a concatenation copy.  The direct engine describes
// an operand as one buffer (DenseFwd's a_op), so the two sources are the pair's two
// sub-problems.  The engine reads W by columns whatever N is; only the x rows' vector loads
// need K % 4 == 0.
inline int dense_fwd_two(const char* name, const float* x0, int rows0, const float* x1, int rows1,
                         int K, const float* w, const float* b, int N, int act, float* y,
                         hipStream_t st) {
  float* y1 = y + (size_t)rows0 * N;
  return K % 4 == 0
             ? dense_fwd_pair_impl<true>(name, x0, rows0, w, b, y, x1, rows1, w, b, y1, K, N, act, st)
             : dense_fwd_pair_impl<false>(name, x0, rows0, w, b, y, x1, rows1, w, b, y1, K, N, act, st);
}

// One backward launch (gemm::ZMulti): a layer's input gradient together with the weight
// gradients whose dZ is already written (the same layer's, the previous LayerNorm's first
// layer).  The problems read finished tensors and write disjoint outputs, so the weight
// gradients fill CUs the input gradient leaves idle instead of running as launches of
// their own.
struct BwdGroup {
  std::vector<DenseDgrad<true>> dg;
  std::vector<DenseDgrad<false>> dgn;  // widths not a multiple of 4 (the heads)
  std::vector<DenseWgrad<true>> wg;
  std::vector<DenseWgrad<false>> wgn;
};

// dW = X^T dZ over `rows` rows, db = column sums of dZ.
inline void add_wgrad(BwdGroup& g, const float* x, int rows, int Nin, const float* dz, int Nout,
                      float* dw, float* db) {
  auto fill = [&](auto& p) {
    p.M = Nin; p.N = Nout; p.K = rows; p.k_chunk = rows;
    p.x = x; p.ldx = Nin; p.dz = dz; p.out = dw; p.bias_out = db;
  };
  if (Nin % 4 == 0 && Nout % 4 == 0) {
    DenseWgrad<true> p;
    fill(p);
    g.wg.push_back(p);
  } else {
    DenseWgrad<false> p;
    fill(p);
    g.wgn.push_back(p);
  }
}

// dX = act'(xprev) * (dZ @ W^T): dz [rows][Nout], W [Nin][Nout], xprev/dx [rows][Nin].
inline void add_dgrad(BwdGroup& g, const float* dz, int rows, int Nout, const float* w, int Nin,
                      const float* xprev, int act, float* dx) {
  auto fill = [&](auto& p) {
    p.M = rows; p.N = Nin; p.K = Nout; p.k_chunk = Nout;
    p.dz = dz; p.w = w; p.xprev = xprev; p.ldx = Nin; p.dx = dx; p.act = act;
  };
  if (Nout % 4 == 0 && Nin % 4 == 0) {
    DenseDgrad<true> p;
    fill(p);
    g.dg.push_back(p);
  } else {
    DenseDgrad<false> p;
    fill(p);
    g.dgn.push_back(p);
  }
}

constexpr int kZ = 3;  // sub-problems of one type per backward launch

template <class Q>
bool fill_zset(gemm::ZSet<Q, kZ>& z, int& n, const std::vector<Q>& qs, int& tiles, int& count,
               double& flops, int& kmax) {
  if (qs.size() > (size_t)kZ) return false;
  n = (int)qs.size();
  if (!qs.empty()) static_cast<Q&>(z) = qs[0];
  for (int i = 0; i < n; ++i) {
    z.sub[i] = qs[i];
    tiles = std::max(tiles, (int)(ceil_div(qs[i].M, 32) * ceil_div(qs[i].N, 32)));
    flops += 2.0 * qs[i].M * (double)qs[i].N * qs[i].K;
    kmax = std::max(kmax, qs[i].K);
  }
  count += n;
  return true;
}

template <class Q0, class... R>
bool fill_multi(gemm::ZMulti<gemm::ZSet<Q0, kZ>, gemm::ZSet<R, kZ>...>& m, int& tiles,
                int& count, double& flops, int& kmax, const std::vector<Q0>& q0,
                const std::vector<R>&... r) {
  if (!fill_zset(m.s, m.n, q0, tiles, count, flops, kmax)) return false;
  if constexpr (sizeof...(R) > 0) return fill_multi(m.rest, tiles, count, flops, kmax, r...);
  return true;
}

// One launch over the problems of the given types (gemm_f32_multi_kernel instantiated for
// exactly these types: its LDS and registers are their maximum).
template <class... Q>
int launch_multi(const char* name, hipStream_t st, const std::vector<Q>&... qs) {
  gemm::ZMulti<gemm::ZSet<Q, kZ>...> m;
  int tiles = 0, count = 0, kmax = 0;
  double flops = 0.0;
  if (!fill_multi(m, tiles, count, flops, kmax, qs...))
    return (set_error("too many GEMMs in one backward launch"), ACME_ERR_INVALID);
  if (count == 0) return ACME_OK;
  ACME_PROF_PEAK(name, st, flops, 0.0, 157.3);
  const hipError_t e = gemm::launch_direct_multi(m, tiles, count, kmax, st);
  if (e != hipSuccess) {
    set_error("gemm launch failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    return ACME_ERR_HIP;
  }
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

// The hidden layers' launches carry 4-aligned problems only; the heads' and the first
// layers' the rest.
inline int launch_bwd(const char* name, BwdGroup& g, hipStream_t st) {
  int rc;
  // (The concat first layer's weight gradient is two DenseWgrad problems, ln_backward.)
  if (g.dgn.empty() && g.wgn.empty())
    rc = launch_multi(name, st, g.dg, g.wg);
  else if (g.dg.empty() && g.wg.empty())
    rc = launch_multi(name, st, g.dgn, g.wgn);
  else
    rc = launch_multi(name, st, g.dg, g.wg, g.dgn, g.wgn);
  g = BwdGroup{};
  return rc;
}

}  // namespace dense
}  // namespace acme
