// The recurrent network the IMPALA and R2D2 learners share: OAR embedding (AtariTorso or a flat
// observation, one-hot previous action, tanh previous reward) -> snt.LSTM -> head.
// RecurrentNet holds its dimensions, tensor indices and workspace; acme_impala and acme_r2d2
// derive from it and add their heads, losses and optimizer tails.  Written once here: the
// configuration checks, the tensor table and the allocations of that part, and the step's
// blocks around the LSTM unroll (the OAR projection and the W_i backward, each on the plane
// engine and on the f32 engine), which differ between the learners only in values: row
// counts and offsets, tile and split constants, buffers, profiler names.  What picks another
// kernel or instantiation per learner (the LSTM unroll's dispatch, the plane W_i weight
// gradient's engine, losses, heads, guard modes) stays in the learner.
// Included into each learner's translation unit (internal linkage, as lstm.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "conv.h"
#include "conv_p3.h"
#include "gemm.h"
#include "gemm_p3.h"
#include "gemm_x6.h"
#include "kernels.h"
#include "launch.h"
#include "learner_common.h"
#include "lstm.h"
#include "plane_guard.h"
#include "profiler.h"
#include "torso.h"

namespace acme {

struct RecurrentNet : PlaneGuard {
  std::vector<Tensor> tensors;
  int64_t flat = 0;
  std::vector<void*> allocs;
  bool atari_torso = false;
  int max_batch = 0;
  int F = 0, D = 0, H = 0, H2 = 0, A = 0;  // features, embedding, lstm, head, actions
  int t_c[6] = {-1, -1, -1, -1, -1, -1};   // torso w1 b1 w2 b2 w3 b3
  int t_wi = -1, t_wh = -1, t_b = -1;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  int64_t num_steps = 0;
  // Torso activations and their gradients (Atari torso; on the plane path x1..x3 serve the
  // debug buffers only: the planes joined to f32), the f32 engines' split-K slab.
  float *x1 = nullptr, *x2 = nullptr, *x3 = nullptr, *dz1 = nullptr, *dz2 = nullptr,
        *dz3 = nullptr;
  float* slab = nullptr;
  // LSTM unroll and BPTT.
  float *gx = nullptr, *gates = nullptr, *h = nullptr, *c = nullptr;
  float *dh = nullptr, *dgates = nullptr, *dc = nullptr;
  // One-launch unroll (lstm.h lstm_fwd_rg_kernel / lstm_bwd_rg_kernel): the forward's h_t
  // granules [2][B * H] and the backward's partial-product granules [2][rg_groups][B * H]
  // (8 B: tag | value bits), never cleared between launches (next_lstm_tags); the sticky
  // spin-timeout words; lstm_steps: per-step launches instead (tests).
  unsigned long long *xg = nullptr, *xb = nullptr;
  int rg_groups = 0;
  unsigned* tmo = nullptr;
  unsigned lstm_epoch = 0;
  bool lstm_steps = false;
  // Plane path of the Atari torso (scaled two-plane f16 MFMA, gemm_p3.h): parameter planes of
  // the torso + W_i prefix of the flat buffer, refreshed at the start of every pass;
  // activation / gradient planes; its own split-K slab; the rows of the last step.
  int64_t p3_prefix = 0;  // floats of the flat buffer split into planes (torso + W_i)
  uint16_t* wpl = nullptr;
  torso::Plane x1p{}, x2p{}, x3p{}, dz1p{}, dz2p{}, dz3p{}, dgp{};
  float* pslab = nullptr;
  int64_t last_rows = 0;
};

}  // namespace acme

namespace {

using namespace acme;
using namespace acme::conv;

constexpr int kOarSplits = 8;  // split-K of the f32 Atari OAR projection (K = 7744 + A + 1)

// Scale records both learners have: the transient activations / gradients, then the online
// parameter planes.  A learner's further records follow kScRecurrent.
enum { kScX1, kScX2, kScX3, kScDz3, kScDz2, kScDz1, kScDgates, kScParams, kScRecurrent };

inline bool atari(const RecurrentNet* l) { return l->atari_torso; }

inline int check_recurrent_config(int torso, int obs_dim, int max_batch, int lstm_size) {
  ACME_CHECK_ARG(torso == ACME_IMPALA_TORSO_ATARI || torso == ACME_IMPALA_TORSO_FLAT,
                 "unknown torso %d", torso);
  ACME_CHECK_ARG(torso == ACME_IMPALA_TORSO_ATARI || obs_dim >= 1,
                 "obs_dim must be >= 1 for the flat torso");
  ACME_CHECK_ARG(max_batch >= 1 && max_batch <= 1024, "max_batch must be in [1, 1024]");
  ACME_CHECK_ARG(lstm_size >= 8 && lstm_size % 8 == 0,
                 "lstm_size must be a positive multiple of 8");
  return ACME_OK;
}

// The dimensions, and the torso and LSTM tensors "<pre>atari_torso/...", "<pre>lstm/...".
inline void add_recurrent_tensors(RecurrentNet* l, const std::string& pre, int torso, int obs_dim,
                                  int num_actions, int lstm_size, int head_size, int max_batch) {
  l->atari_torso = torso == ACME_IMPALA_TORSO_ATARI;
  l->max_batch = max_batch;
  l->A = num_actions;
  l->H = lstm_size;
  l->H2 = head_size;
  l->F = atari(l) ? torso::kFlat : obs_dim;
  l->D = l->F + l->A + 1;
  if (atari(l)) {
    l->t_c[0] = add_tensor(l, pre + "atari_torso/conv2_d/w", {8, 8, 4, 32});
    l->t_c[1] = add_tensor(l, pre + "atari_torso/conv2_d/b", {32});
    l->t_c[2] = add_tensor(l, pre + "atari_torso/conv2_d_1/w", {4, 4, 32, 64});
    l->t_c[3] = add_tensor(l, pre + "atari_torso/conv2_d_1/b", {64});
    l->t_c[4] = add_tensor(l, pre + "atari_torso/conv2_d_2/w", {3, 3, 64, 64});
    l->t_c[5] = add_tensor(l, pre + "atari_torso/conv2_d_2/b", {64});
  }
  l->t_wi = add_tensor(l, pre + "lstm/w_i", {l->D, 4 * l->H});
  l->t_wh = add_tensor(l, pre + "lstm/w_h", {l->H, 4 * l->H});
  l->t_b = add_tensor(l, pre + "lstm/b", {4 * l->H});
}

// Workspace of the f32 path: R rows run forward, RL of them backward; the slab holds at
// least min_slab floats.
inline int alloc_recurrent(RecurrentNet* l, int64_t R, int64_t RL, int64_t min_slab) {
  const int64_t H = l->H;
  int64_t slab = min_slab;
  int rc;
  if (atari(l)) {
    slab = std::max<int64_t>({slab, torso::wgrad_slab_floats(), (int64_t)kOarSplits * R * 4 * H});
    if ((rc = dev_alloc(l, &l->x1, R * torso::kX1)) || (rc = dev_alloc(l, &l->x2, R * torso::kFlat)) ||
        (rc = dev_alloc(l, &l->x3, R * torso::kFlat)) || (rc = dev_alloc(l, &l->dz1, RL * torso::kX1)) ||
        (rc = dev_alloc(l, &l->dz2, RL * torso::kFlat)) || (rc = dev_alloc(l, &l->dz3, RL * torso::kFlat)))
      return rc;
  }
  if ((rc = dev_alloc(l, &l->slab, slab)) || (rc = dev_alloc(l, &l->gx, R * 4 * H)) ||
      (rc = dev_alloc(l, &l->gates, R * 4 * H)) || (rc = dev_alloc(l, &l->h, R * H)) ||
      (rc = dev_alloc(l, &l->c, R * H)) || (rc = dev_alloc(l, &l->dh, R * H)) ||
      (rc = dev_alloc(l, &l->dgates, RL * 4 * H)) || (rc = dev_alloc(l, &l->dc, l->max_batch * H)))
    return rc;
  return ACME_OK;
}

// Plane path: n_scales records (the shared ones first), the online parameter planes, the
// activation / gradient planes and the slab (the plane OAR projection runs oar_splits splits).
inline int alloc_recurrent_planes(RecurrentNet* l, int64_t R, int64_t RL, int n_scales,
                                  int oar_splits) {
  const int64_t N = 4 * (int64_t)l->H;
  l->p3_prefix = align64(l->tensors[l->t_wi].offset + l->tensors[l->t_wi].numel);
  int rc;
  if ((rc = scales_init(l, n_scales)) || (rc = dev_alloc(l, &l->wpl, gemm::kPlanes * l->flat)) ||
      (rc = plane_alloc(l, &l->x1p, R * torso::kX1, kScX1)) ||
      (rc = plane_alloc(l, &l->x2p, R * torso::kFlat, kScX2)) ||
      (rc = plane_alloc(l, &l->x3p, R * torso::kFlat, kScX3)) ||
      (rc = plane_alloc(l, &l->dz1p, RL * torso::kX1, kScDz1)) ||
      (rc = plane_alloc(l, &l->dz2p, RL * torso::kFlat, kScDz2)) ||
      (rc = plane_alloc(l, &l->dz3p, RL * torso::kFlat, kScDz3)) ||
      (rc = plane_alloc(l, &l->dgp, RL * N, kScDgates)) ||
      (rc = dev_alloc(l, &l->pslab, std::max<int64_t>(torso::wgrad_slab_floats_p3(),
                                                      (int64_t)oar_splits * R * N))))
    return rc;
  return ACME_OK;
}

// The one-launch unroll's zeroed exchange buffers and timeout words; groups = workgroups per
// row group of the BPTT kernel, 0: no one-launch BPTT for this shape (no xb).
inline int alloc_lstm_granules(RecurrentNet* l, int groups) {
  const int64_t BH = (int64_t)l->max_batch * l->H;
  int rc;
  l->rg_groups = groups;
  if ((rc = dev_alloc(l, &l->xg, 2 * BH)) || (rc = dev_alloc(l, &l->tmo, 4)) ||
      (groups > 0 && (rc = dev_alloc(l, &l->xb, 2 * groups * BH))))
    return rc;
  if (hipMemset(l->xg, 0, (size_t)2 * BH * 8) != hipSuccess ||
      hipMemset(l->tmo, 0, 4 * sizeof(unsigned)) != hipSuccess ||
      (l->xb && hipMemset(l->xb, 0, (size_t)2 * groups * BH * 8) != hipSuccess))
    return (set_error("hipMemset failed"), ACME_ERR_HIP);
  return ACME_OK;
}

// The granule tags of the next one-launch unroll: tag0 + t (t < 2^shift), tag0 = 2^shift x a
// per-learner launch count, so no launch can match a granule an earlier one left (the buffers
// are never cleared between launches); the buffers are cleared once the count wraps.
inline unsigned next_lstm_tags(RecurrentNet* l, hipStream_t st, int shift) {
  if (++l->lstm_epoch >= (1u << 24)) {
    l->lstm_epoch = 1;
    const size_t BH = (size_t)l->max_batch * l->H;
    (void)hipMemsetAsync(l->xg, 0, 2 * BH * 8, st);
    (void)hipMemsetAsync(l->xb, 0, 2 * l->rg_groups * BH * 8, st);
  }
  return l->lstm_epoch << shift;
}

// ---- views of the flat buffers
inline torso::Weights torso_w(const RecurrentNet* l, const float* prm) {
  return torso::Weights{P(l, prm, l->t_c[0]), P(l, prm, l->t_c[1]), P(l, prm, l->t_c[2]),
                        P(l, prm, l->t_c[3]), P(l, prm, l->t_c[4]), P(l, prm, l->t_c[5])};
}
inline torso::Grads torso_grads(const RecurrentNet* l) {
  float* gr = l->grads;
  return torso::Grads{Pm(l, gr, l->t_c[0]), Pm(l, gr, l->t_c[1]), Pm(l, gr, l->t_c[2]),
                      Pm(l, gr, l->t_c[3]), Pm(l, gr, l->t_c[4]), Pm(l, gr, l->t_c[5])};
}
// Plane view of parameter tensor t in a [2][flat] parameter plane set (scale record rec).
inline torso::Plane WP(const RecurrentNet* l, uint16_t* planes, int rec, int t) {
  return torso::Plane{planes + l->tensors[t].offset, l->flat, l->scales + rec};
}
inline torso::PWeights torso_pw(const RecurrentNet* l, const float* prm, uint16_t* planes, int rec) {
  return torso::PWeights{WP(l, planes, rec, l->t_c[0]), WP(l, planes, rec, l->t_c[2]),
                         WP(l, planes, rec, l->t_c[4]), P(l, prm, l->t_c[1]),
                         P(l, prm, l->t_c[3]), P(l, prm, l->t_c[5])};
}

// ---- the step's blocks around the LSTM unroll

// The torso + W_i planes of parameter buffer prm at record rec's scale.
inline int split_param_planes(RecurrentNet* l, const float* prm, uint16_t* planes, int rec,
                              const char* name, hipStream_t st) {
  ACME_PROF(name, st, 0.0, 8.0 * (double)l->p3_prefix);
  return launch_split_planes_lagged(prm, l->p3_prefix, planes, l->flat, l->scales + rec, st);
}

// Plane OAR projection over `rows` frames: the plane torso, feat @ W_i[0:F] on the plane
// engine (BM x BN tiles, `splits` splits), then the embedding tail (one-hot(prev a),
// tanh(prev r) rows of W_i) and the bias -> gx.
template <int BM, int BN>
int oar_forward_p3(RecurrentNet* l, const float* prm, uint16_t* planes, int rec,
                   const torso::Frames& frames, int rows, int splits, int keep_x1,
                   const int32_t* prev_a, const float* prev_r, const char* fwd_name,
                   const char* reduce_name, hipStream_t st) {
  int rc = torso::forward_p3(torso_pw(l, prm, planes, rec), frames, rows,
                             torso::PActs{l->x1p, l->x2p, l->x3p}, st, keep_x1);
  if (rc != ACME_OK) return rc;
  const int F = l->F, N = 4 * l->H;
  P3DenseFwd p;
  p.M = rows; p.N = N; p.K = F; p.k_chunk = chunk_for(F, splits);
  p.a_src = SRC(l->x3p, (int64_t)rows * F); p.ldx = F;
  p.b_src = SRC(WP(l, planes, rec, l->t_wi), (int64_t)F * N); p.slab = l->pslab;
  ACME_P3WS_GEMM(fwd_name, BM, BN, 2, 2, 32, p, splits);
  {
    ACME_PROF(reduce_name, st, 0.0, 4.0 * (splits + 1) * (double)rows * N);
    const int64_t n4 = (int64_t)rows * N / 4;
    oar_finish_kernel<<<(unsigned)ceil_div(n4, 256), 256, 0, st>>>(
        l->pslab, splits, rows, N, P(l, prm, l->t_wi) + (size_t)F * N, P(l, prm, l->t_b), prev_a,
        prev_r, l->A, l->gx);
    ACME_LAUNCH_CHECK();
  }
  return ACME_OK;
}

// f32 OAR projection over `rows` rows of obs (uint8 frames through the f32 torso, or flat
// f32 observations) -> gx; split-K with a slab reduction on the Atari torso.
inline int oar_forward_f32(RecurrentNet* l, const float* prm, const void* obs, int rows,
                           const int32_t* prev_a, const float* prev_r, const char* fwd_name,
                           const char* reduce_name, hipStream_t st) {
  const int H = l->H;
  const float* feat = static_cast<const float*>(obs);
  if (atari(l)) {
    int rc = torso::forward(torso_w(l, prm), true, obs, obs, rows, rows,
                            torso::Acts{l->x1, l->x2, l->x3}, st);
    if (rc != ACME_OK) return rc;
    feat = l->x3;
  }
  OarFwd p;
  p.M = rows; p.N = 4 * H; p.K = l->D;
  p.x = Oar{feat, l->F, l->A, prev_a, prev_r};
  p.w = P(l, prm, l->t_wi); p.bias = P(l, prm, l->t_b); p.y = l->gx;
  if (atari(l)) {
    p.k_chunk = chunk_for(p.K, kOarSplits);
    p.slab = l->slab;
    ACME_GEMM(fwd_name, 64, 64, 2, 2, 16, 1, p, kOarSplits);
    ACME_PROF(reduce_name, st, 0.0, 4.0 * (kOarSplits + 1) * (double)rows * 4 * H);
    int rc = launch_slab_reduce(l->slab, kOarSplits, (int64_t)rows * 4 * H, l->gx,
                                (int64_t)rows * 4 * H, nullptr, P(l, prm, l->t_b), 4 * H, 0, st);
    if (rc != ACME_OK) return rc;
  } else {
    p.k_chunk = p.K;
    p.slab = nullptr;
    ACME_GEMM(fwd_name, 32, 32, 1, 1, 16, 8, p, 1);
  }
  return ACME_OK;
}

// Plane W_i backward, first part: dgates of `rows` rows as planes.
inline int dgates_to_planes(RecurrentNet* l, int rows, const char* name, hipStream_t st) {
  const int N = 4 * l->H;
  ACME_PROF(name, st, 0.0, 8.0 * (double)rows * N);
  return launch_split_planes_lagged(l->dgates, (int64_t)rows * N, l->dgp.p, l->dgp.stride,
                                    l->dgp.sc, st);
}
// dW_i[0:F] = feat^T dgates (+ db) over `rows` rows from row `off` of the x3 planes: the
// problem, which each learner launches on the engine and tiles it measured best.
inline P3DenseWgrad wi_wgrad_p3(RecurrentNet* l, int rows, int64_t off) {
  const int F = l->F, N = 4 * l->H;
  P3DenseWgrad p;
  p.M = F; p.N = N; p.K = rows; p.k_chunk = rows;
  p.a_src = SRC(rows_from(l->x3p, off, F), (int64_t)rows * F); p.ldx = F;
  p.b_src = SRC(l->dgp, (int64_t)rows * N); p.out = Pm(l, l->grads, l->t_wi);
  p.bias_out = Pm(l, l->grads, l->t_b);
  return p;
}
// Plane W_i backward, the rest: the embedding tail rows of dW_i, the feature gradient masked
// by conv3's ReLU (BM x BN tiles) and the plane torso backward, over `rows` rows from row
// `off` of the forward's (frames: those rows' frames).
template <int BM, int BN>
int wi_backward_p3(RecurrentNet* l, const torso::Frames& frames, int rows, int64_t off,
                   const int32_t* prev_a, const float* prev_r, const char* tail_name,
                   const char* dgrad_name, hipStream_t st) {
  const int F = l->F, N = 4 * l->H, A = l->A;
  float* gr = l->grads;
  const torso::Plane x3s = rows_from(l->x3p, off, F);
  {
    ACME_PROF(tail_name, st, 0.0, 4.0 * (double)rows * N);
    const int tw = tail_waves(A), tc = tail_chunk(A);
    const dim3 grid((unsigned)ceil_div(N, 64), (unsigned)ceil_div(A + 1, tc));
    oar_wgrad_tail_kernel<<<grid, 64 * tw, (size_t)tw * tc * 64 * sizeof(float), st>>>(
        l->dgates, rows, N, prev_a + off, prev_r + off, A, tc,
        Pm(l, gr, l->t_wi) + (size_t)F * N);
    ACME_LAUNCH_CHECK();
  }
  {
    P3DenseDgrad p;
    p.M = rows; p.N = F; p.K = N; p.k_chunk = N;
    p.a_src = SRC(l->dgp, (int64_t)rows * N);
    p.b_src = SRC(WP(l, l->wpl, kScParams, l->t_wi), (int64_t)F * N);
    p.xprev = CP(x3s); p.ldx = F;
    p.dx = PP(l->dz3p);
    ACME_P3WS_GEMM(dgrad_name, BM, BN, 2, 2, 32, p, 1);
  }
  return torso::backward_p3(torso_pw(l, l->params, l->wpl, kScParams), torso_grads(l), frames, rows,
                            torso::PActs{rows_from(l->x1p, off, torso::kX1),
                                         rows_from(l->x2p, off, F), x3s},
                            l->dz3p, l->dz2p, l->dz1p, l->pslab, st);
}

// f32 W_i backward over `rows` rows from row `off` of obs: dW_i (+ db) over the OAR
// embedding, and on the Atari torso the feature gradient into the f32 torso backward.
inline int wi_backward_f32(RecurrentNet* l, const void* obs, int rows, int64_t off,
                           const int32_t* prev_a, const float* prev_r, const char* wgrad_name,
                           const char* dgrad_name, hipStream_t st) {
  const int H = l->H;
  float* gr = l->grads;
  const float* feat = (atari(l) ? l->x3 : static_cast<const float*>(obs)) + (size_t)off * l->F;
  OarWgrad o;
  o.M = l->D; o.N = 4 * H; o.K = rows; o.k_chunk = rows;
  o.x = Oar{feat, l->F, l->A, prev_a + off, prev_r + off};
  o.dz = l->dgates; o.out = Pm(l, gr, l->t_wi); o.bias_out = Pm(l, gr, l->t_b);
  if (atari(l)) ACME_GEMM(wgrad_name, 128, 128, 2, 2, 16, 1, o, 1);
  else ACME_GEMM(wgrad_name, 32, 32, 1, 1, 16, 8, o, 1);
  if (!atari(l)) return ACME_OK;
  DenseDgrad<true> d;  // embedding features -> conv3 dZ -> torso backward
  d.M = rows; d.N = l->F; d.K = 4 * H; d.k_chunk = 4 * H;
  d.dz = l->dgates; d.w = P(l, l->params, l->t_wi); d.xprev = feat; d.ldx = l->F;
  d.dx = l->dz3; d.act = ACT_RELU;
  ACME_GEMM(dgrad_name, 64, 128, 2, 2, 16, 1, d, 1);
  return torso::backward(torso_w(l, l->params), torso_grads(l), true,
                         static_cast<const uint8_t*>(obs) + (size_t)off * torso::kObsBytes, rows,
                         torso::Acts{l->x1 + off * torso::kX1, l->x2 + off * torso::kFlat,
                                     l->x3 + off * torso::kFlat},
                         l->dz3, l->dz2, l->dz1, l->slab, st);
}

// One learner step, step(apply).  A plane step on newly bound parameters first calibrates
// the plane scales: forward + backward passes without the update (the first at the current
// scales, whose maxima are measured before the split; each ends with the rescale).  Four
// passes: the input-gradient chain dgates -> dz3 -> dz2 -> dz1 is four tensors deep, and a
// tensor computed from planes that underflowed at their initial scale measures 0 until its
// input is calibrated (as the DQN learner's calibrate_scales).  Overflows at the initial
// scales are expected and cleared, and a calibration pass's LSTM timeout is not the step's.
template <class Step>
int calibrate_then_step(RecurrentNet* l, bool plane_step, hipStream_t st, Step step) {
  int rc = ACME_OK;
  if (plane_step && !l->scales_ok) {
    for (int pass = 0; pass < 4 && rc == ACME_OK; ++pass) rc = step(false);
    if (rc != ACME_OK) return rc;
    if ((rc = calibration_done(l, st)) != ACME_OK) return rc;
    if (l->tmo) ACME_HIP_TRY(hipMemsetAsync(l->tmo, 0, sizeof(unsigned), st));
  }
  if ((rc = step(true)) != ACME_OK) return rc;
  l->num_steps += 1;
  return ACME_OK;
}

// The debug buffers x1 / x2 / x3 after a plane step: the planes of the last step's rows
// joined into the f32 buffer.  Other names: nothing to do.
inline int join_torso_planes(const RecurrentNet* l, const char* name) {
  const struct {
    const char* n;
    float* x;
    torso::Plane pl;
    int64_t per_row;
  } tab[] = {{"x1", l->x1, l->x1p, torso::kX1},
             {"x2", l->x2, l->x2p, torso::kFlat},
             {"x3", l->x3, l->x3p, torso::kFlat}};
  for (const auto& q : tab)
    if (strcmp(q.n, name) == 0) {
      ACME_HIP_TRY(hipDeviceSynchronize());
      int rc = launch_join_planes(q.pl.p, q.pl.stride, l->last_rows * q.per_row, q.x, q.pl.sc, 0);
      if (rc != ACME_OK) return rc;
      ACME_HIP_TRY(hipDeviceSynchronize());
    }
  return ACME_OK;
}

}  // namespace
