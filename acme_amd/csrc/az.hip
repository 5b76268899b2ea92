// AlphaZero-style learner step and network evaluation of the MCTS agent for MI355X: the
// replacement of AZLearner._step (acme/agents/tf/mcts/learning.py:53-82) and of the network call
// in MCTSActor._forward (acting.py:67-77) behind the C ABI (include/acme_hip.h, acme_az_*).
//
// Network: snt.Sequential([snt.Flatten(), snt.nets.MLP(hidden, activate_final),
// PolicyValueHead(A)]): dense ReLU trunk, then logits = h Wp + bp [A] and v = h wv + bv.
//
// One step = one stream, no host synchronisation, 2 nl + 2 launches for nl trunk layers:
//   trunk forward over the 2B rows [o_t; o_tp1], one launch per layer on the register-operand
//     dense engine (the first layer reads its two sources as two sub-problems of one launch);
//   az_head_loss_kernel: both heads of row b, v' of row b + B, the max-subtracted softmax
//     cross-entropy against pi, the TD error, dloss/dlogits, dloss/dv and the gradient at the
//     last trunk layer's pre-activation; the batch means of the two losses summed in block order;
//   backward over the B o_t rows: the heads' weight gradients ride with the last trunk layer's
//     launch, then one launch per layer (input gradient + weight gradient);
//   snt.Adam over the flat buffer (launch_adam, t = num_steps + 1).
// Nothing uses a float atomic: every sum has a fixed order, so a step repeats bit for bit.
//
// Evaluation (the actor's latency path: MCTS calls it once per tree node, one row at a time):
// az_eval_fused_kernel runs the whole network in ONE launch for up to ACME_AZ_FUSED_MAX_ROWS
// rows of layers up to ACME_AZ_FUSED_MAX_WIDTH wide; past either, the trunk goes layer by layer
// through the dense engine and az_eval_head_kernel forms the heads and the softmax.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "conv.h"
#include "dense_launch.h"
#include "kernels.h"
#include "learner_common.h"
#include "profiler.h"

using namespace acme;
using namespace acme::conv;
using namespace acme::dense;

namespace {

constexpr int kHeadRows = 4;  // rows per 256-thread block of the head kernels: one wave each
constexpr int kEvRows = 4;    // rows per block of the fused evaluation
constexpr int kEvWidth = ACME_AZ_FUSED_MAX_WIDTH;

}  // namespace

struct acme_az {
  acme_az_config cfg;
  std::vector<Tensor> tensors;
  int64_t flat = 0;
  std::vector<void*> allocs;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  int64_t num_steps = 0;
  int nl = 0;
  int w[ACME_MAX_MLP_LAYERS] = {}, b[ACME_MAX_MLP_LAYERS] = {};  // mlp/linear_i
  int pw = -1, pb = -1, vw = -1, vb = -1;                        // the two heads
  float* h[ACME_MAX_MLP_LAYERS] = {};   // [2 max_batch][hidden[i]] trunk activations
  float* dz[ACME_MAX_MLP_LAYERS] = {};  // [max_batch][hidden[i]] pre-activation gradients
  float *logits = nullptr, *dlogits = nullptr;        // [max_batch][A]
  float *val = nullptr;                               // [2 max_batch]: v, then v'
  float *td = nullptr, *dv = nullptr;                 // [max_batch]
  float* part = nullptr;                              // [blocks][2] loss partials
  unsigned* ticket = nullptr;                         // blocks of the head kernel that finished
  float* loss_tmp = nullptr;                          // [3] outputs the caller did not ask for
  float* eh[2] = {};                                  // [max_eval_rows][widest] layered evaluation
  int64_t last_batch = 0;                             // B of the last step (debug buffers)
};

namespace {

int pow2_at_least(int x) {
  int p = 1;
  while (p < x) p *= 2;
  return p;
}

// ------------------------------------------------------------------ the two heads of one row
// One wave, row h [H] (global or LDS): lane = g * AP + a with AP = A rounded up to a power of
// two and G = 64 / AP k-groups.  Group g sums k = g, g + G, ... of logit a (W[k, :] read
// coalesced over a), the groups are summed by a butterfly over the lane bits above AP, so every
// lane ends with the logit of action lane % AP (-inf for a >= A).  The value: lane-strided
// partial sums, then the butterfly of wave_sum.
__device__ __forceinline__ float value_row(const float* h, const float* __restrict__ wv,
                                           const float* __restrict__ bv, int H, int lane) {
  float acc = 0.f;
#pragma unroll 4
  for (int k = lane; k < H; k += 64) acc = fmaf(h[k], wv[k], acc);
  return wave_sum(acc) + bv[0];
}

__device__ __forceinline__ float logit_row(const float* h, const float* __restrict__ wp,
                                           const float* __restrict__ bp, int H, int A, int AP,
                                           int lane) {
  const int a = lane & (AP - 1);
  const int G = 64 / AP, g = lane / AP;
  const bool on = a < A;
  const int col = on ? a : 0;  // lanes past A read column 0 and drop it
  float acc = 0.f;
#pragma unroll 4
  for (int k = g; k < H; k += G) acc = fmaf(h[k], wp[(size_t)k * A + col], acc);
  for (int o = AP; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
  return on ? acc + bp[col] : -INFINITY;
}

// softmax over the lanes < A of a wave (x = -inf elsewhere): maximum, exponential, sum.
struct Softmax {
  float m, e, s;
};
__device__ __forceinline__ Softmax wave_softmax(float x, bool on) {
  Softmax o;
  o.m = wave_max(on ? x : -INFINITY);
  o.e = on ? expf(x - o.m) : 0.f;
  o.s = wave_sum(o.e);
  return o;
}

// ------------------------------------------------------------------ heads + loss + gradients
struct HeadLossArgs {
  const float* h;  // [2B][H] trunk output: the o_t rows, then the o_tp1 rows
  const float *wp, *bp, *wv, *bv;
  const float *r, *d, *pi;  // [B], [B], [B][A]
  int B, H, A, AP, relu_final;
  float discount;
  float *logits, *dlogits;  // [B][A]
  float* val;               // [2B]
  float *td, *dv;           // [B]
  float* dh;                // [B][H] gradient at the last trunk layer's pre-activation
  float* part;              // [gridDim.x][2]
  unsigned* ticket;
  float *loss, *value_loss, *policy_loss;
};

__global__ void __launch_bounds__(256) az_head_loss_kernel(const HeadLossArgs a) {
  __shared__ float red[kHeadRows][2];
  __shared__ unsigned last_s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * kHeadRows + w;
  float vl = 0.f, ce = 0.f;
  if (row < a.B) {  // uniform per wave
    const float* h = a.h + (size_t)row * a.H;
    const float logit = logit_row(h, a.wp, a.bp, a.H, a.A, a.AP, lane);
    const float v = value_row(h, a.wv, a.bv, a.H, lane);
    const float v2 = value_row(a.h + (size_t)(row + a.B) * a.H, a.wv, a.bv, a.H, lane);
    const bool on = lane < a.A;  // the first k-group holds the row's logits
    const Softmax sm = wave_softmax(logit, on);
    const float pi = on ? a.pi[(size_t)row * a.A + lane] : 0.f;
    const float logp = on ? (logit - sm.m) - logf(sm.s) : 0.f;
    ce = -wave_sum(pi * logp);
    const float sum_pi = wave_sum(pi);
    const float invB = 1.f / (float)a.B;
    const float dl = on ? ((sm.e / sm.s) * sum_pi - pi) * invB : 0.f;
    const float td = (a.r[row] + (a.discount * a.d[row]) * v2) - v;
    vl = td * td;
    const float dv = -2.f * td * invB;
    if (on) {
      a.logits[(size_t)row * a.A + lane] = logit;
      a.dlogits[(size_t)row * a.A + lane] = dl;
    }
    if (lane == 0) {
      a.val[row] = v;
      a.val[row + a.B] = v2;
      a.td[row] = td;
      a.dv[row] = dv;
    }
    // dh[k] = dv wv[k] + sum_j dl_j Wp[k, j], masked by the final ReLU when there is one
    // (dl_j from lane j by readlane: j is uniform).
    for (int k = lane; k < a.H; k += 64) {
      float s = dv * a.wv[k];
      const float* wr = a.wp + (size_t)k * a.A;
      for (int j = 0; j < a.A; ++j) {
        const float dj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dl), j));
        s = fmaf(dj, wr[j], s);
      }
      if (a.relu_final) s = act_bwd(ACT_RELU, h[k], s);
      a.dh[(size_t)row * a.H + k] = s;
    }
  }
  // The batch means: the block's four rows in order, then the blocks' partials by the block
  // that finishes last (agent-scope stores, a release before the ticket, an acquire after it).
  if (lane == 0) {
    red[w][0] = vl;
    red[w][1] = ce;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float sv = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    const float sc = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    __hip_atomic_store(&a.part[2 * blockIdx.x], sv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.part[2 * blockIdx.x + 1], sc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    const unsigned t =
        __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last_s = t == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (last_s != 0u && w == 0) {  // uniform per block, then per wave
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    float sv = 0.f, sc = 0.f;
    for (int i = lane; i < (int)gridDim.x; i += 64) {
      sv += __hip_atomic_load(&a.part[2 * i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sc += __hip_atomic_load(&a.part[2 * i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    sv = wave_sum(sv);
    sc = wave_sum(sc);
    if (lane == 0) {
      const float value_loss = sv / (float)a.B, policy_loss = sc / (float)a.B;
      *a.value_loss = value_loss;
      *a.policy_loss = policy_loss;
      *a.loss = value_loss + policy_loss;
      __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------ evaluation
// The heads and the softmax of `rows` rows of trunk output: one wave per row.
struct EvalHeadArgs {
  const float* h;  // [rows][H]
  const float *wp, *bp, *wv, *bv;
  int rows, H, A, AP;
  float *probs, *value;
};

__device__ __forceinline__ void eval_head_row(const float* h, const EvalHeadArgs& a, int row,
                                              int lane) {
  const float logit = logit_row(h, a.wp, a.bp, a.H, a.A, a.AP, lane);
  const float v = value_row(h, a.wv, a.bv, a.H, lane);
  const bool on = lane < a.A;
  const Softmax sm = wave_softmax(logit, on);
  if (on) a.probs[(size_t)row * a.A + lane] = sm.e / sm.s;
  if (lane == 0) a.value[row] = v;
}

__global__ void __launch_bounds__(256) az_eval_head_kernel(const EvalHeadArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kHeadRows + (threadIdx.x >> 6);
  if (row >= a.rows) return;  // uniform per wave, no barrier below
  eval_head_row(a.h + (size_t)row * a.H, a, row, lane);
}

// The whole network in one launch: kEvRows rows per 256-thread block, activations ping-pong in
// LDS.  Layer K -> N (N <= kEvWidth): thread t owns output column n = t % NP (NP = N rounded up
// to a power of two) and k-group g = t / NP of G = 256 / NP; it reads W[k, n] coalesced over n
// for k = g, g + G, ... and each x[r][k] as an LDS broadcast; the G partials are summed in
// group order through LDS.  Then one wave per row forms the heads and the softmax.
struct EvalFusedArgs {
  const float* obs;  // [rows][D]
  int rows, D, nl, relu_final;
  int sizes[ACME_MAX_MLP_LAYERS];
  const float* w[ACME_MAX_MLP_LAYERS];
  const float* b[ACME_MAX_MLP_LAYERS];
  EvalHeadArgs head;
};

__global__ void __launch_bounds__(256) az_eval_fused_kernel(const EvalFusedArgs a) {
  static_assert(kEvRows == 4 && kHeadRows == 4, "one wave per row of the block");
  __shared__ __attribute__((aligned(16))) float act[2][kEvRows][kEvWidth];
  __shared__ __attribute__((aligned(16))) float part[kEvRows][256];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * kEvRows;
  for (int i = t; i < kEvRows * a.D; i += 256) {
    const int r = i / a.D, k = i - r * a.D;
    act[0][r][k] = r0 + r < a.rows ? a.obs[(size_t)(r0 + r) * a.D + k] : 0.f;
  }
  __syncthreads();
  int cur = 0, K = a.D;
  for (int i = 0; i < a.nl; ++i) {
    const int N = a.sizes[i];
    int NP = 1;
    while (NP < N) NP *= 2;
    const int G = 256 / NP, n = t & (NP - 1), g = t / NP;
    const bool on = n < N;
    const float* __restrict__ wcol = a.w[i] + (on ? n : 0);
    float acc[kEvRows] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = g; k < K; k += G) {
      const float wk = wcol[(size_t)k * N];
#pragma unroll
      for (int r = 0; r < kEvRows; ++r) acc[r] = fmaf(act[cur][r][k], wk, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kEvRows; ++r) part[r][t] = acc[r];
    __syncthreads();
    if (g == 0 && on) {
      const float bias = a.b[i][n];
      const bool relu = i + 1 < a.nl || a.relu_final != 0;
#pragma unroll
      for (int r = 0; r < kEvRows; ++r) {
        float s = part[r][n];
        for (int q = 1; q < G; ++q) s += part[r][q * NP + n];
        s += bias;
        act[cur ^ 1][r][n] = relu ? act_fwd(ACT_RELU, s) : s;
      }
    }
    __syncthreads();
    cur ^= 1;
    K = N;
  }
  const int r = t >> 6, row = r0 + r;
  if (row < a.rows) eval_head_row(&act[cur][r][0], a.head, row, t & 63);
}

// ------------------------------------------------------------------ host
int check_config(const acme_az_config* c) {
  ACME_CHECK_ARG(c, "null config");
  ACME_CHECK_ARG(c->num_hidden >= 1 && c->num_hidden <= ACME_MAX_MLP_LAYERS,
                 "num_hidden must be in [1, %d], got %d", ACME_MAX_MLP_LAYERS, c->num_hidden);
  ACME_CHECK_ARG(c->obs_dim >= 1 && c->obs_dim <= ACME_AZ_MAX_WIDTH,
                 "obs_dim must be in [1, %d], got %d", ACME_AZ_MAX_WIDTH, c->obs_dim);
  for (int i = 0; i < c->num_hidden; ++i)
    ACME_CHECK_ARG(c->hidden[i] >= 1 && c->hidden[i] <= ACME_AZ_MAX_WIDTH,
                   "hidden[%d] must be in [1, %d], got %d", i, ACME_AZ_MAX_WIDTH, c->hidden[i]);
  ACME_CHECK_ARG(c->num_actions >= 1 && c->num_actions <= ACME_AZ_MAX_ACTIONS,
                 "num_actions must be in [1, %d], got %d", ACME_AZ_MAX_ACTIONS, c->num_actions);
  ACME_CHECK_ARG(c->max_batch >= 1 && c->max_batch <= ACME_AZ_MAX_ROWS,
                 "max_batch must be in [1, %d], got %d", ACME_AZ_MAX_ROWS, c->max_batch);
  ACME_CHECK_ARG(c->max_eval_rows >= 1 && c->max_eval_rows <= ACME_AZ_MAX_ROWS,
                 "max_eval_rows must be in [1, %d], got %d", ACME_AZ_MAX_ROWS, c->max_eval_rows);
  ACME_CHECK_ARG(c->activate_final == 0 || c->activate_final == 1,
                 "activate_final must be 0 or 1, got %d", c->activate_final);
  ACME_CHECK_ARG(std::isfinite(c->discount), "discount must be finite");
  ACME_CHECK_ARG(c->learning_rate >= 0.f && std::isfinite(c->learning_rate),
                 "learning_rate must be finite and >= 0");
  ACME_CHECK_ARG(c->adam_beta1 >= 0.f && c->adam_beta1 < 1.f, "adam_beta1 must be in [0, 1)");
  ACME_CHECK_ARG(c->adam_beta2 >= 0.f && c->adam_beta2 < 1.f, "adam_beta2 must be in [0, 1)");
  ACME_CHECK_ARG(c->adam_epsilon > 0.f, "adam_epsilon must be > 0");
  return ACME_OK;
}

int init_learner(acme_az* l) {
  const acme_az_config& c = l->cfg;
  l->nl = c.num_hidden;
  int din = c.obs_dim, widest = 0;
  for (int i = 0; i < l->nl; ++i) {
    const std::string p = "mlp/linear_" + std::to_string(i);
    l->w[i] = add_tensor(l, p + "/w", {din, c.hidden[i]});
    l->b[i] = add_tensor(l, p + "/b", {c.hidden[i]});
    din = c.hidden[i];
    widest = std::max(widest, din);
  }
  l->pw = add_tensor(l, "policy_value_network/linear/w", {din, c.num_actions});
  l->pb = add_tensor(l, "policy_value_network/linear/b", {c.num_actions});
  l->vw = add_tensor(l, "policy_value_network/linear_1/w", {din, 1});
  l->vb = add_tensor(l, "policy_value_network/linear_1/b", {1});
  const int64_t B = c.max_batch, A = c.num_actions;
  int rc;
  for (int i = 0; i < l->nl; ++i)
    if ((rc = dev_alloc(l, &l->h[i], 2 * B * c.hidden[i])) ||
        (rc = dev_alloc(l, &l->dz[i], B * c.hidden[i])))
      return rc;
  if ((rc = dev_alloc(l, &l->logits, B * A)) || (rc = dev_alloc(l, &l->dlogits, B * A)) ||
      (rc = dev_alloc(l, &l->val, 2 * B)) || (rc = dev_alloc(l, &l->td, B)) ||
      (rc = dev_alloc(l, &l->dv, B)) ||
      (rc = dev_alloc(l, &l->part, 2 * ceil_div(B, kHeadRows))) ||
      (rc = dev_alloc(l, &l->ticket, 1)) || (rc = dev_alloc(l, &l->loss_tmp, 3)) ||
      (rc = dev_alloc(l, &l->eh[0], (int64_t)c.max_eval_rows * widest)) ||
      (rc = dev_alloc(l, &l->eh[1], (int64_t)c.max_eval_rows * widest)))
    return rc;
  ACME_HIP_TRY(hipMemset(l->ticket, 0, sizeof(unsigned)));
  return ACME_OK;
}

int step_impl(acme_az* l, const acme_az_batch* bt, const acme_az_outputs* out, hipStream_t st) {
  const acme_az_config& c = l->cfg;
  const int B = (int)bt->batch, D = c.obs_dim, nl = l->nl, A = c.num_actions;
  const int H = c.hidden[nl - 1];
  int rc;
  // Trunk over the 2B rows: the o_t rows, then the o_tp1 rows.
  for (int i = 0; i < nl; ++i) {
    const int act = i + 1 < nl || c.activate_final ? ACT_RELU : ACT_NONE;
    const float *w = P(l, l->params, l->w[i]), *b = P(l, l->params, l->b[i]);
    rc = i == 0 ? dense_fwd_two("az_trunk_fwd", bt->o_t, B, bt->o_tp1, B, D, w, b, c.hidden[0],
                                act, l->h[0], st)
                : dense_fwd("az_trunk_fwd", l->h[i - 1], 2 * B, c.hidden[i - 1], w, b,
                            c.hidden[i], act, l->h[i], st);
    if (rc != ACME_OK) return rc;
  }
  {
    ACME_PROF("az_head_loss", st, 2.0 * B * (double)H * (2.0 * A + 3.0), 0.0);
    HeadLossArgs a;
    a.h = l->h[nl - 1];
    a.wp = P(l, l->params, l->pw); a.bp = P(l, l->params, l->pb);
    a.wv = P(l, l->params, l->vw); a.bv = P(l, l->params, l->vb);
    a.r = bt->r_t; a.d = bt->d_t; a.pi = bt->pi;
    a.B = B; a.H = H; a.A = A; a.AP = pow2_at_least(A); a.relu_final = c.activate_final;
    a.discount = c.discount;
    a.logits = l->logits; a.dlogits = l->dlogits; a.val = l->val; a.td = l->td; a.dv = l->dv;
    a.dh = l->dz[nl - 1];
    a.part = l->part; a.ticket = l->ticket;
    a.loss = out && out->loss ? out->loss : l->loss_tmp;
    a.value_loss = out && out->value_loss ? out->value_loss : l->loss_tmp + 1;
    a.policy_loss = out && out->policy_loss ? out->policy_loss : l->loss_tmp + 2;
    az_head_loss_kernel<<<(unsigned)ceil_div(B, kHeadRows), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  // Backward over the B o_t rows: the heads' weight gradients ride with the last trunk
  // layer's launch (every dZ they read is the head kernel's).
  BwdGroup g;
  add_wgrad(g, l->h[nl - 1], B, H, l->dlogits, A, Pm(l, l->grads, l->pw), Pm(l, l->grads, l->pb));
  add_wgrad(g, l->h[nl - 1], B, H, l->dv, 1, Pm(l, l->grads, l->vw), Pm(l, l->grads, l->vb));
  for (int i = nl - 1; i >= 0; --i) {
    const float* x = i == 0 ? bt->o_t : l->h[i - 1];
    const int Kin = i == 0 ? D : c.hidden[i - 1];
    add_wgrad(g, x, B, Kin, l->dz[i], c.hidden[i], Pm(l, l->grads, l->w[i]),
              Pm(l, l->grads, l->b[i]));
    if (i > 0)
      add_dgrad(g, l->dz[i], B, c.hidden[i], P(l, l->params, l->w[i]), Kin, l->h[i - 1],
                ACT_RELU, l->dz[i - 1]);
    if ((rc = launch_bwd("az_bwd", g, st)) != ACME_OK) return rc;
  }
  ACME_PROF("az_adam", st, 0.0, 7.0 * 4.0 * (double)l->flat);
  return launch_adam(l->params, l->grads, l->m, l->v, l->flat, c.learning_rate, c.adam_beta1,
                     c.adam_beta2, c.adam_epsilon, l->num_steps + 1, nullptr, 0, st);
}

bool eval_fused(const acme_az_config& c, int64_t rows) {
  if (rows > ACME_AZ_FUSED_MAX_ROWS || c.obs_dim > ACME_AZ_FUSED_MAX_WIDTH) return false;
  for (int i = 0; i < c.num_hidden; ++i)
    if (c.hidden[i] > ACME_AZ_FUSED_MAX_WIDTH) return false;
  return true;
}

int evaluate_impl(acme_az* l, const float* obs, int rows, float* probs, float* value,
                  hipStream_t st) {
  const acme_az_config& c = l->cfg;
  const int nl = l->nl;
  EvalHeadArgs hd;
  hd.wp = P(l, l->params, l->pw); hd.bp = P(l, l->params, l->pb);
  hd.wv = P(l, l->params, l->vw); hd.bv = P(l, l->params, l->vb);
  hd.rows = rows; hd.H = c.hidden[nl - 1]; hd.A = c.num_actions;
  hd.AP = pow2_at_least(c.num_actions);
  hd.probs = probs; hd.value = value;
  hd.h = nullptr;
  if (eval_fused(c, rows)) {
    double flops = 0.0;
    EvalFusedArgs a;
    a.obs = obs; a.rows = rows; a.D = c.obs_dim; a.nl = nl; a.relu_final = c.activate_final;
    for (int i = 0; i < ACME_MAX_MLP_LAYERS; ++i) {
      a.sizes[i] = i < nl ? c.hidden[i] : 0;
      a.w[i] = i < nl ? P(l, l->params, l->w[i]) : nullptr;
      a.b[i] = i < nl ? P(l, l->params, l->b[i]) : nullptr;
      if (i < nl) flops += 2.0 * rows * (double)(i ? c.hidden[i - 1] : c.obs_dim) * c.hidden[i];
    }
    a.head = hd;
    ACME_PROF("az_eval_fused", st, flops, 0.0);
    az_eval_fused_kernel<<<(unsigned)ceil_div(rows, kEvRows), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
    return ACME_OK;
  }
  const float* x = obs;
  for (int i = 0; i < nl; ++i) {
    const int act = i + 1 < nl || c.activate_final ? ACT_RELU : ACT_NONE;
    int rc = dense_fwd("az_eval_fwd", x, rows, i ? c.hidden[i - 1] : c.obs_dim,
                       P(l, l->params, l->w[i]), P(l, l->params, l->b[i]), c.hidden[i], act,
                       l->eh[i & 1], st);
    if (rc != ACME_OK) return rc;
    x = l->eh[i & 1];
  }
  hd.h = x;
  ACME_PROF("az_eval_head", st, 2.0 * rows * (double)hd.H * (hd.A + 1.0), 0.0);
  az_eval_head_kernel<<<(unsigned)ceil_div(rows, kHeadRows), 256, 0, st>>>(hd);
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

}  // namespace

extern "C" {

int acme_az_create(const acme_az_config* cfg, acme_az** out) {
  ACME_CHECK_ARG(out, "null output handle");
  int rc = check_config(cfg);
  if (rc != ACME_OK) return rc;
  acme_az* l = new acme_az();
  l->cfg = *cfg;
  rc = init_learner(l);
  if (rc != ACME_OK) {
    acme_az_destroy(l);
    return rc;
  }
  *out = l;
  return ACME_OK;
}

int acme_az_destroy(acme_az* l) {
  if (!l) return ACME_OK;
  for (void* p : l->allocs) (void)hipFree(p);
  delete l;
  return ACME_OK;
}

int64_t acme_az_flat_size(const acme_az* l) { return l ? l->flat : 0; }
int32_t acme_az_num_tensors(const acme_az* l) { return l ? (int32_t)l->tensors.size() : 0; }

int acme_az_tensor_info(const acme_az* l, int32_t i, int64_t* offset, int64_t* numel,
                        int32_t* ndim, int64_t* shape4, const char** name) {
  return tensor_info(l, i, offset, numel, ndim, shape4, name);
}

int acme_az_bind(acme_az* l, float* params, float* grads, float* adam_m, float* adam_v) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(params && grads && adam_m && adam_v, "null buffer");
  l->params = params;
  l->grads = grads;
  l->m = adam_m;
  l->v = adam_v;
  return ACME_OK;
}

int acme_az_step(acme_az* l, const acme_az_batch* batch, const acme_az_outputs* out,
                 void* stream) {
  ACME_CHECK_ARG(l && batch, "null argument");
  ACME_CHECK_ARG(l->params, "acme_az_step before acme_az_bind");
  ACME_CHECK_ARG(batch->batch >= 1 && batch->batch <= l->cfg.max_batch,
                 "batch must be in [1, max_batch = %d], got %lld", l->cfg.max_batch,
                 (long long)batch->batch);
  ACME_CHECK_ARG(batch->o_t && batch->r_t && batch->d_t && batch->o_tp1 && batch->pi,
                 "null batch tensor");
  const int rc = step_impl(l, batch, out, as_stream(stream));
  if (rc != ACME_OK) return rc;
  l->last_batch = batch->batch;
  ++l->num_steps;
  return ACME_OK;
}

int acme_az_evaluate(acme_az* l, const float* obs, int64_t rows, float* probs, float* value,
                     void* stream) {
  ACME_CHECK_ARG(l && obs && probs && value, "null argument");
  ACME_CHECK_ARG(l->params, "acme_az_evaluate before acme_az_bind");
  ACME_CHECK_ARG(rows >= 1 && rows <= l->cfg.max_eval_rows,
                 "rows must be in [1, max_eval_rows = %d], got %lld", l->cfg.max_eval_rows,
                 (long long)rows);
  return evaluate_impl(l, obs, (int)rows, probs, value, as_stream(stream));
}

int64_t acme_az_num_steps(const acme_az* l) { return l ? l->num_steps : 0; }

int acme_az_set_num_steps(acme_az* l, int64_t n) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(n >= 0, "num_steps must be >= 0, got %lld", (long long)n);
  l->num_steps = n;
  return ACME_OK;
}

int acme_az_debug_buffer(const acme_az* l, const char* name, const float** out, int64_t* count) {
  ACME_CHECK_ARG(l && name && out && count, "null argument");
  const int64_t B = l->last_batch, A = l->cfg.num_actions, H = l->cfg.hidden[l->nl - 1];
  const DebugItem items[] = {
      {"h", l->h[l->nl - 1], 2 * B * H}, {"logits", l->logits, B * A}, {"v", l->val, 2 * B},
      {"td", l->td, B},                  {"dlogits", l->dlogits, B * A}, {"dv", l->dv, B},
      {"dh", l->dz[l->nl - 1], B * H},
  };
  return find_debug_buffer(items, name, out, count);
}

}  // extern "C"
