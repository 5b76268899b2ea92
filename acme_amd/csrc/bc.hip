// Behavioural-cloning learner step and acting call for MI355X: the replacement of
// BCLearner._step (acme/agents/tf/bc/learning.py) and of the evaluator network of
// examples/bsuite/run_bc.py behind the C ABI (include/acme_hip.h, acme_bc_*).
//
// Network: snt.Sequential([snt.Flatten(), snt.nets.MLP([*hidden, A])]): dense ReLU layers, none
// after the last.  Loss: Keras SparseCategoricalCrossentropy(from_logits=True), default
// reduction: mean_b(logsumexp(z_b) - z_b[a_b]).
//
// One step = one stream, no host synchronisation, 2 nl + 2 launches for nl >= 1 hidden layers
// (3 for a linear model):
//   hidden layers forward over the B rows, one launch per layer on the register-operand dense
//     engine (dense_launch.h);
//   bc_head_loss_kernel: the output layer itself, the row's logits in LDS, the max-subtracted
//     log-sum-exp, the loss, dloss/dlogits and the gradient at the last hidden layer's
//     pre-activation; the batch mean summed in block order;
//   backward: the output layer's weight gradient rides with the last hidden layer's launch, then
//     one launch per layer (input gradient + weight gradient);
//   bc_adam_norm_kernel: snt.Adam over the flat buffer (t = num_steps + 1) and, from the
//     gradients it already holds in registers, global_norm(grads) in f64, summed in block order.
// Nothing uses a float atomic: every sum has a fixed order, so a step repeats bit for bit.
//
// An action outside [0, A) is never used as an index: such a row adds nothing to the loss or to
// any gradient, and the mean still divides by B.
//
// Acting: bc_act_fused_kernel runs the whole network and acme_epsilon_greedy's selection in ONE
// launch for up to ACME_BC_FUSED_MAX_ROWS rows of layers up to ACME_BC_FUSED_MAX_WIDTH wide; past
// either, one dense launch per layer and the epsilon-greedy launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "conv.h"
#include "dense_launch.h"
#include "epsilon_greedy.h"
#include "kernels.h"
#include "learner_common.h"
#include "profiler.h"

using namespace acme;
using namespace acme::conv;
using namespace acme::dense;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// No packed f32 arithmetic in this file's kernels, and a barrier that inlines into them: see
// mlp_model.hip and DESIGN.md 4.5.
#ifdef __HIP_DEVICE_COMPILE__
#define ACME_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define ACME_NO_PK_F32
#endif

__device__ ACME_NO_PK_F32 __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int kHeadRows = 4;  // rows per 256-thread block of the head kernel: one wave each
constexpr int kMaxA = ACME_BC_MAX_ACTIONS;
constexpr int kActRows = 4;  // rows per block of the fused acting kernel
constexpr int kActWidth = ACME_BC_FUSED_MAX_WIDTH;
constexpr int kLayers = ACME_MAX_MLP_LAYERS + 1;  // linear layers: the hidden ones and the output
constexpr int kNormBlocks = 8192;                 // grid cap of the Adam launch (launch_adam's)

static_assert(kActSlots * 64 >= kMaxA, "select_action holds a row of ACME_BC_MAX_ACTIONS");

}  // namespace

struct acme_bc {
  acme_bc_config cfg;
  std::vector<Tensor> tensors;
  int64_t flat = 0;
  std::vector<void*> allocs;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  int64_t num_steps = 0;
  int nl = 0;                          // hidden layers; linear layer nl is the output layer
  int size[kLayers] = {};              // hidden[0..nl), then A
  int w[kLayers] = {}, b[kLayers] = {};  // mlp/linear_i
  float* h[ACME_MAX_MLP_LAYERS] = {};   // [max_batch][hidden[i]] activations
  float* dz[ACME_MAX_MLP_LAYERS] = {};  // [max_batch][hidden[i]] pre-activation gradients
  float *logits = nullptr, *dlogits = nullptr;  // [max_batch][A]
  float* part = nullptr;        // [blocks] loss partials of the head kernel
  double* npart = nullptr;      // [kNormBlocks] sum-of-squares partials of the Adam launch
  unsigned* ticket = nullptr;   // [2]: blocks finished, head kernel and Adam launch
  float* out_tmp = nullptr;     // [2] outputs the caller did not ask for
  float* eh[2] = {};            // [max_act_rows][widest hidden] layered acting
  float* act_logits = nullptr;  // [max_act_rows][A] layered acting without logits_out
  int64_t last_batch = 0;       // B of the last step (debug buffers)
  bool act_layered = false;     // ACME_V_BC_ACT=1 (tools/bc_time.py): never the fused acting kernel
};

namespace {

int pow2_at_least(int x) {
  int p = 1;
  while (p < x) p *= 2;
  return p;
}

__device__ ACME_NO_PK_F32 __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The end of both reducing kernels: thread 0 has the block's partial already stored at agent
// scope; it releases, draws a ticket, and tells the block whether it drew the last one.
__device__ ACME_NO_PK_F32 __forceinline__ unsigned draw_ticket(unsigned* ticket) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  return t == gridDim.x - 1 ? 1u : 0u;
}

// ------------------------------------------------------------------ output layer + loss
struct HeadLossArgs {
  const float* x;        // [B][K] last hidden layer's output, or the observations (no hidden layer)
  const float *w, *b;    // [K][A], [A]
  const int32_t* label;  // [B]
  int B, K, A, AP;
  float *logits, *dlogits;  // [B][A]
  float* dh;                // [B][K] gradient at the last hidden pre-activation; null without one
  float* part;              // [gridDim.x]
  unsigned* ticket;
  float* loss;
};

// One wave per row.  Logits: actions in passes of 64 lanes; for A < 64, lane = g * AP + a with
// AP = A rounded up to a power of two and G = 64 / AP k-groups; group g sums k = g, g + G, ... of
// logit a (W[k, :] read coalesced over a) and a butterfly over the lane bits above AP adds the
// groups (az_head_loss_kernel's split).  The row's logits go to LDS; maximum, log-sum-exp and
// gradient are lane-strided over A with wave reductions; dlogits overwrite the logits in LDS
// (element j by the lane that read it) and dh is lane-strided over k from there.  A wave whose
// row is past B works on row B - 1 and stores nothing, so every wave meets every barrier.
__global__ void ACME_NO_PK_F32 __launch_bounds__(256) bc_head_loss_kernel(const HeadLossArgs a) {
  __shared__ float z[kHeadRows][kMaxA];
  __shared__ float red[kHeadRows];
  __shared__ unsigned last_s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row0 = blockIdx.x * kHeadRows + w;
  const bool live = row0 < a.B;
  const int row = live ? row0 : a.B - 1;
  const int K = a.K, A = a.A, AP = a.AP;
  const float* x = a.x + (size_t)row * K;
  float* zr = z[w];
  {
    const int G = 64 / AP, g = lane / AP, al = lane & (AP - 1);
    for (int a0 = 0; a0 < A; a0 += 64) {
      const int col = a0 + al;
      const bool on = col < A;
      const int c = on ? col : 0;  // lanes past A read column 0 and drop it
      float acc = 0.f;
#pragma unroll 4
      for (int k = g; k < K; k += G) acc = fmaf(x[k], a.w[(size_t)k * A + c], acc);
      for (int o = AP; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
      if (on && g == 0) zr[col] = acc + a.b[c];
    }
  }
  block_sync();
  float m = -INFINITY;
  for (int j = lane; j < A; j += 64) m = fmaxf(m, zr[j]);
  m = wave_max(m);
  const int lab = a.label[row];
  const bool ok = live && lab >= 0 && lab < A;  // a bad action is never an index
  // s = sum_j e_j and so = sum_{j != label} e_j with e_j = exp(z_j - m): softmax_label - 1 is
  // -so / s, with no cancellation when the label holds nearly all of the mass.
  float s = 0.f, so = 0.f;
  for (int j = lane; j < A; j += 64) {
    const float e = expf(zr[j] - m);
    s += e;
    so += j == lab ? 0.f : e;
  }
  s = wave_sum(s);
  so = wave_sum(so);
  const float zl = zr[ok ? lab : 0];
  const float ce = !ok ? 0.f : zl == m ? log1pf(so) : logf(s) - (zl - m);
  const float invB = 1.f / (float)a.B;
  for (int j = lane; j < A; j += 64) {
    const float zj = zr[j];
    const float d = ok ? (j == lab ? -so / s : expf(zj - m) / s) * invB : 0.f;
    if (live) {
      a.logits[(size_t)row * A + j] = zj;
      a.dlogits[(size_t)row * A + j] = d;
    }
    zr[j] = d;
  }
  block_sync();
  if (a.dh) {
    // dh[k] = sum_j dlogits_j W[k, j], masked by the last hidden layer's ReLU.
    for (int k = lane; k < K; k += 64) {
      const float* wr = a.w + (size_t)k * A;
      float acc = 0.f;
#pragma unroll 4
      for (int j = 0; j < A; ++j) acc = fmaf(zr[j], wr[j], acc);
      acc = x[k] > 0.f ? acc : 0.f;
      if (live) a.dh[(size_t)row * K + k] = acc;
    }
  }
  // The batch mean: the block's four rows in order, then the blocks' partials by the block that
  // finishes last (agent-scope stores, a release before the ticket, an acquire after it).
  if (lane == 0) red[w] = ce;
  block_sync();
  if (threadIdx.x == 0) {
    const float sc = ((red[0] + red[1]) + red[2]) + red[3];
    __hip_atomic_store(&a.part[blockIdx.x], sc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = draw_ticket(a.ticket);
  }
  block_sync();
  if (last_s != 0u && w == 0) {  // uniform per block, then per wave
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    float sc = 0.f;
    for (int i = lane; i < (int)gridDim.x; i += 64)
      sc += __hip_atomic_load(&a.part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sc = wave_sum(sc);
    if (lane == 0) {
      *a.loss = sc / (float)a.B;
      __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------ Adam + gradient norm
struct AdamNormArgs {
  float* p;
  const float* g;
  float *m, *v;
  int64_t n4;
  float lr, b1, omb1, b2, omb2, bc1, bc2, eps;
  double* part;  // [gridDim.x]
  unsigned* ticket;
  float* norm;
};

// snt.Adam on float4 i of the flat buffers (adam_update4's operations), and the sum of squares
// of the gradients it has just loaded: per thread in f64 in index order, the wave by butterfly,
// the block's four waves in order, the blocks' partials by the block that draws the last ticket.
// The padding between tensors is zero in `grads` and adds nothing.
__global__ void ACME_NO_PK_F32 __launch_bounds__(256) bc_adam_norm_kernel(const AdamNormArgs a) {
  __shared__ double red[4];
  __shared__ unsigned last_s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double ss = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4;
       i += (int64_t)gridDim.x * 256) {
    const f32x4 gg = reinterpret_cast<const f32x4*>(a.g)[i];
    f32x4 mm = reinterpret_cast<const f32x4*>(a.m)[i];
    f32x4 vv = reinterpret_cast<const f32x4*>(a.v)[i];
    f32x4 pp = reinterpret_cast<const f32x4*>(a.p)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float mj = __fadd_rn(__fmul_rn(a.b1, mm[j]), __fmul_rn(a.omb1, gg[j]));
      const float vj =
          __fadd_rn(__fmul_rn(a.b2, vv[j]), __fmul_rn(a.omb2, __fmul_rn(gg[j], gg[j])));
      const float mh = __fdiv_rn(mj, a.bc1);
      const float vh = __fdiv_rn(vj, a.bc2);
      const float den = __fadd_rn(__fsqrt_rn(vh), a.eps);
      mm[j] = mj;
      vv[j] = vj;
      pp[j] = __fsub_rn(pp[j], __fdiv_rn(__fmul_rn(a.lr, mh), den));
      ss += (double)gg[j] * (double)gg[j];
    }
    reinterpret_cast<f32x4*>(a.m)[i] = mm;
    reinterpret_cast<f32x4*>(a.v)[i] = vv;
    reinterpret_cast<f32x4*>(a.p)[i] = pp;
  }
  ss = wave_sum_f64(ss);
  if (lane == 0) red[w] = ss;
  block_sync();
  if (threadIdx.x == 0) {
    const double sb = ((red[0] + red[1]) + red[2]) + red[3];
    __hip_atomic_store(&a.part[blockIdx.x], sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = draw_ticket(a.ticket);
  }
  block_sync();
  if (last_s != 0u && w == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double s = 0.0;
    for (int i = lane; i < (int)gridDim.x; i += 64)
      s += __hip_atomic_load(&a.part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s = wave_sum_f64(s);
    if (lane == 0) {
      *a.norm = (float)sqrt(s);
      __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------ acting in one launch
// The whole network for kActRows rows per 256-thread block, activations ping-pong in LDS.  Layer
// K -> N (N <= kActWidth): thread t owns output column n = t % NP (NP = N rounded up to a power
// of two) and k-group g = t / NP of G = 256 / NP; it reads W[k, n] coalesced over n for
// k = g, g + G, ... and each x[r][k] as an LDS broadcast; the G partials are summed in group
// order through LDS.  The last layer's row is the logits; one wave per row then takes them from
// LDS, lane l holding actions l, l + 64, ..., and applies select_action to them.
struct ActFusedArgs {
  const float* obs;  // [rows][D]
  int rows, D, L;    // L linear layers
  int sizes[kLayers];
  const float* w[kLayers];
  const float* b[kLayers];
  double epsilon;
  uint64_t seed, step;
  float* logits;     // [rows][A], optional
  int32_t* actions;  // [rows]
};

__global__ void ACME_NO_PK_F32 __launch_bounds__(256) bc_act_fused_kernel(const ActFusedArgs a) {
  static_assert(kActRows == 4, "one wave per row of the block");
  __shared__ __attribute__((aligned(16))) float act[2][kActRows][kActWidth];
  __shared__ __attribute__((aligned(16))) float part[kActRows][256];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * kActRows;
  for (int i = t; i < kActRows * a.D; i += 256) {
    const int r = i / a.D, k = i - r * a.D;
    act[0][r][k] = r0 + r < a.rows ? a.obs[(size_t)(r0 + r) * a.D + k] : 0.f;
  }
  block_sync();
  int cur = 0, K = a.D;
  for (int i = 0; i < a.L; ++i) {
    const int N = a.sizes[i];
    int NP = 1;
    while (NP < N) NP *= 2;
    const int G = 256 / NP, n = t & (NP - 1), g = t / NP;
    const bool on = n < N;
    const float* __restrict__ wcol = a.w[i] + (on ? n : 0);
    float acc[kActRows] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = g; k < K; k += G) {
      const float wk = wcol[(size_t)k * N];
#pragma unroll
      for (int r = 0; r < kActRows; ++r) acc[r] = fmaf(act[cur][r][k], wk, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kActRows; ++r) part[r][t] = acc[r];
    block_sync();
    if (g == 0 && on) {
      const float bias = a.b[i][n];
      const bool relu = i + 1 < a.L;
#pragma unroll
      for (int r = 0; r < kActRows; ++r) {
        float s = part[r][n];
        for (int q = 1; q < G; ++q) s += part[r][q * NP + n];
        s += bias;
        act[cur ^ 1][r][n] = relu ? (s > 0.f ? s : 0.f) : s;
      }
    }
    block_sync();
    cur ^= 1;
    K = N;
  }
  const int r = t >> 6, lane = t & 63, row = r0 + r, A = K;
  if (row >= a.rows) return;  // uniform per wave, no barrier below
  float qv[kActSlots];
#pragma unroll
  for (int i = 0; i < kActSlots; ++i) {
    const int j = lane + 64 * i;
    qv[i] = 64 * i < kActWidth && j < A ? act[cur][r][j] : 0.f;
    if (64 * i < kActWidth && j < A && a.logits) a.logits[(size_t)row * A + j] = qv[i];
  }
  const int action = select_action(qv, A, lane, (uint32_t)row, a.epsilon, a.seed, a.step);
  if (lane == 0) a.actions[row] = action;
}

// ------------------------------------------------------------------ host
int check_config(const acme_bc_config* c) {
  ACME_CHECK_ARG(c, "null config");
  ACME_CHECK_ARG(c->num_hidden >= 0 && c->num_hidden <= ACME_MAX_MLP_LAYERS,
                 "num_hidden must be in [0, %d], got %d", ACME_MAX_MLP_LAYERS, c->num_hidden);
  ACME_CHECK_ARG(c->obs_dim >= 1 && c->obs_dim <= ACME_BC_MAX_WIDTH,
                 "obs_dim must be in [1, %d], got %d", ACME_BC_MAX_WIDTH, c->obs_dim);
  for (int i = 0; i < c->num_hidden; ++i)
    ACME_CHECK_ARG(c->hidden[i] >= 1 && c->hidden[i] <= ACME_BC_MAX_WIDTH,
                   "hidden[%d] must be in [1, %d], got %d", i, ACME_BC_MAX_WIDTH, c->hidden[i]);
  ACME_CHECK_ARG(c->num_actions >= 1 && c->num_actions <= ACME_BC_MAX_ACTIONS,
                 "num_actions must be in [1, %d], got %d", ACME_BC_MAX_ACTIONS, c->num_actions);
  ACME_CHECK_ARG(c->max_batch >= 1 && c->max_batch <= ACME_BC_MAX_ROWS,
                 "max_batch must be in [1, %d], got %d", ACME_BC_MAX_ROWS, c->max_batch);
  ACME_CHECK_ARG(c->max_act_rows >= 1 && c->max_act_rows <= ACME_BC_MAX_ROWS,
                 "max_act_rows must be in [1, %d], got %d", ACME_BC_MAX_ROWS, c->max_act_rows);
  ACME_CHECK_ARG(c->learning_rate >= 0.f && std::isfinite(c->learning_rate),
                 "learning_rate must be finite and >= 0");
  ACME_CHECK_ARG(c->adam_beta1 >= 0.f && c->adam_beta1 < 1.f, "adam_beta1 must be in [0, 1)");
  ACME_CHECK_ARG(c->adam_beta2 >= 0.f && c->adam_beta2 < 1.f, "adam_beta2 must be in [0, 1)");
  ACME_CHECK_ARG(c->adam_epsilon > 0.f, "adam_epsilon must be > 0");
  return ACME_OK;
}

int init_learner(acme_bc* l) {
  const acme_bc_config& c = l->cfg;
  l->nl = c.num_hidden;
  l->act_layered = tune_variant("BC_ACT") == 1;  // read once, at creation
  int din = c.obs_dim, widest = 1;
  for (int i = 0; i <= l->nl; ++i) {
    l->size[i] = i < l->nl ? c.hidden[i] : c.num_actions;
    const std::string p = "mlp/linear_" + std::to_string(i);
    l->w[i] = add_tensor(l, p + "/w", {din, l->size[i]});
    l->b[i] = add_tensor(l, p + "/b", {l->size[i]});
    din = l->size[i];
    if (i < l->nl) widest = std::max(widest, din);
  }
  const int64_t B = c.max_batch, A = c.num_actions, R = c.max_act_rows;
  int rc;
  for (int i = 0; i < l->nl; ++i)
    if ((rc = dev_alloc(l, &l->h[i], B * c.hidden[i])) ||
        (rc = dev_alloc(l, &l->dz[i], B * c.hidden[i])))
      return rc;
  if ((rc = dev_alloc(l, &l->logits, B * A)) || (rc = dev_alloc(l, &l->dlogits, B * A)) ||
      (rc = dev_alloc(l, &l->part, ceil_div(B, kHeadRows))) ||
      (rc = dev_alloc(l, &l->npart, kNormBlocks)) || (rc = dev_alloc(l, &l->ticket, 2)) ||
      (rc = dev_alloc(l, &l->out_tmp, 2)) || (rc = dev_alloc(l, &l->eh[0], R * widest)) ||
      (rc = dev_alloc(l, &l->eh[1], R * widest)) || (rc = dev_alloc(l, &l->act_logits, R * A)))
    return rc;
  ACME_HIP_TRY(hipMemset(l->ticket, 0, 2 * sizeof(unsigned)));
  return ACME_OK;
}

int step_impl(acme_bc* l, const acme_bc_batch* bt, const acme_bc_outputs* out, hipStream_t st) {
  const acme_bc_config& c = l->cfg;
  const int B = (int)bt->batch, D = c.obs_dim, nl = l->nl, A = c.num_actions;
  int rc;
  const float* x = bt->o_tm1;
  int K = D;
  for (int i = 0; i < nl; ++i) {
    rc = dense_fwd("bc_fwd", x, B, K, P(l, l->params, l->w[i]), P(l, l->params, l->b[i]),
                   c.hidden[i], ACT_RELU, l->h[i], st);
    if (rc != ACME_OK) return rc;
    x = l->h[i];
    K = c.hidden[i];
  }
  {
    ACME_PROF("bc_head_loss", st, 4.0 * B * (double)K * A, 0.0);
    HeadLossArgs a;
    a.x = x;
    a.w = P(l, l->params, l->w[nl]); a.b = P(l, l->params, l->b[nl]);
    a.label = bt->a_tm1;
    a.B = B; a.K = K; a.A = A; a.AP = std::min(64, pow2_at_least(A));
    a.logits = l->logits; a.dlogits = l->dlogits;
    a.dh = nl ? l->dz[nl - 1] : nullptr;
    a.part = l->part; a.ticket = l->ticket;
    a.loss = out && out->loss ? out->loss : l->out_tmp;
    bc_head_loss_kernel<<<(unsigned)ceil_div(B, kHeadRows), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  // Backward: the output layer's weight gradient rides with the last hidden layer's launch
  // (the dZ it reads is the head kernel's); without a hidden layer it is a launch of its own.
  BwdGroup g;
  add_wgrad(g, x, B, K, l->dlogits, A, Pm(l, l->grads, l->w[nl]), Pm(l, l->grads, l->b[nl]));
  if (nl == 0 && (rc = launch_bwd("bc_bwd", g, st)) != ACME_OK) return rc;
  for (int i = nl - 1; i >= 0; --i) {
    const float* xin = i == 0 ? bt->o_tm1 : l->h[i - 1];
    const int Kin = i == 0 ? D : c.hidden[i - 1];
    add_wgrad(g, xin, B, Kin, l->dz[i], c.hidden[i], Pm(l, l->grads, l->w[i]),
              Pm(l, l->grads, l->b[i]));
    if (i > 0)
      add_dgrad(g, l->dz[i], B, c.hidden[i], P(l, l->params, l->w[i]), Kin, l->h[i - 1],
                ACT_RELU, l->dz[i - 1]);
    if ((rc = launch_bwd("bc_bwd", g, st)) != ACME_OK) return rc;
  }
  {
    ACME_PROF("bc_adam_norm", st, 0.0, 7.0 * 4.0 * (double)l->flat);
    const float b1 = c.adam_beta1, b2 = c.adam_beta2, t = (float)(l->num_steps + 1);
    AdamNormArgs a;
    a.p = l->params; a.g = l->grads; a.m = l->m; a.v = l->v;
    a.n4 = l->flat / 4;  // tensors start at multiples of 64 floats
    a.lr = c.learning_rate; a.b1 = b1; a.omb1 = 1.f - b1; a.b2 = b2; a.omb2 = 1.f - b2;
    a.bc1 = 1.f - powf(b1, t); a.bc2 = 1.f - powf(b2, t); a.eps = c.adam_epsilon;
    a.part = l->npart; a.ticket = l->ticket + 1;
    a.norm = out && out->gradient_norm ? out->gradient_norm : l->out_tmp + 1;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(a.n4, 256), kNormBlocks);
    bc_adam_norm_kernel<<<std::max(grid, 1u), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  return ACME_OK;
}

bool act_fused(const acme_bc* l, int64_t rows) {
  if (l->act_layered || rows > ACME_BC_FUSED_MAX_ROWS || l->cfg.obs_dim > kActWidth) return false;
  for (int i = 0; i <= l->nl; ++i)
    if (l->size[i] > kActWidth) return false;
  return true;
}

int act_impl(acme_bc* l, const float* obs, int rows, double epsilon, uint64_t seed,
             uint64_t step_counter, float* logits_out, int32_t* actions, hipStream_t st) {
  const acme_bc_config& c = l->cfg;
  const int nl = l->nl, A = c.num_actions;
  if (act_fused(l, rows)) {
    double flops = 0.0;
    ActFusedArgs a;
    a.obs = obs; a.rows = rows; a.D = c.obs_dim; a.L = nl + 1;
    for (int i = 0; i < kLayers; ++i) {
      a.sizes[i] = i <= nl ? l->size[i] : 0;
      a.w[i] = i <= nl ? P(l, l->params, l->w[i]) : nullptr;
      a.b[i] = i <= nl ? P(l, l->params, l->b[i]) : nullptr;
      if (i <= nl) flops += 2.0 * rows * (double)(i ? l->size[i - 1] : c.obs_dim) * l->size[i];
    }
    a.epsilon = epsilon; a.seed = seed; a.step = step_counter;
    a.logits = logits_out; a.actions = actions;
    ACME_PROF("bc_act_fused", st, flops, 0.0);
    bc_act_fused_kernel<<<(unsigned)ceil_div(rows, kActRows), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
    return ACME_OK;
  }
  float* lg = logits_out ? logits_out : l->act_logits;
  const float* x = obs;
  for (int i = 0; i <= nl; ++i) {
    float* y = i == nl ? lg : l->eh[i & 1];
    int rc = dense_fwd("bc_act_fwd", x, rows, i ? l->size[i - 1] : c.obs_dim,
                       P(l, l->params, l->w[i]), P(l, l->params, l->b[i]), l->size[i],
                       i == nl ? ACT_NONE : ACT_RELU, y, st);
    if (rc != ACME_OK) return rc;
    x = y;
  }
  return launch_epsilon_greedy(lg, rows, A, epsilon, seed, step_counter, actions, st);
}

}  // namespace

extern "C" {

int acme_bc_create(const acme_bc_config* cfg, acme_bc** out) {
  ACME_CHECK_ARG(out, "null output handle");
  int rc = check_config(cfg);
  if (rc != ACME_OK) return rc;
  acme_bc* l = new acme_bc();
  l->cfg = *cfg;
  rc = init_learner(l);
  if (rc != ACME_OK) {
    acme_bc_destroy(l);
    return rc;
  }
  *out = l;
  return ACME_OK;
}

int acme_bc_destroy(acme_bc* l) {
  if (!l) return ACME_OK;
  for (void* p : l->allocs) (void)hipFree(p);
  delete l;
  return ACME_OK;
}

int64_t acme_bc_flat_size(const acme_bc* l) { return l ? l->flat : 0; }
int32_t acme_bc_num_tensors(const acme_bc* l) { return l ? (int32_t)l->tensors.size() : 0; }

int acme_bc_tensor_info(const acme_bc* l, int32_t i, int64_t* offset, int64_t* numel,
                        int32_t* ndim, int64_t* shape4, const char** name) {
  return tensor_info(l, i, offset, numel, ndim, shape4, name);
}

int acme_bc_bind(acme_bc* l, float* params, float* grads, float* adam_m, float* adam_v) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(params && grads && adam_m && adam_v, "null buffer");
  l->params = params;
  l->grads = grads;
  l->m = adam_m;
  l->v = adam_v;
  return ACME_OK;
}

int acme_bc_step(acme_bc* l, const acme_bc_batch* batch, const acme_bc_outputs* out,
                 void* stream) {
  ACME_CHECK_ARG(l && batch, "null argument");
  ACME_CHECK_ARG(l->params, "acme_bc_step before acme_bc_bind");
  ACME_CHECK_ARG(batch->batch >= 1 && batch->batch <= l->cfg.max_batch,
                 "batch must be in [1, max_batch = %d], got %lld", l->cfg.max_batch,
                 (long long)batch->batch);
  ACME_CHECK_ARG(batch->o_tm1 && batch->a_tm1, "null batch tensor");
  const int rc = step_impl(l, batch, out, as_stream(stream));
  if (rc != ACME_OK) return rc;
  l->last_batch = batch->batch;
  ++l->num_steps;
  return ACME_OK;
}

int acme_bc_act(acme_bc* l, const float* obs, int64_t rows, double epsilon, uint64_t seed,
                uint64_t step_counter, float* logits_out, int32_t* actions_out, void* stream) {
  ACME_CHECK_ARG(l && obs && actions_out, "null argument");
  ACME_CHECK_ARG(l->params, "acme_bc_act before acme_bc_bind");
  ACME_CHECK_ARG(rows >= 1 && rows <= l->cfg.max_act_rows,
                 "rows must be in [1, max_act_rows = %d], got %lld", l->cfg.max_act_rows,
                 (long long)rows);
  ACME_CHECK_ARG(epsilon >= 0.0 && epsilon <= 1.0, "epsilon must be in [0, 1]");  // NaN fails
  return act_impl(l, obs, (int)rows, epsilon, seed, step_counter, logits_out, actions_out,
                  as_stream(stream));
}

int64_t acme_bc_num_steps(const acme_bc* l) { return l ? l->num_steps : 0; }

int acme_bc_set_num_steps(acme_bc* l, int64_t n) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(n >= 0, "num_steps must be >= 0, got %lld", (long long)n);
  l->num_steps = n;
  return ACME_OK;
}

int acme_bc_debug_buffer(const acme_bc* l, const char* name, const float** out, int64_t* count) {
  ACME_CHECK_ARG(l && name && out && count, "null argument");
  const int64_t B = l->last_batch, A = l->cfg.num_actions;
  const int64_t H = l->nl ? l->cfg.hidden[l->nl - 1] : 0;
  const DebugItem items[] = {
      {"logits", l->logits, B * A},
      {"dlogits", l->dlogits, B * A},
      {"dh", l->nl ? l->dz[l->nl - 1] : nullptr, B * H},
  };
  return find_debug_buffer(items, name, out, count);
}

}  // extern "C"
