// D4PG learner step for MI355X: the replacement of D4PGLearner._step
// (acme/agents/tf/d4pg/learning.py:156-247) behind the C ABI (include/acme_hip.h).
//
// One call = the whole step on one stream, no host synchronisation:
//   target <- online when num_steps % period == 0 (at the start)          (:171-175)
//   online policy on o_t (dpg actions), target policy on o_t              (:199, :206)
//   online critic on [o_tm1, a_tm1 ; o_t, dpg_a] as ONE 2B-row pass        (:198, :207)
//   target critic on (o_t, target actions)                                (:199)
//   fused loss kernel: categorical L2 projection + softmax cross-entropy   (:202-203)
//     for rows < B, d mean(q) / d logits for the dpg rows                  (:208)
//   critic backward over 2B rows (weight gradients from the first B rows
//     only); the LayerNorm backward of the dpg rows also forms dq/da,
//     tf.clip_by_norm(., 1) and dloss/da = -dqda / B                      (:211-218, dpg.py)
//   policy backward; clip_by_global_norm(40) per network; two Adams       (:221-241)
//
// Networks (examples/control_suite/run_d4pg.py:60-81): LayerNormMLP
// (acme/tf/networks/continuous.py:37-68) = Linear -> LayerNorm -> tanh -> MLP(elu,
// activate_final); policy head NearZeroInitializedLinear + TanhToSpec
// (rescaling.py:55-74); critic head DiscreteValuedHead (distributional.py:36-67).
//
// One learner core, five handle types.  acme_d4pg, acme_ddpg, acme_mpo, acme_dmpo and acme_crr
// derive from acme_actor_critic, whose Head says which step it takes; the flat-buffer layout,
// bind, the step entry (checks, graph or eager, step count), the LayerNormMLP passes, the
// backward launches, clip_and_adam and the debug-buffer lookup are written once over that core,
// and the exports are one-line calls into them.
//
// DDPG (acme_ddpg_*, acme/agents/tf/ddpg/learning.py:143-237) is Head::kScalar: the critic
// is LayerNormMLP(critic_sizes + (1,)), and ddpg_head_td_kernel (head forward, TD loss
// 0.5 (r + discount d q_t - q_tm1)^2, the head's input gradient) stands where the head GEMMs,
// the categorical loss kernel and the head's input-gradient problem stand for D4PG;
// everything else of d4pg_step_impl is shared.
//
// MPO (acme_mpo_*, acme/agents/tf/mpo/learning.py:145-260, acme/tf/losses/mpo.py) is
// Head::kMpo: a Gaussian policy head, N actions per state sampled from the target policy on
// the device, the scalar critic over those N B rows, the decoupled MPO loss and its dual
// variables as a third parameter group.  Its kernels are in mpo_kernels.h, its step is
// mpo_step_impl below.
//
// DMPO (acme_dmpo_*, acme/agents/tf/dmpo/learning.py:147-276) is Head::kMpoCategorical: MPO's
// policy side and duals with D4PG's DiscreteValuedHead critic, the head run over the N B
// sampled rows and the bootstrap distribution of each state the mixture of its N sampled
// distributions (dmpo_mix_loss_kernel, mpo_kernels.h).  Its step is dmpo_step_impl, built from
// the blocks of mpo_step_impl and the categorical head's backward of d4pg_step_impl.
//
// CRR (acme_crr_*, acme/agents/tf/crr/recurrent_learning.py:197-377 with stateless networks) is
// Head::kCrr: MPO's Gaussian policy head and DMPO's categorical critic without the duals, a
// second set of sampled actions through the online critic for the value estimate, the
// advantage-weighted behaviour-cloning loss and a target copy after the update.  Its kernels
// are in crr_kernels.h, its step is crr_step_impl.
//
// Small-batch regime (B = 256, widths <= 512): the step is ~1.5 GFLOP, so it is latency
// bound.  Dense layers go through the fp32 MFMA GEMM engine with fused bias/activation
// epilogues and masked dgrads; the row-wise work (LayerNorm+tanh, TanhToSpec head,
// projection loss, LayerNorm backward + dpg) are one-kernel-per-stage row kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "conv.h"
#include "dense_launch.h"
#include "detmath.h"
#include "gemm.h"
#include "gemm_direct.h"
#include "kernels.h"
#include "launch.h"
#include "learner_common.h"
#include "profiler.h"


using namespace acme;
using namespace acme::conv;
using namespace acme::dense;

namespace {

constexpr int kRows = 4;      // rows per block of the LayerNorm row kernels
constexpr int kMaxWidth = 1024;
constexpr int kMaxIn = 64;    // obs_dim + act_dim
constexpr int kNormBlocks = 256;
constexpr int kGraphKeys = 11;  // pointers that key a captured step graph (MPO uses all)

// Tensor indices of one LayerNormMLP + output layer.
struct NetDesc {
  int din = 0, nl = 0, nout = 0;
  int sizes[ACME_D4PG_MAX_LAYERS] = {};
  int w1 = -1, b1 = -1, scale = -1, offset = -1;
  int w[ACME_D4PG_MAX_LAYERS] = {}, b[ACME_D4PG_MAX_LAYERS] = {};  // mlp linear_{i-1}, i >= 1
  int ow = -1, ob = -1;                                            // output layer
};

// Activations of one evaluation of a network over `rows` rows.
struct Acts {
  float* z1 = nullptr;    // [rows][H0] first linear output (pre-LayerNorm)
  float* mean = nullptr;  // [rows]
  float* rstd = nullptr;  // [rows]
  float* h[ACME_D4PG_MAX_LAYERS] = {};  // h[0] = tanh(LN(z1)), h[i] = elu(...)
  float* out = nullptr;   // policy: actions [rows][act]; critic: logits [rows][atoms]
  float* t = nullptr;     // policy: tanh of the head [rows][act]
};

// What the critic ends in, and with it which step the learner takes.
enum class Head {
  kCategorical,  // D4PG: DiscreteValuedHead, categorical projection loss
  kScalar,       // DDPG: one scalar, TD loss
  kMpo,          // MPO: scalar critic, Gaussian policy head, the dual variables
  kMpoCategorical,  // DMPO: MPO's policy side, D4PG's DiscreteValuedHead critic
  kCrr,          // CRR: the Gaussian policy head, DMPO's critic, no duals
};

// The kinds with a Gaussian policy head, sampled actions and dual variables (MPO's policy side).
constexpr bool has_duals(Head h) { return h == Head::kMpo || h == Head::kMpoCategorical; }
// The kinds whose critic ends in a DiscreteValuedHead over the support `values`.
constexpr bool is_categorical(Head h) {
  return h == Head::kCategorical || h == Head::kMpoCategorical || h == Head::kCrr;
}
// The kinds whose policy ends in a MultivariateNormalDiagHead.
constexpr bool has_gauss_head(Head h) { return has_duals(h) || h == Head::kCrr; }

}  // namespace

// The learner behind the four handle types of this file (below): the LayerNormMLP policy and
// critic in one flat buffer, their workspaces and the captured step graphs.
struct acme_actor_critic {
  virtual ~acme_actor_critic() = default;
  Head head = Head::kCategorical;
  acme_d4pg_config cfg;
  std::vector<Tensor> tensors;
  int64_t flat = 0, policy_flat = 0;
  float *params = nullptr, *target = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  int64_t num_steps = 0;
  NetDesc pol, cri;
  std::vector<void*> allocs;
  Acts pon, ptg, con, ctg;
  float* cdz[ACME_D4PG_MAX_LAYERS] = {};  // critic pre-activation grads [2B][C_i]
  float* pdz[ACME_D4PG_MAX_LAYERS] = {};  // policy [B][P_i]
  float* dlogits = nullptr;               // [2B][atoms]
  float* du = nullptr;                    // [B][act] dloss/d(policy head pre-tanh)
  float* dqda = nullptr;                  // [B][act] clipped dq/da
  float* values = nullptr;                // [atoms] support
  float* act_lo = nullptr;                // [act]
  float* act_scale = nullptr;             // [act]
  float* lnslab = nullptr;                // LayerNorm parameter-gradient partials (critic)
  float* lnslab2 = nullptr;               // (policy: both are reduced after the backward)
  float* ploss_part = nullptr;            // per-block dpg loss partials
  double* norm_part = nullptr;            // [2][kNormBlocks]
  float* norms = nullptr;                 // [2] global norms (policy, critic)
  float* loss_tmp = nullptr;              // [3] critic / policy loss, CRR's mean coefficient
  float* ce = nullptr;                    // [B] per-row cross-entropy (DDPG: 0.5 td^2)
  // Scalar heads (DDPG, MPO): the critic ends in one scalar, con.out / ctg.out hold q.
  float* td = nullptr;                    // [B] TD error
  float* dq = nullptr;                    // [2B] dloss/dq (rows < B), 1 (dpg rows)
  int64_t* dev_step = nullptr;            // device mirror of num_steps (Adam t)
  // MPO (acme_mpo_create): Gaussian policy head, N sampled actions per state, scalar critic,
  // the dual variables as a third parameter group [critic_end, flat).
  acme_mpo_config mcfg;
  int64_t critic_end = 0;                 // end of the critic's floats (= flat without duals)
  int sw = -1, sb = -1;                   // the head's scale layer (pol.ow / pol.ob: its mean layer)
  int t_temp = -1, t_amean = -1, t_astd = -1, t_ptemp = -1;  // dual tensors
  struct MpoBufs {
    float *sd_on, *sd_t;                  // [B][A] stddevs (means: pon.out / ptg.out, pre-softplus: .t)
    float *noise, *act;                   // [N B][A] eps used, sampled actions
    float *cost, *tiled;                  // [N B] out-of-bound cost, [N B][obs] o_t tiled N times
    float *w, *pw;                        // [N B] normalized weights, penalty weights
    float *sq;                            // [N B] sampled target values (MPO: ctg.out itself)
    float *qt;                            // [B] mean_n of the sampled target values
    float *dmean, *dpre;                  // [B][A] dloss / d(online mean, pre-softplus scale)
    float *part;                          // [ceil(B / 4)][kMpoCols] per-block sums of the loss kernel
    float *stats, *klm_rel, *kls_rel, *ploss;  // outputs when the caller passes none
  } mb = {};
  // DMPO (acme_dmpo_create): the categorical head over the N B sampled rows (ctg.out holds
  // their logits, mb.sq their means) and the bootstrap mixture of each state.
  float* mixture = nullptr;               // [B][atoms] normalised mixture probabilities
  // CRR (acme_crr_create): mb's policy-side buffers with both action sets in noise / act /
  // tiled ([N_td R] rows for the target critic, then [N_pw R] for the online critic, whose
  // logits follow the R rows of con.out), and the policy loss's per-state values.
  acme_crr_config ccfg;
  struct CrrBufs {
    float *q_mean, *v_est, *adv, *coef, *logp;  // [B]
    float* coef_part;                           // [ceil(B / 4)] per-block coefficient sums
  } cb = {};
  int64_t crr_rows = 0;                   // R of the last step (the debug buffers' packing)
  // Captured step graphs, keyed by the batch / output pointers (MPO, DMPO, CRR: the noise
  // pointer too), B and the target-copy flags (CRR's copy is the graph's last node).
  struct Graph {
    const void* key[kGraphKeys];
    int64_t B;
    int copy;
    hipGraphExec_t exec;
  };
  std::vector<Graph> graphs;
  hipStream_t capture = nullptr;
};

// The handle types of the C ABI: each *_create allocates its own, everything else works on
// the learner they share.
struct acme_d4pg : acme_actor_critic {};
struct acme_ddpg : acme_actor_critic {};
struct acme_mpo : acme_actor_critic {};
struct acme_dmpo : acme_actor_critic {};
struct acme_crr : acme_actor_critic {};

namespace {

void add_net(acme_actor_critic* l, NetDesc& d, const char* prefix, int din, int nl,
             const int32_t* sizes, int nout, const char* head) {
  d.din = din;
  d.nl = nl;
  d.nout = nout;
  for (int i = 0; i < nl; ++i) d.sizes[i] = sizes[i];
  const std::string p = std::string(prefix) + "/layer_norm_mlp";
  d.w1 = add_tensor(l, p + "/linear/w", {din, sizes[0]});
  d.b1 = add_tensor(l, p + "/linear/b", {sizes[0]});
  d.scale = add_tensor(l, p + "/layer_norm/scale", {sizes[0]});
  d.offset = add_tensor(l, p + "/layer_norm/offset", {sizes[0]});
  for (int i = 1; i < nl; ++i) {
    const std::string q = p + "/mlp/linear_" + std::to_string(i - 1);
    d.w[i] = add_tensor(l, q + "/w", {sizes[i - 1], sizes[i]});
    d.b[i] = add_tensor(l, q + "/b", {sizes[i]});
  }
  // head == nullptr: the output layer is the LayerNormMLP's own last linear (DDPG's critic,
  // LayerNormMLP(sizes + (1,))).
  const std::string h = head ? std::string(prefix) + "/" + head
                             : p + "/mlp/linear_" + std::to_string(nl - 1);
  d.ow = add_tensor(l, h + "/w", {sizes[nl - 1], nout});
  d.ob = add_tensor(l, h + "/b", {nout});
}

int alloc_acts(acme_actor_critic* l, Acts& a, const NetDesc& d, int rows, bool policy) {
  int rc;
  if ((rc = dev_alloc(l, &a.z1, (int64_t)rows * d.sizes[0])) ||
      (rc = dev_alloc(l, &a.mean, rows)) || (rc = dev_alloc(l, &a.rstd, rows)) ||
      (rc = dev_alloc(l, &a.out, (int64_t)rows * d.nout)))
    return rc;
  for (int i = 0; i < d.nl; ++i)
    if ((rc = dev_alloc(l, &a.h[i], (int64_t)rows * d.sizes[i]))) return rc;
  if (policy && (rc = dev_alloc(l, &a.t, (int64_t)rows * d.nout))) return rc;
  return ACME_OK;
}

// ------------------------------------------------------------------ device helpers

// Sums N per-thread values over a 256-thread block; every thread gets the totals.
template <int N>
__device__ __forceinline__ void block_sum256(float (&v)[N], float (*red)[N]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) red[wave][i] = v[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// ------------------------------------------------------------------ LayerNorm first layer
// h = tanh(LayerNorm(concat(xa, xb) @ W + b)) for kRows rows per 256-thread block.
// Rows < split read (xa0, xb0), the others (xa1, xb1) at row - split.
// The policy head in front of the critic: part p's xb (the actions) computed in the block from
// the policy's last hidden layer when head[p].h is set (and written to head[p].t / .a as
// policy_head_kernel would), instead of read from xb.
struct PolHeadSrc {
  const float* h;  // [rows of the part][Hp], null: xb is given
  float *t, *a;    // tanh outputs, actions
};
struct LnFirstArgs {
  const float *xa0, *xb0, *xa1, *xb1;
  int split, rows, da, db, H;
  const float *w, *b, *scale, *offset;
  float eps;
  float *z, *mean, *rstd, *h;
  PolHeadSrc head[2];
  const float *hw, *hb;  // the policy head of this evaluation's network
};

// Two evaluations in one launch (the online and target networks): blockIdx.y picks the
// argument set; blocks past that set's rows leave at once.
struct LnFirstPair {
  LnFirstArgs a[2];
  const float *lo, *scale;  // TanhToSpec range of the fused policy heads
  int Hp;                   // policy hidden width
};

// One row of a narrow head, lane j < A: h_row . W[:, j] (lane-strided partial sums, then the
// butterfly sum); lanes >= A get 0.  The policy heads of every learner here go through it.
__device__ __forceinline__ float head_dot_row(const float* __restrict__ h, const float* __restrict__ w,
                                              int H, int A, int lane) {
  float acc[ACME_D4PG_MAX_ACT];
#pragma unroll
  for (int j = 0; j < ACME_D4PG_MAX_ACT; ++j) acc[j] = 0.f;
  // Four k steps per chunk with their loads issued together (the sums still run k by k).
  for (int k0 = lane; k0 < H; k0 += 4 * 64) {
    float hv[4], wv[4][ACME_D4PG_MAX_ACT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = min(k0 + 64 * u, H - 1);
      hv[u] = h[k];
#pragma unroll
      for (int j = 0; j < ACME_D4PG_MAX_ACT; ++j) wv[u][j] = j < A ? w[(size_t)k * A + j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (k0 + 64 * u >= H) break;
#pragma unroll
      for (int j = 0; j < ACME_D4PG_MAX_ACT; ++j)
        if (j < A) acc[j] = fmaf(hv[u], wv[u][j], acc[j]);
    }
  }
  float mine = 0.f;
#pragma unroll
  for (int j = 0; j < ACME_D4PG_MAX_ACT; ++j) {
    if (j >= A) break;
    const float s = wave_sum(acc[j]);
    if (lane == j) mine = s;
  }
  return mine;
}

// One row of the deterministic policy head: u_j = h_row . W[:, j] + b_j and the TanhToSpec
// action; policy_head_kernel and the fused head of ln_first_kernel share it, so both give the
// same bits.
__device__ __forceinline__ void policy_head_row(const float* __restrict__ h, const float* __restrict__ w,
                                                const float* __restrict__ b, const float* __restrict__ lo,
                                                const float* __restrict__ scale, int H, int A,
                                                int lane, float& t, float& act) {
  const float mine = head_dot_row(h, w, H, A, lane);
  t = 0.f;
  act = 0.f;
  if (lane < A) {
    t = tanhf(mine + b[lane]);
    act = (0.5f * (t + 1.f)) * scale[lane] + lo[lane];
  }
}

template <int C>  // feature columns per thread: H <= 256 C
__global__ void __launch_bounds__(256) ln_first_kernel(const LnFirstPair pair) {
  __shared__ float xs[kRows][kMaxIn];
  __shared__ float red[4][kRows];
  const LnFirstArgs& a = pair.a[blockIdx.y];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kRows;
  if (r0 >= a.rows) return;  // uniform per block
  const int din = a.da + a.db;
  // Loads that depend on nothing go out first: the bias / LayerNorm parameters of this
  // thread's columns and the first KU input rows of their weights (clamped indices; the
  // products below still run in k order).
  constexpr int KU = 32;
  float bj[C], scj[C], ofj[C], wk[C][KU];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = min(tid + 256 * c, a.H - 1);
    bj[c] = a.b[j];
    scj[c] = a.scale[j];
    ofj[c] = a.offset[j];
#pragma unroll
    for (int u = 0; u < KU; ++u) wk[c][u] = a.w[(size_t)min(u, din - 1) * a.H + j];
  }
  for (int i = tid; i < kRows * din; i += 256) {
    const int r = i / din, k = i - r * din, row = r0 + r;
    float v = 0.f;
    if (row < a.rows) {
      const bool second = row >= a.split;
      const int rr = second ? row - a.split : row;
      if (k >= a.da && a.head[second].h) continue;  // the fused head writes it
      v = k < a.da ? (second ? a.xa1 : a.xa0)[(size_t)rr * a.da + k]
                   : (second ? a.xb1 : a.xb0)[(size_t)rr * a.db + (k - a.da)];
    }
    xs[r][k] = v;
  }
  {
    // Fused policy head: wave r computes row r0 + r's actions.
    static_assert(kRows == 4, "one wave per row of the block");
    const int r = tid >> 6, lane = tid & 63, row = r0 + r;
    const bool second = row >= a.split;
    const PolHeadSrc hs = a.head[second];
    if (row < a.rows && hs.h) {  // uniform per wave
      const int rr = second ? row - a.split : row;
      float t, act;
      policy_head_row(hs.h + (size_t)rr * pair.Hp, a.hw, a.hb, pair.lo, pair.scale, pair.Hp,
                      a.db, lane, t, act);
      if (lane < a.db) {
        if (hs.t) hs.t[(size_t)rr * a.db + lane] = t;
        hs.a[(size_t)rr * a.db + lane] = act;
        xs[r][a.da + lane] = act;
      }
    }
  }
  __syncthreads();
  float acc[kRows][C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = tid + 256 * c;
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r][c] = 0.f;
    if (j < a.H) {
      for (int k0 = 0; k0 < din; k0 += KU) {
        if (k0 > 0) {
#pragma unroll
          for (int u = 0; u < KU; ++u)
            wk[c][u] = k0 + u < din ? a.w[(size_t)(k0 + u) * a.H + j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          if (k0 + u >= din) break;
#pragma unroll
          for (int r = 0; r < kRows; ++r) acc[r][c] = fmaf(xs[r][k0 + u], wk[c][u], acc[r][c]);
        }
      }
#pragma unroll
      for (int r = 0; r < kRows; ++r) acc[r][c] += bj[c];
    }
  }
  // tf.nn.moments over the feature axis: mean, then mean of squared deviations.
  float s[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    s[r] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (tid + 256 * c < a.H) s[r] += acc[r][c];
  }
  block_sum256<kRows>(s, red);
  const float invH = 1.f / (float)a.H;
  float mean[kRows], q[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    mean[r] = s[r] * invH;
    q[r] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (tid + 256 * c < a.H) {
        const float dv = acc[r][c] - mean[r];
        q[r] = fmaf(dv, dv, q[r]);
      }
  }
  block_sum256<kRows>(q, red);
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int row = r0 + r;
    if (row >= a.rows) continue;
    const float rs = 1.f / sqrtf(q[r] * invH + a.eps);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = tid + 256 * c;
      if (j >= a.H) continue;
      const size_t idx = (size_t)row * a.H + j;
      a.z[idx] = acc[r][c];
      const float y = (acc[r][c] - mean[r]) * rs * scj[c] + ofj[c];
      a.h[idx] = tanhf(y);
    }
    if (tid == 0) {
      a.mean[row] = mean[r];
      a.rstd[row] = rs;
    }
  }
}

// ------------------------------------------------------------------ policy head
// One wave per row: u = h @ W + b (A <= 16 outputs), t = tanh(u),
// a = (0.5 (t + 1)) * (max - min) + min  (TanhToSpec, rescaling.py:70-73).
struct PolicyHeadArgs {
  const float *h, *w, *b;
  int rows;
  float *t_out, *a_out;
};
struct PolicyHeadPair {
  PolicyHeadArgs a[2];  // blockIdx.y
  const float *lo, *scale;
  int H, A;
};

__global__ void __launch_bounds__(256) policy_head_kernel(const PolicyHeadPair pr) {
  const PolicyHeadArgs& pa = pr.a[blockIdx.y];
  const float* __restrict__ h = pa.h;
  const float* __restrict__ w = pa.w;
  const float* __restrict__ b = pa.b;
  const float* __restrict__ lo = pr.lo;
  const float* __restrict__ scale = pr.scale;
  const int rows = pa.rows, H = pr.H, A = pr.A;
  float* __restrict__ t_out = pa.t_out;
  float* __restrict__ a_out = pa.a_out;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float t, act;
  policy_head_row(h + (size_t)row * H, w, b, lo, scale, H, A, lane, t, act);
  if (lane < A) {
    if (t_out) t_out[(size_t)row * A + lane] = t;
    a_out[(size_t)row * A + lane] = act;
  }
}

// ------------------------------------------------------------------ loss
// One wave per row (4 rows per 256-thread block); lane i = atom i.
//   rows < B  : categorical TD loss (distributional.py:22-41) with the L2 projection
//               written exactly as l2_project (:44-83); dlogits = (softmax - target) / B,
//               ce[row] = cross-entropy (summed into the loss by adam_clip_kernel).
//   rows >= B : dpg rows; q = sum softmax * values, dq/dlogits = (values - q) * softmax.
// The softmax of one row of logits in registers (lane = atom, -inf past K): its maximum, the
// sum of the exponentials and the lane's probability.
struct RowSoftmax {
  float m, s, p;
};
__device__ __forceinline__ RowSoftmax row_softmax(float x, bool on) {
  RowSoftmax o;
  o.m = wave_max(x);
  const float e = on ? expf(x - o.m) : 0.f;
  o.s = wave_sum(e);
  o.p = e / o.s;
  return o;
}

// The categorical loss of row `row` < B from the online critic's logits ql with their softmax
// q and the target probabilities pj (lane = atom; D4PG: the target critic's softmax, DMPO: the
// mixture over the sampled actions): l2_project, the cross entropy and dlogits = (softmax -
// target) / row_div (the batch size; CRR: R T / (T - 1)).
__device__ __forceinline__ void categorical_loss_row(
    float ql, const RowSoftmax& q, float pj, float vi, int row, int lane,
    const float* __restrict__ r, const float* __restrict__ d, const float* __restrict__ values,
    float row_div, int K, float discount, float* __restrict__ dlogits,
    float* __restrict__ ce_out) {
  const bool on = lane < K;
  const float m2 = q.m, s2 = q.s, sm = q.p;
  const float vmin = values[0], vmax = values[K - 1];
  // Support spacings of l2_project: d_pos = Zq[i+1] - Zq[i] (wrapping to vmin), d_neg =
  // Zq[i] - Zq[i-1] (wrapping to vmax).
  const float dpos = on ? ((lane + 1 < K ? values[lane + 1] : vmin) - vi) : 1.f;
  const float dneg = on ? (vi - (lane > 0 ? values[lane - 1] : vmax)) : 1.f;
  const float gd = discount * d[row];
  const float zc = fminf(fmaxf(r[row] + gd * vi, vmin), vmax);
  // delta_hat = (sg dq) / d_pos - ((1 - sg) dq) / d_neg with sg = (dq >= 0): one of the two
  // terms is an exact zero, so delta_hat = |dq| / (sg ? d_pos : d_neg), the same bits with
  // one division.  Source atom j's values come from lane j by readlane (j is uniform).
  float tgt = 0.f;
  for (int j = 0; j < K; ++j) {
    const float zcj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(zc), j));
    const float pjj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pj), j));
    const float dq = zcj - vi;
    const float dh = fabsf(dq) / (dq >= 0.f ? dpos : dneg);
    tgt += fminf(fmaxf(1.f - dh, 0.f), 1.f) * pjj;
  }
  const float logp = ql - m2 - logf(s2);
  const float ce = wave_sum(on ? -tgt * logp : 0.f);
  if (on) dlogits[(size_t)row * K + lane] = (1.f / row_div) * (sm - tgt);
  if (lane == 0) ce_out[row] = ce;
}

// The loss math of one D4PG row from its logits in registers (ql: the online critic's, tl: the
// target critic's, lane = atom, -inf past K).
__device__ __forceinline__ void loss_row(float ql, float tl, int row, int lane,
                                         const float* __restrict__ r, const float* __restrict__ d,
                                         const float* __restrict__ values, int B, int K,
                                         float discount, float* __restrict__ dlogits,
                                         float* __restrict__ ce_out) {
  const bool on = lane < K;
  const float vi = on ? values[lane] : 0.f;
  const RowSoftmax q = row_softmax(ql, on);
  if (row >= B) {
    const float qv = wave_sum(on ? q.p * vi : 0.f);
    if (on) dlogits[(size_t)row * K + lane] = (vi - qv) * q.p;
    return;
  }
  const RowSoftmax t = row_softmax(tl, on);
  categorical_loss_row(ql, q, t.p, vi, row, lane, r, d, values, (float)B, K, discount, dlogits,
                       ce_out);
}

__global__ void __launch_bounds__(256) d4pg_loss_kernel(
    const float* __restrict__ c_logits, const float* __restrict__ t_logits,
    const float* __restrict__ r, const float* __restrict__ d, const float* __restrict__ values,
    int B, int K, float discount, float* __restrict__ dlogits, float* __restrict__ ce_out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * B) return;
  const bool on = lane < K;
  const float ql = on ? c_logits[(size_t)row * K + lane] : -INFINITY;
  const float tl = on && row < B ? t_logits[(size_t)row * K + lane] : -INFINITY;
  loss_row(ql, tl, row, lane, r, d, values, B, K, discount, dlogits, ce_out);
}

// ------------------------------------------------------------------ DDPG head + TD loss
// The scalar critic head of DDPG (acme/agents/tf/ddpg/learning.py:185-198) forward, the TD
// loss and the head's input gradient in one launch.  One wave per row (4 rows per 256-thread
// block), lane i takes the float4 column groups i, i + 64, ... of the last hidden layer.
//   every row : q = h . w + b (lane partials in k order, then the butterfly sum)
//   rows < B  : q_t from the target critic's row, td = r + discount d q_t - q,
//               loss[row] = 0.5 td^2 (summed into the loss by adam_clip_kernel), dq = -td / B
//   rows >= B : dpg rows, dq = d q / d q = 1
//   dz[row][j] = act'(h[row][j]) * (dq * w[j]): DenseDgrad's epilogue of a K = 1 problem.
struct HeadTdArgs {
  const float *h, *w, *b;     // online critic: last hidden [2B][H], head [H], [1]
  const float *th, *tw, *tb;  // target critic: [B][H], [H], [1]
  const float *r, *d;         // [B]
  int B, H, act;
  float discount;
  float *q, *tq, *td, *dq, *loss;  // [2B], [B], [B], [2B], [B]
  float* dz;                       // [2B][H]
};

__global__ void __launch_bounds__(256) ddpg_head_td_kernel(const HeadTdArgs a) {
  using f32x4 = gemm::f32x4;
  constexpr int kV = kMaxWidth / 256;  // float4 groups per lane
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * a.B) return;  // uniform per wave
  const int n4 = a.H / 4;
  const bool td_row = row < a.B;
  const f32x4* __restrict__ h4 = reinterpret_cast<const f32x4*>(a.h + (size_t)row * a.H);
  const f32x4* __restrict__ w4 = reinterpret_cast<const f32x4*>(a.w);
  const f32x4* __restrict__ th4 =
      reinterpret_cast<const f32x4*>(a.th + (size_t)(td_row ? row : 0) * a.H);
  const f32x4* __restrict__ tw4 = reinterpret_cast<const f32x4*>(a.tw);
  // Every load goes out before the first use (clamped indices; unused groups add nothing).
  f32x4 hv[kV], wv[kV], thv[kV], twv[kV];
#pragma unroll
  for (int u = 0; u < kV; ++u) {
    const int k = min(lane + 64 * u, n4 - 1);
    hv[u] = h4[k];
    wv[u] = w4[k];
    if (td_row) {
      thv[u] = th4[k];
      twv[u] = tw4[k];
    }
  }
  float acc = 0.f, tacc = 0.f;
#pragma unroll
  for (int u = 0; u < kV; ++u) {
    if (lane + 64 * u >= n4) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(hv[u][j], wv[u][j], acc);
    if (td_row) {
#pragma unroll
      for (int j = 0; j < 4; ++j) tacc = fmaf(thv[u][j], twv[u][j], tacc);
    }
  }
  const float q = wave_sum(acc) + a.b[0];
  float dq = 1.f;
  if (td_row) {
    const float tq = wave_sum(tacc) + a.tb[0];
    const float pcont = a.discount * a.d[row];
    const float td = (a.r[row] + pcont * tq) - q;
    dq = -td / (float)a.B;
    if (lane == 0) {
      a.tq[row] = tq;
      a.td[row] = td;
      a.loss[row] = 0.5f * td * td;
    }
  }
  if (lane == 0) {
    a.q[row] = q;
    a.dq[row] = dq;
  }
  f32x4* __restrict__ dz4 = reinterpret_cast<f32x4*>(a.dz + (size_t)row * a.H);
#pragma unroll
  for (int u = 0; u < kV; ++u) {
    const int k = lane + 64 * u;
    if (k >= n4) break;
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = act_bwd(a.act, hv[u][j], dq * wv[u][j]);
    dz4[k] = o;
  }
}

#include "mpo_kernels.h"
#include "crr_kernels.h"

// ------------------------------------------------------------------ LayerNorm backward
// Per row (kRows rows per block): dy = dLoss/d(LayerNorm output) (tanh' already
// applied), xhat = (z - mean) * rstd, g = dy * scale,
//   dz = rstd * (g - mean(g) - xhat * mean(g * xhat))
// Rows < ce_rows: dz is written in place over dy and (dy * xhat, dy) are summed into
// per-block column partials (LayerNorm scale / offset gradients).
// Rows >= ce_rows (the critic's dpg rows): dqda = dz @ W1[act rows]^T, clipped to norm
// <= clip (tf.clip_by_norm; clip <= 0 disables), du = -dqda / B * 0.5 * scale_a * (1-t^2)
// (through TanhToSpec), and 0.5 |dqda|^2 summed into ploss_part[block].
struct LnBwdArgs {
  float* dy;  // [rows][H], overwritten with dz for rows < ce_rows
  const float *z, *mean, *rstd, *scale;
  int rows, ce_rows, H;
  float* colslab;  // [gridDim.x][2][H]
  // dpg
  const float* w1;  // [din][H]
  int act_off, A;
  float clip, invB;
  const float *t, *act_scale;  // [B][A], [A] (policy head tanh, TanhToSpec range)
  float *du, *dqda, *ploss_part;
};

// C: feature columns per thread (H <= 256 C); AM: action slots (A <= AM).  Both sized per
// launch: the widest instantiation (C = 4, AM = 16) spills at H = 512, A = 6.
template <int C, int AM>
__global__ void __launch_bounds__(256) ln_bwd_kernel(const LnBwdArgs a) {
  __shared__ float red[4][2 * kRows];
  __shared__ float redq[4][kRows * AM];
  __shared__ float dq_s[kRows][AM];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kRows;
  const float invH = 1.f / (float)a.H;
  float g[kRows][C], xh[kRows][C], dyv[kRows][C];
  float s[2 * kRows];
  // Every load of the block is issued before the first use: clamped addresses and selects
  // instead of branches around the loads (a branch per load serialises them).  Invalid
  // entries contribute exact zeros to the sums.
  const int last = a.rows - 1;
  const bool has_dpg = r0 + kRows - 1 >= a.ce_rows && r0 < a.rows;  // uniform per block
  float w1v[C][AM];
  if (has_dpg) {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int k = 0; k < AM; ++k)
        w1v[c][k] = a.w1[(size_t)(a.act_off + min(k, a.A - 1)) * a.H + min(tid + 256 * c, a.H - 1)];
  }
  float sc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sc[c] = a.scale[min(tid + 256 * c, a.H - 1)];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int row = r0 + r;
    const bool ok = row < a.rows;
    const float mu0 = a.mean[min(row, last)], rs0 = a.rstd[min(row, last)];
    const float mu = ok ? mu0 : 0.f, rs = ok ? rs0 : 0.f;
    s[2 * r] = s[2 * r + 1] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = tid + 256 * c;
      const bool v = ok && j < a.H;
      const size_t idx = (size_t)min(row, last) * a.H + min(j, a.H - 1);
      const float dy = a.dy[idx], z = a.z[idx];
      dyv[r][c] = v ? dy : 0.f;
      xh[r][c] = v ? (z - mu) * rs : 0.f;
      g[r][c] = v ? dy * sc[c] : 0.f;
      s[2 * r] += g[r][c];
      s[2 * r + 1] = fmaf(g[r][c], xh[r][c], s[2 * r + 1]);
    }
  }
  block_sum256<2 * kRows>(s, red);
  float cs_x[C], cs_1[C];
#pragma unroll
  for (int c = 0; c < C; ++c) cs_x[c] = cs_1[c] = 0.f;
  float dqp[kRows][AM];
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int k = 0; k < AM; ++k) dqp[r][k] = 0.f;
  bool any_dpg = false;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int row = r0 + r;
    if (row >= a.rows) continue;
    const float rs = a.rstd[row];
    const float m1 = s[2 * r] * invH, m2 = s[2 * r + 1] * invH;
    const bool ce = row < a.ce_rows;
    any_dpg |= !ce;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = tid + 256 * c;
      if (j >= a.H) continue;
      const float dz = rs * (g[r][c] - m1 - xh[r][c] * m2);
      if (ce) {
        a.dy[(size_t)row * a.H + j] = dz;
        cs_x[c] = fmaf(dyv[r][c], xh[r][c], cs_x[c]);
        cs_1[c] += dyv[r][c];
      } else {
#pragma unroll
        for (int k = 0; k < AM; ++k)
          dqp[r][k] = k < a.A ? fmaf(dz, w1v[c][k], dqp[r][k]) : dqp[r][k];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = tid + 256 * c;
    if (j < a.H) {
      a.colslab[((size_t)blockIdx.x * 2 + 0) * a.H + j] = cs_x[c];
      a.colslab[((size_t)blockIdx.x * 2 + 1) * a.H + j] = cs_1[c];
    }
  }
  if (!any_dpg) {  // uniform per block: rows are contiguous
    if (tid == 0 && a.ploss_part) a.ploss_part[blockIdx.x] = 0.f;
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int k = 0; k < AM; ++k) {
      if (k >= a.A) break;
      const float v = wave_sum(dqp[r][k]);
      if (lane == 0) redq[wave][r * AM + k] = v;
    }
  __syncthreads();
  if (tid < kRows * AM) {
    const int r = tid / AM, k = tid % AM;
    dq_s[r][k] = ((redq[0][tid] + redq[1][tid]) + redq[2][tid]) + redq[3][tid];
  }
  __syncthreads();
  if (tid < kRows) {
    const int row = r0 + tid;
    float pl = 0.f;
    if (row < a.rows && row >= a.ce_rows) {
      const int b = row - a.ce_rows;
      float n2 = 0.f;
      for (int k = 0; k < a.A; ++k) n2 = fmaf(dq_s[tid][k], dq_s[tid][k], n2);
      // tf.clip_by_norm(t, c): t * c / max(|t|, c), |t| = 0 kept as is.
      const float nrm = n2 > 0.f ? sqrtf(n2) : 0.f;
      const float den = a.clip > 0.f ? fmaxf(nrm, a.clip) : 1.f;
      const float cm = a.clip > 0.f ? a.clip : 1.f;
      for (int k = 0; k < a.A; ++k) {
        const float dq = (dq_s[tid][k] * cm) / den;
        a.dqda[(size_t)b * a.A + k] = dq;
        pl = fmaf(0.5f * dq, dq, pl);
        const float tk = a.t[(size_t)b * a.A + k];
        const float da = -dq * a.invB;
        a.du[(size_t)b * a.A + k] = da * a.act_scale[k] * 0.5f * (1.f - tk * tk);
      }
    }
    // Sum the kRows partials of this block.
    pl += __shfl_down(pl, 2, 64);
    pl += __shfl_down(pl, 1, 64);
    if (tid == 0) a.ploss_part[blockIdx.x] = pl;
  }
}

// ------------------------------------------------------------------ orchestration

// dense_fwd (one layer's forward on the register-operand engine, D4_LAUNCH) and the backward
// launches (BwdGroup, add_wgrad, add_dgrad, launch_multi, launch_bwd): dense_launch.h.

// The same layer of two evaluations (rows0 / rows1 rows, weights w0 / w1) in one launch.
int dense_fwd_pair(const char* name, const float* x0, int rows0, const float* w0,
                   const float* b0, float* y0, const float* x1, int rows1, const float* w1,
                   const float* b1, float* y1, int K, int N, int act, hipStream_t st) {
  if (rows1 == 0) return dense_fwd(name, x0, rows0, K, w0, b0, N, act, y0, st);
  // The direct engine reads W by columns whatever N is; only the x rows' vector loads need
  // K % 4 == 0.
  if (K % 4 != 0) {
    int rc = dense_fwd(name, x0, rows0, K, w0, b0, N, act, y0, st);
    return rc != ACME_OK ? rc : dense_fwd(name, x1, rows1, K, w1, b1, N, act, y1, st);
  }
  return dense_fwd_pair_impl<true>(name, x0, rows0, w0, b0, y0, x1, rows1, w1, b1, y1, K, N, act, st);
}

// One input set of a LayerNormMLP evaluation: rows of concat(xa, xb), the second source
// from row `split` (xa1, xb1), parameters from `prm`, activations into `acts`.
struct NetIn {
  const float* prm;
  const float *xa0, *xb0, *xa1, *xb1;
  int split, rows;
  Acts* acts;
  PolHeadSrc head[2] = {};  // critic inputs: policy heads fused into the first layer
  const float* head_prm = nullptr;  // parameters holding that policy head
};

// Two evaluations of one LayerNormMLP (the online and the target network) in one launch
// per layer: the LayerNorm first layer, the ELU layers.
int lnmlp_forward_pair(acme_actor_critic* l, const NetDesc& d, const NetIn (&in)[2], int da, int db,
                       const char* tag, hipStream_t st) {
  {
    ACME_PROF(tag, st, 2.0 * (in[0].rows + in[1].rows) * (double)(da + db) * d.sizes[0], 0.0);
    LnFirstPair f;
    for (int i = 0; i < 2; ++i) {
      LnFirstArgs& g = f.a[i];
      g.xa0 = in[i].xa0; g.xb0 = in[i].xb0; g.xa1 = in[i].xa1; g.xb1 = in[i].xb1;
      g.split = in[i].split; g.rows = in[i].rows; g.da = da; g.db = db; g.H = d.sizes[0];
      g.w = P(l, in[i].prm, d.w1); g.b = P(l, in[i].prm, d.b1);
      g.scale = P(l, in[i].prm, d.scale); g.offset = P(l, in[i].prm, d.offset);
      g.eps = l->cfg.layer_norm_epsilon;
      Acts& a = *in[i].acts;
      g.z = a.z1; g.mean = a.mean; g.rstd = a.rstd; g.h = a.h[0];
      g.head[0] = in[i].head[0];
      g.head[1] = in[i].head[1];
      g.hw = in[i].head_prm ? P(l, in[i].head_prm, l->pol.ow) : nullptr;
      g.hb = in[i].head_prm ? P(l, in[i].head_prm, l->pol.ob) : nullptr;
    }
    f.lo = l->act_lo; f.scale = l->act_scale; f.Hp = l->pol.sizes[l->pol.nl - 1];
    const int rows = std::max(in[0].rows, in[1].rows);
    const int H = d.sizes[0];
    auto k = H <= 256 ? ln_first_kernel<1> : H <= 512 ? ln_first_kernel<2> : ln_first_kernel<4>;
    k<<<dim3((unsigned)ceil_div(rows, kRows), in[1].rows > 0 ? 2 : 1), 256, 0, st>>>(f);
    ACME_LAUNCH_CHECK();
  }
  for (int i = 1; i < d.nl; ++i) {
    Acts &a0 = *in[0].acts, &a1 = *in[1].acts;
    int rc = dense_fwd_pair("d4pg_mlp_fwd", a0.h[i - 1], in[0].rows, P(l, in[0].prm, d.w[i]),
                            P(l, in[0].prm, d.b[i]), a0.h[i], a1.h[i - 1], in[1].rows,
                            P(l, in[1].prm, d.w[i]), P(l, in[1].prm, d.b[i]), a1.h[i],
                            d.sizes[i - 1], d.sizes[i], ACT_ELU, st);
    if (rc != ACME_OK) return rc;
  }
  return ACME_OK;
}

// Up to two policy evaluations (TanhToSpec actions into out[i]); in[1].rows = 0: one.
int policy_forward_pair(acme_actor_critic* l, const NetIn (&in)[2], float* const (&out)[2],
                        hipStream_t st) {
  const NetDesc& d = l->pol;
  int rc = lnmlp_forward_pair(l, d, in, l->cfg.obs_dim, 0, "d4pg_policy_ln", st);
  if (rc != ACME_OK) return rc;
  const int rows = std::max(in[0].rows, in[1].rows);
  ACME_PROF("d4pg_policy_head", st,
            2.0 * (in[0].rows + in[1].rows) * (double)d.sizes[d.nl - 1] * d.nout, 0.0);
  PolicyHeadPair h;
  for (int i = 0; i < 2; ++i) {
    h.a[i].h = in[i].acts->h[d.nl - 1];
    h.a[i].w = P(l, in[i].prm, d.ow);
    h.a[i].b = P(l, in[i].prm, d.ob);
    h.a[i].rows = in[i].rows;
    h.a[i].t_out = in[i].acts->t;
    h.a[i].a_out = out[i];
  }
  h.lo = l->act_lo; h.scale = l->act_scale; h.H = d.sizes[d.nl - 1]; h.A = d.nout;
  policy_head_kernel<<<dim3((unsigned)ceil_div(rows, 4), in[1].rows > 0 ? 2 : 1), 256, 0,
                       st>>>(h);
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

// The online critic (2B rows: [o_tm1, a_tm1 ; o_t, dpg actions]) and the target critic
// (B rows: [o_t, target actions]).
int critic_forward_pair(acme_actor_critic* l, const NetIn (&in)[2], hipStream_t st) {
  const NetDesc& d = l->cri;
  int rc = lnmlp_forward_pair(l, d, in, l->cfg.obs_dim, l->cfg.act_dim, "d4pg_critic_ln", st);
  if (rc != ACME_OK) return rc;
  Acts &a0 = *in[0].acts, &a1 = *in[1].acts;
  return dense_fwd_pair("d4pg_critic_head", a0.h[d.nl - 1], in[0].rows, P(l, in[0].prm, d.ow),
                        P(l, in[0].prm, d.ob), a0.out, a1.h[d.nl - 1], in[1].rows,
                        P(l, in[1].prm, d.ow), P(l, in[1].prm, d.ob), a1.out,
                        d.sizes[d.nl - 1], d.nout, ACT_NONE, st);
}

inline int act_of_layer(int i) { return i == 0 ? ACT_TANH : ACT_ELU; }

// LayerNorm scale / offset gradients of one LayerNorm: the block partials [nblk][2][H] of
// ln_bwd_kernel, summed after the last one.
struct LnReduce {
  const float* slab;
  int nblk, H;
  float *scale, *offset;
};
// The reduction as a member of the last backward launch (gemm_direct.h kCustom): a
// 512-thread block sums 16 float4 columns over 32 partial groups (group g: partials g, g+32,
// ...), then the groups in order.  M x N = 32 x (32 blocks) sizes the launch's grid.
struct LnReduceBlock {
  static constexpr bool kCustom = true;
  int M, N, K, k_chunk;
  LnReduce r;
  __device__ void run_block(int blk, float* smem) const {
    using f32x4 = gemm::f32x4;
    static_assert(gemm::kDirectWaves == 8, "512-thread blocks");
    f32x4* red = reinterpret_cast<f32x4*>(smem);  // [32][16]
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int count4 = r.H / 2;
    const int e = blk * 16 + c;
    if (blk * 16 >= count4) return;  // block-uniform
    const f32x4* s4 = reinterpret_cast<const f32x4*>(r.slab);
    f32x4 acc{0.f, 0.f, 0.f, 0.f};
    if (e < count4) {
#pragma unroll 4
      for (int sp = g; sp < r.nblk; sp += 32) acc += s4[(size_t)sp * count4 + e];
    }
    red[g * 16 + c] = acc;
    __syncthreads();
    if (g == 0 && e < count4) {
      f32x4 v = red[c];
#pragma unroll
      for (int k = 1; k < 32; ++k) v += red[k * 16 + c];
      const int h4 = r.H / 4;
      if (e < h4) reinterpret_cast<f32x4*>(r.scale)[e] = v;
      else reinterpret_cast<f32x4*>(r.offset)[e - h4] = v;
    }
  }
};

// The step's last backward launch and the LayerNorm parameter reductions in one launch of
// the direct engine (the reductions read only ln_bwd's partials).
int launch_bwd_last(const char* name, BwdGroup& g, const std::vector<LnReduce>& ln,
                    hipStream_t st) {
  std::vector<LnReduceBlock> lr;
  for (const LnReduce& x : ln) {
    LnReduceBlock b;
    b.M = 32;
    b.N = 32 * (int)ceil_div(x.H / 2, 16);
    b.K = 0;
    b.k_chunk = 0;
    b.r = x;
    lr.push_back(b);
  }
  int rc;
  if (g.dgn.empty() && g.wgn.empty())
    rc = launch_multi(name, st, g.dg, g.wg, lr);
  else
    rc = launch_multi(name, st, g.dg, g.wg, g.dgn, g.wgn, lr);
  g = BwdGroup{};
  return rc;
}

// Backward through the MLP part of a LayerNormMLP: `g` holds the launch that forms dz[nl-1]
// (the pre-activation gradient of the last hidden layer, `rows` rows) — it is issued here
// with that layer's weight gradient's predecessor problems.  Each layer's launch: its input
// gradient and its weight gradient (over the first `wrows` rows).  Leaves dLoss/d(LayerNorm
// output) in dz[0].
int lnmlp_backward_mlp(acme_actor_critic* l, const NetDesc& d, const Acts& a, float* const* dz,
                       int rows, int wrows, BwdGroup& g, const char* tag, hipStream_t st,
                       bool dz_ready = false) {
  // dz_ready (DDPG: the head kernel wrote dz[nl-1]): what `g` holds rides with the first
  // layer launch instead of taking one of its own.
  int rc = dz_ready && d.nl > 1 ? ACME_OK : launch_bwd(tag, g, st);
  for (int i = d.nl - 1; i >= 1 && rc == ACME_OK; --i) {
    add_wgrad(g, a.h[i - 1], wrows, d.sizes[i - 1], dz[i], d.sizes[i], Pm(l, l->grads, d.w[i]),
              Pm(l, l->grads, d.b[i]));
    add_dgrad(g, dz[i], rows, d.sizes[i], P(l, l->params, d.w[i]), d.sizes[i - 1], a.h[i - 1],
              act_of_layer(i - 1), dz[i - 1]);
    rc = launch_bwd("d4pg_bwd_mlp", g, st);
  }
  return rc;
}

// LayerNorm backward of the first layer; its weight gradient (concat inputs) joins the next
// backward launch, its scale/offset partials the final reductions.
int ln_backward(acme_actor_critic* l, const NetDesc& d, const Acts& a, float* dy, int rows,
                int ce_rows, bool dpg, const float* xa, const float* xb, int da, int db,
                float* slab, BwdGroup& g, std::vector<LnReduce>& ln, hipStream_t st) {
  const int H = d.sizes[0];
  const int nblk = (int)ceil_div(rows, kRows);
  {
    ACME_PROF("d4pg_ln_bwd", st, 0.0, 0.0);
    LnBwdArgs b;
    b.dy = dy; b.z = a.z1; b.mean = a.mean; b.rstd = a.rstd;
    b.scale = P(l, l->params, d.scale);
    b.rows = rows; b.ce_rows = ce_rows; b.H = H; b.colslab = slab;
    b.w1 = P(l, l->params, d.w1); b.act_off = l->cfg.obs_dim; b.A = l->cfg.act_dim;
    b.clip = l->cfg.clipping ? 1.f : 0.f; b.invB = 1.f / (float)ce_rows;
    b.t = l->pon.t; b.act_scale = l->act_scale;
    b.du = l->du; b.dqda = l->dqda; b.ploss_part = dpg ? l->ploss_part : nullptr;
    const int c = H <= 256 ? 1 : H <= 512 ? 2 : 4;
    const int am = !dpg || b.A <= 4 ? 4 : b.A <= 8 ? 8 : 16;
    auto k = c == 1 ? (am == 4 ? ln_bwd_kernel<1, 4> : am == 8 ? ln_bwd_kernel<1, 8> : ln_bwd_kernel<1, 16>)
           : c == 2 ? (am == 4 ? ln_bwd_kernel<2, 4> : am == 8 ? ln_bwd_kernel<2, 8> : ln_bwd_kernel<2, 16>)
                    : (am == 4 ? ln_bwd_kernel<4, 4> : am == 8 ? ln_bwd_kernel<4, 8> : ln_bwd_kernel<4, 16>);
    k<<<(unsigned)nblk, 256, 0, st>>>(b);
    ACME_LAUNCH_CHECK();
  }
  ln.push_back({slab, nblk, H, Pm(l, l->grads, d.scale), Pm(l, l->grads, d.offset)});
  // dW1 = concat(xa, xb)^T dz: the xa rows and the xb rows of dW1 as two weight gradients
  // (strided operands); the bias gradient (column sums of dz) from the first.
  float* dw = Pm(l, l->grads, d.w1);
  add_wgrad(g, xa, ce_rows, da, dy, H, dw, Pm(l, l->grads, d.b1));
  if (db > 0) add_wgrad(g, xb, ce_rows, db, dy, H, dw + (size_t)da * H, nullptr);
  return ACME_OK;
}

// Global-norm clipping + Adam (t = steps taken including this one) of the policy and critic
// groups in the first `floats` floats.  The policy loss is the sum of ploss[0, n_ploss) over
// div_ploss, the critic loss the sum of ce[0, B) over div_ce; a null output goes to loss_tmp.
int clip_and_adam(acme_actor_critic* l, int64_t floats, const float* ploss, int n_ploss,
                  float div_ploss, int B, float div_ce, float* policy_loss, float* critic_loss,
                  hipStream_t st) {
  ACME_PROF("d4pg_adam", st, 0.0, 7.0 * 4.0 * (double)floats);
  const int64_t n4 = floats / 4, pol4 = l->policy_flat / 4;
  int rc = launch_grad_sumsq(l->grads, n4, pol4, l->norm_part, kNormBlocks, l->dev_step, st);
  if (rc != ACME_OK) return rc;
  ClipAdamArgs a;
  a.p = l->params; a.m = l->m; a.v = l->v; a.g = l->grads; a.n4 = n4; a.group0_4 = pol4;
  a.part = l->norm_part; a.nparts = kNormBlocks; a.clipping = l->cfg.clipping;
  a.clip_norm = 40.f;
  a.lr0 = l->cfg.policy_learning_rate; a.lr1 = l->cfg.critic_learning_rate;
  a.b1 = l->cfg.adam_beta1; a.b2 = l->cfg.adam_beta2; a.eps = l->cfg.adam_epsilon;
  a.dev_step = l->dev_step; a.norms = l->norms;
  a.sum_a = ploss; a.n_a = n_ploss; a.div_a = div_ploss;
  a.out_a = policy_loss ? policy_loss : l->loss_tmp + 1;
  a.sum_b = l->ce; a.n_b = B; a.div_b = div_ce;
  a.out_b = critic_loss ? critic_loss : l->loss_tmp;
  return launch_clip_adam(a, st);
}

int d4pg_step_impl(acme_actor_critic* l, const acme_d4pg_batch* bt, const acme_d4pg_outputs* out,
                   bool copy_target, hipStream_t st) {
  const int B = (int)bt->batch;
  const int od = l->cfg.obs_dim, ad = l->cfg.act_dim;
  const NetDesc& pd = l->pol;
  const NetDesc& cd = l->cri;
  const bool scalar = l->head == Head::kScalar;
  int rc;
  if (copy_target) {
    ACME_PROF("d4pg_target_copy", st, 0.0, 2.0 * 4.0 * (double)l->flat);
    ACME_HIP_TRY(hipMemcpyAsync(l->target, l->params, (size_t)l->flat * sizeof(float),
                                hipMemcpyDeviceToDevice, st));
  }
  // Forwards: the online and target evaluations of each network share every launch.
  {
    const NetIn pin[2] = {{l->params, bt->o_t, nullptr, bt->o_t, nullptr, B, B, &l->pon},
                          {l->target, bt->o_t, nullptr, bt->o_t, nullptr, B, B, &l->ptg}};
    // The policy heads run inside the critic's first-layer launch below (a launch of their
    // own measured 2 us slower per step, profiles/r05/ab/d4pg_fused_head.log).
    if ((rc = lnmlp_forward_pair(l, pd, pin, od, 0, "d4pg_policy_ln", st))) return rc;
  }
  {
    NetIn cin[2] = {{l->params, bt->o_tm1, bt->a_tm1, bt->o_t, l->pon.out, B, 2 * B, &l->con},
                    {l->target, bt->o_t, l->ptg.out, bt->o_t, l->ptg.out, B, B, &l->ctg}};
    // Online rows B.. take the online policy's actions (part 1), every target row the
    // target policy's (part 0).
    cin[0].head[1] = {l->pon.h[pd.nl - 1], l->pon.t, l->pon.out};
    cin[0].head_prm = l->params;
    cin[1].head[0] = {l->ptg.h[pd.nl - 1], l->ptg.t, l->ptg.out};
    cin[1].head_prm = l->target;
    if (scalar)
      rc = lnmlp_forward_pair(l, cd, cin, od, ad, "d4pg_critic_ln", st);
    else
      rc = critic_forward_pair(l, cin, st);
    if (rc) return rc;
  }
  BwdGroup g;
  std::vector<LnReduce> ln;
  const int cL = cd.nl - 1;
  if (scalar) {
    // DDPG: head forward, TD loss and the head's input gradient in one launch; the head's
    // weight gradient (one live column) joins the first backward launch.
    ACME_PROF("ddpg_head_td", st, 2.0 * 5.0 * B * (double)cd.sizes[cL], 0.0);
    HeadTdArgs a;
    a.h = l->con.h[cL]; a.w = P(l, l->params, cd.ow); a.b = P(l, l->params, cd.ob);
    a.th = l->ctg.h[cL]; a.tw = P(l, l->target, cd.ow); a.tb = P(l, l->target, cd.ob);
    a.r = bt->r_t; a.d = bt->d_t;
    a.B = B; a.H = cd.sizes[cL]; a.act = act_of_layer(cL); a.discount = l->cfg.discount;
    a.q = l->con.out; a.tq = l->ctg.out; a.td = l->td; a.dq = l->dq; a.loss = l->ce;
    a.dz = l->cdz[cL];
    ddpg_head_td_kernel<<<(unsigned)ceil_div(2 * B, 4), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
    add_wgrad(g, l->con.h[cL], B, cd.sizes[cL], l->dq, 1, Pm(l, l->grads, cd.ow),
              Pm(l, l->grads, cd.ob));
  } else {
    ACME_PROF("d4pg_loss", st, 0.0, 0.0);
    d4pg_loss_kernel<<<(unsigned)ceil_div(2 * B, 4), 256, 0, st>>>(
        l->con.out, l->ctg.out, bt->r_t, bt->d_t, l->values, B, cd.nout, l->cfg.discount,
        l->dlogits, l->ce);
    ACME_LAUNCH_CHECK();
  }
  // Critic backward: 2B rows of input gradients (CE rows + dpg rows), weight gradients from
  // the first B.  Launch k carries layer k's input gradient and weight gradient.
  if (!scalar) {
    add_wgrad(g, l->con.h[cL], B, cd.sizes[cL], l->dlogits, cd.nout, Pm(l, l->grads, cd.ow),
              Pm(l, l->grads, cd.ob));
    add_dgrad(g, l->dlogits, 2 * B, cd.nout, P(l, l->params, cd.ow), cd.sizes[cL], l->con.h[cL],
              act_of_layer(cL), l->cdz[cL]);
  }
  if ((rc = lnmlp_backward_mlp(l, cd, l->con, l->cdz, 2 * B, B, g, "d4pg_bwd_head", st,
                               scalar)) ||
      (rc = ln_backward(l, cd, l->con, l->cdz[0], 2 * B, B, true, bt->o_tm1, bt->a_tm1, od, ad,
                        l->lnslab, g, ln, st)))
    return rc;
  // Policy backward from du = dloss/d(head pre-activation); its head launch also carries the
  // critic's first-layer weight gradient.
  const int pL = pd.nl - 1;
  add_wgrad(g, l->pon.h[pL], B, pd.sizes[pL], l->du, ad, Pm(l, l->grads, pd.ow),
            Pm(l, l->grads, pd.ob));
  add_dgrad(g, l->du, B, ad, P(l, l->params, pd.ow), pd.sizes[pL], l->pon.h[pL],
            act_of_layer(pL), l->pdz[pL]);
  if ((rc = lnmlp_backward_mlp(l, pd, l->pon, l->pdz, B, B, g, "d4pg_bwd_phead", st)) ||
      (rc = ln_backward(l, pd, l->pon, l->pdz[0], B, B, false, bt->o_t, nullptr, od, 0,
                        l->lnslab2, g, ln, st)) ||
      (rc = launch_bwd_last("d4pg_wgrad_first", g, ln, st)))
    return rc;
  return clip_and_adam(l, l->flat, l->ploss_part, (int)ceil_div(2 * B, kRows), (float)B, B,
                       (float)B, out ? out->policy_loss : nullptr,
                       out ? out->critic_loss : nullptr, st);
}

// ------------------------------------------------------------------ MPO step
// init_scale / softplus(0): what the Gaussian head multiplies its softplus by.
float mpo_scale_mul(const acme_actor_critic* l) {
  return (float)((double)l->mcfg.init_scale / std::log(2.0));
}

// Slot i of a gauss_head_kernel launch (`rows` rows of h, the head's two linears from `prm`)
// and the launch's constants.
void set_gauss_head(const acme_actor_critic* l, GaussHeadPair& p, int i, const float* prm,
                    const float* h, int rows, float* mean, float* pre, float* sd) {
  const NetDesc& pd = l->pol;
  p.a[i] = {h, P(l, prm, pd.ow), P(l, prm, pd.ob), P(l, prm, l->sw), P(l, prm, l->sb), rows,
            mean, pre, sd};
  p.H = pd.sizes[pd.nl - 1]; p.A = l->cfg.act_dim;
  p.scale_mul = mpo_scale_mul(l); p.min_scale = l->mcfg.min_scale;
}

// MPOLearner._step (acme/agents/tf/mpo/learning.py:145-260) on one stream:
//   target policy / critic <- online under their own periods (at the start)      (:159-165)
//   online and target policy on o_t, the Gaussian head of both                   (:193-194)
//   N actions per state from the target policy, their out-of-bound cost, o_t tiled (:197-198)
//   online critic on [o_tm1, a_tm1] (B rows), target critic on the N B samples   (:201-212)
//   head + TD loss against q_t = mean_n                                           (:209-217)
//   MPO loss, its backward into the policy head; dual gradients, stats, dual Adam (:220-224)
//   policy backward, critic backward, global-norm clipping, two Adams             (:236-251)
// The policy head's input gradient is formed by the loss kernel (its two linears' weight
// gradients ride the first policy backward launch), and the policy's backward runs before
// the critic's so that no launch carries more than kZ weight gradients.
//
// The blocks MPO's step shares with DMPO's (dmpo_step_impl) are functions of their own: the
// target copies, the policy side up to the sampled actions, the MPO loss with the duals, and
// the policy backward.

// The two start-of-step target copies: bit 0 of `copy` the policy, bit 1 the critic.
int mpo_target_copies(acme_actor_critic* l, int copy, hipStream_t st) {
  if (copy & 1) {
    ACME_PROF("mpo_target_copy", st, 0.0, 2.0 * 4.0 * (double)l->policy_flat);
    ACME_HIP_TRY(hipMemcpyAsync(l->target, l->params, (size_t)l->policy_flat * sizeof(float),
                                hipMemcpyDeviceToDevice, st));
  }
  if (copy & 2) {
    ACME_PROF("mpo_target_copy", st, 0.0, 2.0 * 4.0 * (double)(l->critic_end - l->policy_flat));
    ACME_HIP_TRY(hipMemcpyAsync(l->target + l->policy_flat, l->params + l->policy_flat,
                                (size_t)(l->critic_end - l->policy_flat) * sizeof(float),
                                hipMemcpyDeviceToDevice, st));
  }
  return ACME_OK;
}

// The online and the target policy on o_t with their Gaussian heads, then N actions per state
// from the target policy, their out-of-bound cost and o_t tiled N times.
int mpo_policy_and_sample(acme_actor_critic* l, const acme_mpo_batch* bt, hipStream_t st) {
  const acme_mpo_config& mc = l->mcfg;
  const int B = (int)bt->batch, N = mc.num_samples, NB = N * B;
  const int od = l->cfg.obs_dim, ad = l->cfg.act_dim;
  const NetDesc& pd = l->pol;
  const int pL = pd.nl - 1;
  auto& mb = l->mb;
  int rc;
  {
    const NetIn pin[2] = {{l->params, bt->o_t, nullptr, bt->o_t, nullptr, B, B, &l->pon},
                          {l->target, bt->o_t, nullptr, bt->o_t, nullptr, B, B, &l->ptg}};
    if ((rc = lnmlp_forward_pair(l, pd, pin, od, 0, "mpo_policy_ln", st))) return rc;
    ACME_PROF("mpo_gauss_head", st, 2.0 * 2.0 * 2.0 * B * (double)pd.sizes[pL] * ad, 0.0);
    GaussHeadPair h;
    set_gauss_head(l, h, 0, l->params, l->pon.h[pL], B, l->pon.out, l->pon.t, mb.sd_on);
    set_gauss_head(l, h, 1, l->target, l->ptg.h[pL], B, l->ptg.out, l->ptg.t, mb.sd_t);
    gauss_head_kernel<<<dim3((unsigned)ceil_div(B, 4), 2), 256, 0, st>>>(h);
    ACME_LAUNCH_CHECK();
  }
  {
    ACME_PROF("mpo_sample", st, 0.0, 4.0 * NB * (3.0 * ad + od + 1.0));
    MpoSampleArgs a;
    a.mean = l->ptg.out; a.sd = mb.sd_t; a.noise_in = bt->noise; a.o_t = bt->o_t;
    a.dev_step = l->dev_step; a.seed = mc.seed;
    a.B = B; a.N = N; a.A = ad; a.od = od;
    a.noise = mb.noise; a.act = mb.act; a.cost = mb.cost; a.tiled = mb.tiled;
    mpo_sample_kernel<<<(unsigned)ceil_div(NB, 256), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  return ACME_OK;
}

// The MPO loss over the sampled values mb.sq with its backward into the policy head (dz[pL],
// dmean, dpre), then the dual gradients, the stats and the duals' Adam.
int mpo_loss_and_duals(acme_actor_critic* l, const acme_mpo_batch* bt, const acme_mpo_outputs* out,
                       hipStream_t st) {
  const acme_mpo_config& mc = l->mcfg;
  const int B = (int)bt->batch, N = mc.num_samples;
  const int ad = l->cfg.act_dim;
  const int D = mc.per_dim_constraining ? ad : 1;
  const NetDesc& pd = l->pol;
  const int pL = pd.nl - 1;
  auto& mb = l->mb;
  const float scale_mul = mpo_scale_mul(l);
  const int nblk = (int)ceil_div(B, 4);
  float* stats = out && out->stats ? out->stats : mb.stats;
  float* klm_rel = out && out->kl_mean_rel ? out->kl_mean_rel : mb.klm_rel;
  float* kls_rel = out && out->kl_stddev_rel ? out->kl_stddev_rel : mb.kls_rel;
  {
    ACME_PROF("mpo_loss", st, 0.0, 0.0);
    MpoLossArgs a;
    a.sq = mb.sq; a.cost = mb.cost; a.act = mb.act;
    a.mu_on = l->pon.out; a.sd_on = mb.sd_on; a.pre_on = l->pon.t;
    a.mu_t = l->ptg.out; a.sd_t = mb.sd_t;
    a.log_temp = P(l, l->params, l->t_temp); a.log_amean = P(l, l->params, l->t_amean);
    a.log_astd = P(l, l->params, l->t_astd);
    a.log_ptemp = l->t_ptemp >= 0 ? P(l, l->params, l->t_ptemp) : nullptr;
    a.B = B; a.N = N; a.A = ad; a.D = D; a.H = pd.sizes[pL]; a.act_fn = act_of_layer(pL);
    a.scale_mul = scale_mul;
    a.h = l->pon.h[pL]; a.wm = P(l, l->params, pd.ow); a.ws = P(l, l->params, l->sw);
    a.dmean = mb.dmean; a.dpre = mb.dpre; a.dz = l->pdz[pL];
    a.w_out = mb.w; a.pw_out = mb.pw; a.part = mb.part;
    mpo_loss_kernel<<<(unsigned)nblk, 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  {
    ACME_PROF("mpo_finalize", st, 0.0, 0.0);
    MpoFinalArgs a;
    a.part = mb.part; a.nblk = nblk; a.B = B; a.N = N; a.A = ad; a.D = D;
    a.penal = l->t_ptemp >= 0;
    a.p = l->params; a.g = l->grads; a.m = l->m; a.v = l->v;
    a.o_temp = l->tensors[l->t_temp].offset; a.o_amean = l->tensors[l->t_amean].offset;
    a.o_astd = l->tensors[l->t_astd].offset;
    a.o_ptemp = l->t_ptemp >= 0 ? l->tensors[l->t_ptemp].offset : -1;
    a.eps = mc.epsilon; a.eps_mean = mc.epsilon_mean; a.eps_std = mc.epsilon_stddev;
    a.eps_pen = mc.epsilon_penalty;
    a.lr = mc.dual_learning_rate; a.b1 = l->cfg.adam_beta1; a.b2 = l->cfg.adam_beta2;
    a.adam_eps = l->cfg.adam_epsilon; a.dev_step = l->dev_step;
    a.stats = stats; a.klm_rel = klm_rel; a.kls_rel = kls_rel; a.ploss = mb.ploss;
    mpo_finalize_kernel<<<1, 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  return ACME_OK;
}

// Policy backward from dz[pL] (written by the loss kernel) over the B rows `obs` the online
// policy ran on; leaves the first layer's weight gradient in `g` for the critic's first
// backward launch.
int mpo_policy_backward(acme_actor_critic* l, int B, const float* obs, BwdGroup& g,
                        std::vector<LnReduce>& ln, hipStream_t st) {
  const int od = l->cfg.obs_dim, ad = l->cfg.act_dim;
  const NetDesc& pd = l->pol;
  const int pL = pd.nl - 1;
  auto& mb = l->mb;
  int rc;
  add_wgrad(g, l->pon.h[pL], B, pd.sizes[pL], mb.dmean, ad, Pm(l, l->grads, pd.ow),
            Pm(l, l->grads, pd.ob));
  add_wgrad(g, l->pon.h[pL], B, pd.sizes[pL], mb.dpre, ad, Pm(l, l->grads, l->sw),
            Pm(l, l->grads, l->sb));
  if ((rc = lnmlp_backward_mlp(l, pd, l->pon, l->pdz, B, B, g, "mpo_bwd_phead", st, true)))
    return rc;
  return ln_backward(l, pd, l->pon, l->pdz[0], B, B, false, obs, nullptr, od, 0, l->lnslab2, g,
                     ln, st);
}

int mpo_step_impl(acme_actor_critic* l, const acme_mpo_batch* bt, const acme_mpo_outputs* out,
                  int copy, hipStream_t st) {
  const int B = (int)bt->batch, N = l->mcfg.num_samples, NB = N * B;
  const int od = l->cfg.obs_dim, ad = l->cfg.act_dim;
  const NetDesc& cd = l->cri;
  const int cL = cd.nl - 1;
  auto& mb = l->mb;
  int rc;
  if ((rc = mpo_target_copies(l, copy, st)) || (rc = mpo_policy_and_sample(l, bt, st))) return rc;
  {
    const NetIn cin[2] = {{l->params, bt->o_tm1, bt->a_tm1, bt->o_tm1, bt->a_tm1, B, B, &l->con},
                          {l->target, mb.tiled, mb.act, mb.tiled, mb.act, NB, NB, &l->ctg}};
    if ((rc = lnmlp_forward_pair(l, cd, cin, od, ad, "mpo_critic_ln", st))) return rc;
  }
  {
    ACME_PROF("mpo_head_td", st, 2.0 * (NB + 2.0 * B) * (double)cd.sizes[cL], 0.0);
    MpoHeadTdArgs a;
    a.h = l->con.h[cL]; a.w = P(l, l->params, cd.ow); a.b = P(l, l->params, cd.ob);
    a.th = l->ctg.h[cL]; a.tw = P(l, l->target, cd.ow); a.tb = P(l, l->target, cd.ob);
    a.r = bt->r_t; a.d = bt->d_t;
    a.B = B; a.N = N; a.H = cd.sizes[cL]; a.act = act_of_layer(cL); a.discount = l->cfg.discount;
    a.q = l->con.out; a.sq = mb.sq; a.qt = mb.qt; a.td = l->td; a.dq = l->dq; a.loss = l->ce;
    a.dz = l->cdz[cL];
    mpo_head_td_kernel<<<(unsigned)ceil_div(B, 4), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  BwdGroup g;
  std::vector<LnReduce> ln;
  if ((rc = mpo_loss_and_duals(l, bt, out, st)) ||
      (rc = mpo_policy_backward(l, B, bt->o_t, g, ln, st)))
    return rc;
  // Critic backward over the B TD rows; the head's weight gradient (one live column) and the
  // policy's first-layer weight gradient ride its first launch.
  add_wgrad(g, l->con.h[cL], B, cd.sizes[cL], l->dq, 1, Pm(l, l->grads, cd.ow),
            Pm(l, l->grads, cd.ob));
  if ((rc = lnmlp_backward_mlp(l, cd, l->con, l->cdz, B, B, g, "mpo_bwd_chead", st, true)) ||
      (rc = ln_backward(l, cd, l->con, l->cdz[0], B, B, false, bt->o_tm1, bt->a_tm1, od, ad,
                        l->lnslab, g, ln, st)) ||
      (rc = launch_bwd_last("d4pg_wgrad_first", g, ln, st)))
    return rc;
  // The duals' floats past critic_end are the finalize kernel's.
  return clip_and_adam(l, l->critic_end, mb.ploss, 1, 1.f, B, (float)B,
                       out ? out->policy_loss : nullptr,
                       out ? out->critic_loss : nullptr, st);
}

// DistributionalMPOLearner._step (acme/agents/tf/dmpo/learning.py:147-276) on one stream: MPO's
// step with D4PG's categorical critic.
//   target copies, policy side, sampling: MPO's blocks                             (:161-204)
//   online critic on [o_tm1, a_tm1] (B rows), target critic on the N B samples, the
//     DiscreteValuedHead of both in one launch (B and N B rows)                    (:207-224)
//   dmpo_mix_loss_kernel: sampled q, the bootstrap mixture of each state, the categorical
//     loss and dlogits of the B online rows                                        (:212-233)
//   MPO loss and duals, policy backward: MPO's blocks                              (:236-240)
//   critic backward as D4PG's over the B rows (no dpg rows), clipping, two Adams   (:252-267)
// Launches at B = 256, N = 20, policy 256x3, critic 512/512/256, no target copy: policy 3 + 1,
// sample 1, critic 3 + 1 head, mixture loss 1, MPO loss 2, policy backward 2 + 1, critic
// backward 1 + 2 + 1 + 1, clipping and Adam 2: 22, two more than MPO's 20 (the head GEMM pair
// and the head's backward launch; the mixture kernel stands where mpo_head_td_kernel stood,
// which also wrote the scalar head's input gradient).
int dmpo_step_impl(acme_actor_critic* l, const acme_mpo_batch* bt, const acme_mpo_outputs* out,
                   int copy, hipStream_t st) {
  const int B = (int)bt->batch, N = l->mcfg.num_samples, NB = N * B;
  const int od = l->cfg.obs_dim, ad = l->cfg.act_dim;
  const NetDesc& cd = l->cri;
  const int cL = cd.nl - 1, K = cd.nout;
  auto& mb = l->mb;
  int rc;
  if ((rc = mpo_target_copies(l, copy, st)) || (rc = mpo_policy_and_sample(l, bt, st))) return rc;
  {
    const NetIn cin[2] = {{l->params, bt->o_tm1, bt->a_tm1, bt->o_tm1, bt->a_tm1, B, B, &l->con},
                          {l->target, mb.tiled, mb.act, mb.tiled, mb.act, NB, NB, &l->ctg}};
    if ((rc = critic_forward_pair(l, cin, st))) return rc;
  }
  {
    ACME_PROF("dmpo_mix_loss", st, 0.0, 4.0 * (double)K * (NB + 3.0 * B));
    DmpoMixArgs a;
    a.c_logits = l->con.out; a.t_logits = l->ctg.out;
    a.r = bt->r_t; a.d = bt->d_t; a.values = l->values;
    a.B = B; a.N = N; a.K = K; a.discount = l->cfg.discount; a.row_div = (float)B;
    a.sq = mb.sq; a.mix = l->mixture; a.dlogits = l->dlogits; a.ce = l->ce;
    dmpo_mix_loss_kernel<<<(unsigned)ceil_div(B, 4), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  BwdGroup g;
  std::vector<LnReduce> ln;
  // The policy's backward first, as in MPO: no launch carries more than kZ weight gradients.
  if ((rc = mpo_loss_and_duals(l, bt, out, st)) ||
      (rc = mpo_policy_backward(l, B, bt->o_t, g, ln, st)))
    return rc;
  // Critic backward over the B rows: the head's launch (its weight and input gradients) also
  // carries the policy's first-layer weight gradient.
  add_wgrad(g, l->con.h[cL], B, cd.sizes[cL], l->dlogits, K, Pm(l, l->grads, cd.ow),
            Pm(l, l->grads, cd.ob));
  add_dgrad(g, l->dlogits, B, K, P(l, l->params, cd.ow), cd.sizes[cL], l->con.h[cL],
            act_of_layer(cL), l->cdz[cL]);
  if ((rc = lnmlp_backward_mlp(l, cd, l->con, l->cdz, B, B, g, "dmpo_bwd_chead", st, false)) ||
      (rc = ln_backward(l, cd, l->con, l->cdz[0], B, B, false, bt->o_tm1, bt->a_tm1, od, ad,
                        l->lnslab, g, ln, st)) ||
      (rc = launch_bwd_last("d4pg_wgrad_first", g, ln, st)))
    return rc;
  return clip_and_adam(l, l->critic_end, mb.ploss, 1, 1.f, B, (float)B,
                       out ? out->policy_loss : nullptr,
                       out ? out->critic_loss : nullptr, st);
}

// RCRRLearner._step (acme/agents/tf/crr/recurrent_learning.py:197-377) for stateless networks
// on one stream, over the R = B (T - 1) transitions its loop over t unrolls into; every batch
// mean of the reference is sum_rows / row_div with row_div = R T / (T - 1) (:327-334).
//   online policy on o_tm1, target policy on o_t, the Gaussian head of both        (:250, :279)
//   crr_sample_kernel: N_td actions per state from the target policy at o_t and N_pw from the
//     online policy at o_tm1, the observations tiled beside them          (:253-257, :285-290)
//   online critic on [o_tm1, a_tm1 ; tiled o_tm1, online samples] (R + N_pw R rows), target
//     critic on the N_td R target samples, the DiscreteValuedHead of both   (:248, :262, :291)
//   dmpo_mix_loss_kernel: the bootstrap mixture, the categorical loss, dlogits     (:265-276)
//   crr_policy_loss_kernel: V, the advantage, the coefficient, -log pi(a_tm1) coef with its
//     backward into the policy head                                                (:293-323)
//   policy backward as MPO's, critic backward as DMPO's over the first R rows (no gradient
//     through the sampled rows), clipping, two Adams                               (:337-359)
//   target <- online AFTER the update when num_steps % period == 0                 (:361-371)
// Launches at R = 256, policy 256x3, critic 512/512/256, no target copy: policy 3 + 1, sample 1,
// critic 3 + 1 head, mixture loss 1, policy loss 1, policy backward 2 + 1, critic backward
// 1 + 2 + 1 + 1, the coefficient's mean 1, clipping and Adam 2: 22, as DMPO (the one-wave mean
// where mpo_finalize_kernel stands).
int crr_step_impl(acme_actor_critic* l, const acme_crr_batch* bt, const acme_crr_outputs* out,
                  bool copy_target, hipStream_t st) {
  const acme_crr_config& cc = l->ccfg;
  const int R = (int)bt->batch;
  const int Ntd = cc.num_action_samples_td_learning, Npw = cc.num_action_samples_policy_weight;
  const int od = l->cfg.obs_dim, ad = l->cfg.act_dim;
  const NetDesc& pd = l->pol;
  const NetDesc& cd = l->cri;
  const int pL = pd.nl - 1, cL = cd.nl - 1, K = cd.nout;
  const float row_div =
      (float)((double)R * cc.sequence_length / (double)(cc.sequence_length - 1));
  auto& mb = l->mb;
  auto& cb = l->cb;
  // The online samples' rows of the concatenated noise / actions / tiled buffers.
  const float* act_on = mb.act + (size_t)Ntd * R * ad;
  const float* tiled_on = mb.tiled + (size_t)Ntd * R * od;
  int rc;
  {
    const NetIn pin[2] = {{l->params, bt->o_tm1, nullptr, bt->o_tm1, nullptr, R, R, &l->pon},
                          {l->target, bt->o_t, nullptr, bt->o_t, nullptr, R, R, &l->ptg}};
    if ((rc = lnmlp_forward_pair(l, pd, pin, od, 0, "crr_policy_ln", st))) return rc;
    ACME_PROF("crr_gauss_head", st, 2.0 * 2.0 * 2.0 * R * (double)pd.sizes[pL] * ad, 0.0);
    GaussHeadPair h;
    set_gauss_head(l, h, 0, l->params, l->pon.h[pL], R, l->pon.out, l->pon.t, mb.sd_on);
    set_gauss_head(l, h, 1, l->target, l->ptg.h[pL], R, l->ptg.out, l->ptg.t, mb.sd_t);
    gauss_head_kernel<<<dim3((unsigned)ceil_div(R, 4), 2), 256, 0, st>>>(h);
    ACME_LAUNCH_CHECK();
  }
  {
    const int rows = (Ntd + Npw) * R;
    ACME_PROF("crr_sample", st, 0.0, 4.0 * rows * (3.0 * ad + od));
    CrrSampleArgs a;
    a.mean_t = l->ptg.out; a.sd_t = mb.sd_t; a.mean_on = l->pon.out; a.sd_on = mb.sd_on;
    a.noise_in = bt->noise; a.o_t = bt->o_t; a.o_tm1 = bt->o_tm1;
    a.dev_step = l->dev_step; a.seed = cc.seed;
    a.R = R; a.Ntd = Ntd; a.Npw = Npw; a.A = ad; a.od = od;
    a.noise = mb.noise; a.act = mb.act; a.tiled = mb.tiled;
    // One thread per tiled observation element as well: at rows = 1,280 a grid sized by the
    // rows alone leaves the tiling's grid-stride loop 24 serial passes on five blocks.
    const int64_t threads = (int64_t)rows * od;
    crr_sample_kernel<<<(unsigned)ceil_div(threads, 256), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  {
    const NetIn cin[2] = {
        {l->params, bt->o_tm1, bt->a_tm1, tiled_on, act_on, R, R + Npw * R, &l->con},
        {l->target, mb.tiled, mb.act, mb.tiled, mb.act, Ntd * R, Ntd * R, &l->ctg}};
    if ((rc = critic_forward_pair(l, cin, st))) return rc;
  }
  {
    ACME_PROF("crr_mix_loss", st, 0.0, 4.0 * (double)K * (Ntd * R + 3.0 * R));
    DmpoMixArgs a;
    a.c_logits = l->con.out; a.t_logits = l->ctg.out;
    a.r = bt->r_t; a.d = bt->d_t; a.values = l->values;
    a.B = R; a.N = Ntd; a.K = K; a.discount = l->cfg.discount; a.row_div = row_div;
    a.sq = mb.sq; a.mix = l->mixture; a.dlogits = l->dlogits; a.ce = l->ce;
    dmpo_mix_loss_kernel<<<(unsigned)ceil_div(R, 4), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  const int nblk = (int)ceil_div(R, 4);
  {
    ACME_PROF("crr_policy_loss", st, 0.0, 4.0 * (double)K * (Npw * R + R));
    CrrLossArgs a;
    a.logits = l->con.out; a.values = l->values;
    a.a_tm1 = bt->a_tm1; a.mu = l->pon.out; a.sd = mb.sd_on; a.pre = l->pon.t;
    a.R = R; a.N = Npw; a.K = K; a.A = ad; a.H = pd.sizes[pL]; a.act_fn = act_of_layer(pL);
    a.reduce = cc.baseline_reduce_function; a.mode = cc.policy_improvement_modes;
    a.beta = cc.beta; a.bound = cc.ratio_upper_bound; a.scale_mul = mpo_scale_mul(l);
    a.row_div = row_div;
    a.h = l->pon.h[pL]; a.wm = P(l, l->params, pd.ow); a.ws = P(l, l->params, l->sw);
    a.q_mean = cb.q_mean; a.v_est = cb.v_est; a.adv = cb.adv; a.coef = cb.coef; a.logp = cb.logp;
    a.dmean = mb.dmean; a.dpre = mb.dpre; a.dz = l->pdz[pL];
    a.loss_part = l->ploss_part; a.coef_part = cb.coef_part;
    crr_policy_loss_kernel<<<(unsigned)nblk, 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  BwdGroup g;
  std::vector<LnReduce> ln;
  // The policy's backward first, as in MPO: no launch carries more than kZ weight gradients.
  if ((rc = mpo_policy_backward(l, R, bt->o_tm1, g, ln, st))) return rc;
  // Critic backward as DMPO's over the first R rows of the online critic's activations.
  add_wgrad(g, l->con.h[cL], R, cd.sizes[cL], l->dlogits, K, Pm(l, l->grads, cd.ow),
            Pm(l, l->grads, cd.ob));
  add_dgrad(g, l->dlogits, R, K, P(l, l->params, cd.ow), cd.sizes[cL], l->con.h[cL],
            act_of_layer(cL), l->cdz[cL]);
  if ((rc = lnmlp_backward_mlp(l, cd, l->con, l->cdz, R, R, g, "crr_bwd_chead", st, false)) ||
      (rc = ln_backward(l, cd, l->con, l->cdz[0], R, R, false, bt->o_tm1, bt->a_tm1, od, ad,
                        l->lnslab, g, ln, st)) ||
      (rc = launch_bwd_last("d4pg_wgrad_first", g, ln, st)))
    return rc;
  {
    // The logged mean coefficient (clip_adam's logged-loss path has room for two sums: the
    // policy loss's block partials and ce go there).
    ACME_PROF("crr_coef_mean", st, 0.0, 0.0);
    float* dst = out && out->policy_loss_coef ? out->policy_loss_coef : l->loss_tmp + 2;
    crr_coef_mean_kernel<<<1, 64, 0, st>>>(cb.coef_part, nblk, row_div, dst);
    ACME_LAUNCH_CHECK();
  }
  if ((rc = clip_and_adam(l, l->critic_end, l->ploss_part, nblk, row_div, R, row_div,
                          out ? out->policy_loss : nullptr, out ? out->critic_loss : nullptr,
                          st)))
    return rc;
  if (copy_target) {
    ACME_PROF("crr_target_copy", st, 0.0, 2.0 * 4.0 * (double)l->critic_end);
    ACME_HIP_TRY(hipMemcpyAsync(l->target, l->params, (size_t)l->critic_end * sizeof(float),
                                hipMemcpyDeviceToDevice, st));
  }
  return ACME_OK;
}

// ------------------------------------------------------------------ step graphs
// The launches of a step (D4PG and MPO 20, DDPG 18, DMPO and CRR 22 and, on CRR's period, the
// memcpy node of its post-update target copy) are captured once per (batch pointers, outputs,
// B, target copy) into a hipGraph on a private capture stream and replayed with one
// hipGraphLaunch on the caller's stream: the launch cost leaves the host critical path.
// ACME_NO_GRAPH=1 disables capture; the section profiler also bypasses it (its event
// records belong to individual launches).
bool graphs_enabled() {
  static const bool on = getenv("ACME_NO_GRAPH") == nullptr;
  return on;
}

// `record(stream)` issues the step's launches; `copy` holds the target-copy flags.
template <class F>
int run_graph(acme_actor_critic* l, const void* const (&key)[kGraphKeys], int64_t B, int copy,
              hipStream_t st, F&& record) {
  for (auto& g : l->graphs)
    if (g.B == B && g.copy == copy && memcmp(g.key, key, sizeof(key)) == 0) {
      ACME_HIP_TRY(hipGraphLaunch(g.exec, st));
      return ACME_OK;
    }
  if (l->graphs.size() >= 16) {  // a caller cycling many buffers: start over
    for (auto& g : l->graphs) (void)hipGraphExecDestroy(g.exec);
    l->graphs.clear();
  }
  if (!l->capture) ACME_HIP_TRY(hipStreamCreateWithFlags(&l->capture, hipStreamNonBlocking));
  ACME_HIP_TRY(hipStreamBeginCapture(l->capture, hipStreamCaptureModeRelaxed));
  int rc = record(l->capture);
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture(l->capture, &graph);
  if (rc != ACME_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (e != hipSuccess) {
    set_error("step graph capture failed: %s", hipGetErrorString(e));
    return ACME_ERR_HIP;
  }
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) {
    set_error("step graph instantiation failed: %s", hipGetErrorString(e));
    return ACME_ERR_HIP;
  }
  acme_actor_critic::Graph g;
  memcpy(g.key, key, sizeof(key));
  g.B = B;
  g.copy = copy;
  g.exec = exec;
  l->graphs.push_back(g);
  ACME_HIP_TRY(hipGraphLaunch(exec, st));
  return ACME_OK;
}

// The entry of every step (l and batch non-null, l of the right head kind): the checks the
// batch types share, then `record(stream)` replayed from the graph keyed by `key`, B and the
// target-copy flags `copy`, or issued eagerly; a step that was issued is counted.  `api`
// names the caller's family in the messages.
template <class Batch, class F>
int run_step(acme_actor_critic* l, const char* api, const Batch* batch,
             const void* const (&key)[kGraphKeys], int copy, void* stream, F&& record) {
  ACME_CHECK_ARG(l->params, "%s_bind must be called first", api);
  ACME_CHECK_ARG(batch->batch >= 1 && batch->batch <= l->cfg.max_batch,
                 "batch %lld outside [1, max_batch=%d]", (long long)batch->batch,
                 l->cfg.max_batch);
  ACME_CHECK_ARG(batch->o_tm1 && batch->a_tm1 && batch->r_t && batch->d_t && batch->o_t,
                 "null batch field");
  hipStream_t st = as_stream(stream);
  const int rc = graphs_enabled() && !prof::enabled()
                     ? run_graph(l, key, batch->batch, copy, st, record)
                     : record(st);
  if (rc != ACME_OK) return rc;
  l->num_steps += 1;
  return ACME_OK;
}

// ------------------------------------------------------------------ the shared learner
// The bodies behind the acme_d4pg_*, acme_ddpg_*, acme_mpo_*, acme_dmpo_* and acme_crr_* exports.

int ac_destroy(acme_actor_critic* l) {
  if (!l) return ACME_OK;
  (void)hipDeviceSynchronize();  // queued work of this learner finishes before its buffers go
  for (auto& g : l->graphs) (void)hipGraphExecDestroy(g.exec);
  if (l->capture) (void)hipStreamDestroy(l->capture);
  for (void* p : l->allocs) (void)hipFree(p);
  delete l;
  return ACME_OK;
}

int check_config(const acme_d4pg_config* cfg, Head head) {
  ACME_CHECK_ARG(cfg->obs_dim >= 1 && cfg->act_dim >= 1 && cfg->obs_dim + cfg->act_dim <= kMaxIn,
                 "obs_dim + act_dim must be in [2, %d]", kMaxIn);
  ACME_CHECK_ARG(cfg->act_dim <= ACME_D4PG_MAX_ACT, "act_dim must be <= %d", ACME_D4PG_MAX_ACT);
  ACME_CHECK_ARG(cfg->max_batch >= 1 && cfg->max_batch <= 65536, "max_batch must be in [1, 65536]");
  if (is_categorical(head)) {
    ACME_CHECK_ARG(cfg->num_atoms >= 2 && cfg->num_atoms <= ACME_D4PG_MAX_ATOMS,
                   "num_atoms must be in [2, %d]", ACME_D4PG_MAX_ATOMS);
    ACME_CHECK_ARG(cfg->vmax > cfg->vmin, "vmax must exceed vmin");
  }
  ACME_CHECK_ARG(cfg->target_update_period >= 1, "target_update_period must be >= 1");
  for (int n : {cfg->num_policy_layers, cfg->num_critic_layers})
    ACME_CHECK_ARG(n >= 1 && n <= ACME_D4PG_MAX_LAYERS, "layer count must be in [1, %d]",
                   ACME_D4PG_MAX_LAYERS);
  for (int i = 0; i < cfg->num_policy_layers; ++i)
    ACME_CHECK_ARG(cfg->policy_sizes[i] >= 4 && cfg->policy_sizes[i] <= kMaxWidth &&
                       cfg->policy_sizes[i] % 4 == 0,
                   "policy layer sizes must be multiples of 4 in [4, %d]", kMaxWidth);
  for (int i = 0; i < cfg->num_critic_layers; ++i)
    ACME_CHECK_ARG(cfg->critic_sizes[i] >= 4 && cfg->critic_sizes[i] <= kMaxWidth &&
                       cfg->critic_sizes[i] % 4 == 0,
                   "critic layer sizes must be multiples of 4 in [4, %d]", kMaxWidth);
  return ACME_OK;
}

// Lays out the tensors and allocates the workspaces of a fresh learner.  Head::kScalar and
// Head::kMpo come with cfg->num_atoms = 1 (the support unused); Head::kMpo and
// Head::kMpoCategorical with `mpo`, Head::kCrr with `crr`.
int init_learner(acme_actor_critic* l, const acme_d4pg_config* cfg, Head head,
                 const acme_mpo_config* mpo, const acme_crr_config* crr = nullptr) {
  l->cfg = *cfg;
  l->head = head;
  const bool gauss = mpo || crr;
  add_net(l, l->pol, "policy", cfg->obs_dim, cfg->num_policy_layers, cfg->policy_sizes,
          cfg->act_dim,
          gauss ? "multivariate_normal_diag_head/linear" : "near_zero_initialized_linear");
  if (gauss) {
    const int64_t hl = cfg->policy_sizes[cfg->num_policy_layers - 1];
    l->sw = add_tensor(l, "policy/multivariate_normal_diag_head/linear_1/w", {hl, cfg->act_dim});
    l->sb = add_tensor(l, "policy/multivariate_normal_diag_head/linear_1/b", {cfg->act_dim});
  }
  l->policy_flat = l->flat;
  add_net(l, l->cri, "critic", cfg->obs_dim + cfg->act_dim, cfg->num_critic_layers,
          cfg->critic_sizes, cfg->num_atoms,
          is_categorical(head) ? "discrete_valued_head/linear" : nullptr);
  l->critic_end = l->flat;
  if (mpo) {
    l->mcfg = *mpo;
    const int64_t D = mpo->per_dim_constraining ? cfg->act_dim : 1;
    l->t_temp = add_tensor(l, "mpo/log_temperature", {1});
    l->t_amean = add_tensor(l, "mpo/log_alpha_mean", {D});
    l->t_astd = add_tensor(l, "mpo/log_alpha_stddev", {D});
    if (mpo->action_penalization) l->t_ptemp = add_tensor(l, "mpo/log_penalty_temperature", {1});
  }
  const int B = cfg->max_batch;
  if (crr) {
    // The Gaussian head's constants and the noise key live where MPO's kernels' setup reads them.
    l->ccfg = *crr;
    memset(&l->mcfg, 0, sizeof(l->mcfg));
    l->mcfg.init_scale = crr->init_scale;
    l->mcfg.min_scale = crr->min_scale;
    l->mcfg.seed = crr->seed;
    l->crr_rows = B;
  }
  const int ntd = crr ? crr->num_action_samples_td_learning : 0;
  const int npw = crr ? crr->num_action_samples_policy_weight : 0;
  // MPO: the online critic sees the B TD rows only, the target critic the N B samples.  CRR:
  // the online critic the B rows and its N_pw B samples, the target critic its N_td B samples.
  const int con_rows = crr ? B * (1 + npw) : mpo ? B : 2 * B;
  const int ctg_rows = crr ? B * ntd : mpo ? B * mpo->num_samples : B;
  int rc;
  int hmax = 0;
  for (int i = 0; i < cfg->num_policy_layers; ++i) hmax = std::max(hmax, cfg->policy_sizes[i]);
  for (int i = 0; i < cfg->num_critic_layers; ++i) hmax = std::max(hmax, cfg->critic_sizes[i]);
  if ((rc = alloc_acts(l, l->pon, l->pol, B, true)) || (rc = alloc_acts(l, l->ptg, l->pol, B, true)) ||
      (rc = alloc_acts(l, l->con, l->cri, con_rows, false)) ||
      (rc = alloc_acts(l, l->ctg, l->cri, ctg_rows, false)))
    return rc;
  if (mpo) {
    const int64_t A = cfg->act_dim, NB = ctg_rows;
    auto& mb = l->mb;
    if ((rc = dev_alloc(l, &mb.sd_on, B * A)) || (rc = dev_alloc(l, &mb.sd_t, B * A)) ||
        (rc = dev_alloc(l, &mb.noise, NB * A)) || (rc = dev_alloc(l, &mb.act, NB * A)) ||
        (rc = dev_alloc(l, &mb.cost, NB)) || (rc = dev_alloc(l, &mb.tiled, NB * cfg->obs_dim)) ||
        (rc = dev_alloc(l, &mb.w, NB)) || (rc = dev_alloc(l, &mb.pw, NB)) ||
        (rc = dev_alloc(l, &mb.qt, B)) || (rc = dev_alloc(l, &mb.dmean, B * A)) ||
        (rc = dev_alloc(l, &mb.dpre, B * A)) ||
        (rc = dev_alloc(l, &mb.part, ceil_div(B, 4) * kMpoCols)) ||
        (rc = dev_alloc(l, &mb.stats, ACME_MPO_NUM_STATS)) || (rc = dev_alloc(l, &mb.klm_rel, A)) ||
        (rc = dev_alloc(l, &mb.kls_rel, A)) || (rc = dev_alloc(l, &mb.ploss, 1)))
      return rc;
    if (hipMemset(mb.pw, 0, (size_t)NB * sizeof(float)) != hipSuccess)
      return (set_error("hipMemset failed"), ACME_ERR_HIP);
    // MPO's scalar head writes the sampled values where DMPO's head writes the N B x K logits
    // (ctg.out, sized by alloc_acts); DMPO keeps the values, and the mixtures, beside them.
    mb.sq = l->ctg.out;
    if (head == Head::kMpoCategorical &&
        ((rc = dev_alloc(l, &mb.sq, NB)) ||
         (rc = dev_alloc(l, &l->mixture, (int64_t)B * cfg->num_atoms))))
      return rc;
  }
  if (crr) {
    const int64_t A = cfg->act_dim, NR = (int64_t)B * (ntd + npw);
    auto& mb = l->mb;
    auto& cb = l->cb;
    if ((rc = dev_alloc(l, &mb.sd_on, B * A)) || (rc = dev_alloc(l, &mb.sd_t, B * A)) ||
        (rc = dev_alloc(l, &mb.noise, NR * A)) || (rc = dev_alloc(l, &mb.act, NR * A)) ||
        (rc = dev_alloc(l, &mb.tiled, NR * cfg->obs_dim)) ||
        (rc = dev_alloc(l, &mb.dmean, B * A)) || (rc = dev_alloc(l, &mb.dpre, B * A)) ||
        (rc = dev_alloc(l, &mb.sq, (int64_t)B * ntd)) ||
        (rc = dev_alloc(l, &l->mixture, (int64_t)B * cfg->num_atoms)) ||
        (rc = dev_alloc(l, &cb.q_mean, B)) || (rc = dev_alloc(l, &cb.v_est, B)) ||
        (rc = dev_alloc(l, &cb.adv, B)) || (rc = dev_alloc(l, &cb.coef, B)) ||
        (rc = dev_alloc(l, &cb.logp, B)) || (rc = dev_alloc(l, &cb.coef_part, ceil_div(B, 4))))
      return rc;
  }
  for (int i = 0; i < l->cri.nl; ++i)
    if ((rc = dev_alloc(l, &l->cdz[i], (int64_t)2 * B * l->cri.sizes[i]))) return rc;
  for (int i = 0; i < l->pol.nl; ++i)
    if ((rc = dev_alloc(l, &l->pdz[i], (int64_t)B * l->pol.sizes[i]))) return rc;
  const int64_t nblk = ceil_div(2 * B, kRows);
  if ((rc = dev_alloc(l, &l->dlogits, (int64_t)2 * B * cfg->num_atoms)) ||
      (rc = dev_alloc(l, &l->du, (int64_t)B * cfg->act_dim)) ||
      (rc = dev_alloc(l, &l->dqda, (int64_t)B * cfg->act_dim)) ||
      (rc = dev_alloc(l, &l->values, cfg->num_atoms)) ||
      (rc = dev_alloc(l, &l->act_lo, cfg->act_dim)) ||
      (rc = dev_alloc(l, &l->act_scale, cfg->act_dim)) ||
      (rc = dev_alloc(l, &l->lnslab, nblk * 2 * hmax)) ||
      (rc = dev_alloc(l, &l->lnslab2, nblk * 2 * hmax)) ||
      (rc = dev_alloc(l, &l->ploss_part, nblk)) ||
      (rc = dev_alloc(l, &l->norm_part, 2 * kNormBlocks)) ||
      (rc = dev_alloc(l, &l->norms, 2)) || (rc = dev_alloc(l, &l->loss_tmp, 3)) ||
      (rc = dev_alloc(l, &l->ce, B)) || (rc = dev_alloc(l, &l->dev_step, 1)))
    return rc;
  if (!is_categorical(head) &&
      ((rc = dev_alloc(l, &l->td, B)) || (rc = dev_alloc(l, &l->dq, 2 * B))))
    return rc;
  // Support: tf.linspace(vmin, vmax, K) (computed in f64, rounded once to f32).
  std::vector<float> vals(cfg->num_atoms), lo(cfg->act_dim), sc(cfg->act_dim);
  const double step = ((double)cfg->vmax - (double)cfg->vmin) / std::max(cfg->num_atoms - 1, 1);
  for (int i = 0; i < cfg->num_atoms; ++i) vals[i] = (float)((double)cfg->vmin + i * step);
  for (int j = 0; j < cfg->act_dim; ++j) {
    lo[j] = cfg->action_min[j];
    sc[j] = cfg->action_max[j] - cfg->action_min[j];
  }
  if (hipMemset(l->dev_step, 0, sizeof(int64_t)) != hipSuccess ||
      hipMemcpy(l->values, vals.data(), vals.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(l->act_lo, lo.data(), lo.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(l->act_scale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return (set_error("hipMemcpy of the D4PG constants failed"), ACME_ERR_HIP);
  return ACME_OK;
}

// A learner of handle type L (acme_d4pg, acme_ddpg, acme_mpo, acme_dmpo, acme_crr) with the
// given head kind.
template <class L>
int create_learner(const acme_d4pg_config* cfg, Head head, const acme_mpo_config* mpo, L** out,
                   const acme_crr_config* crr = nullptr) {
  int rc = check_config(cfg, head);
  if (rc != ACME_OK) return rc;
  L* l = new L();
  if ((rc = init_learner(l, cfg, head, mpo, crr)) != ACME_OK) return (ac_destroy(l), rc);
  *out = l;
  return ACME_OK;
}

// The learner configuration of a DDPG or MPO config (the shared fields carry the same
// names): a critic that ends in one scalar, no support.
template <class C>
acme_d4pg_config scalar_head_config(const C* cfg, int target_update_period) {
  acme_d4pg_config c;
  memset(&c, 0, sizeof(c));
  c.obs_dim = cfg->obs_dim; c.act_dim = cfg->act_dim; c.max_batch = cfg->max_batch;
  c.num_policy_layers = cfg->num_policy_layers;
  c.num_critic_layers = cfg->num_critic_layers;
  memcpy(c.policy_sizes, cfg->policy_sizes, sizeof(c.policy_sizes));
  memcpy(c.critic_sizes, cfg->critic_sizes, sizeof(c.critic_sizes));
  c.num_atoms = 1; c.vmin = 0.f; c.vmax = 0.f;
  memcpy(c.action_min, cfg->action_min, sizeof(c.action_min));
  memcpy(c.action_max, cfg->action_max, sizeof(c.action_max));
  c.discount = cfg->discount; c.target_update_period = target_update_period;
  c.policy_learning_rate = cfg->policy_learning_rate;
  c.critic_learning_rate = cfg->critic_learning_rate;
  c.adam_beta1 = cfg->adam_beta1; c.adam_beta2 = cfg->adam_beta2;
  c.adam_epsilon = cfg->adam_epsilon; c.clipping = cfg->clipping;
  c.layer_norm_epsilon = cfg->layer_norm_epsilon;
  return c;
}

int64_t ac_flat_size(const acme_actor_critic* l) { return l ? l->flat : 0; }
int64_t ac_policy_size(const acme_actor_critic* l) { return l ? l->policy_flat : 0; }
int32_t ac_num_tensors(const acme_actor_critic* l) { return l ? (int32_t)l->tensors.size() : 0; }

int ac_bind(acme_actor_critic* l, float* params, float* target, float* grads, float* adam_m,
            float* adam_v) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(params && target && grads && adam_m && adam_v, "null buffer");
  for (const void* p : {(const void*)params, (const void*)target, (const void*)grads,
                        (const void*)adam_m, (const void*)adam_v})
    ACME_CHECK_ARG(((uintptr_t)p & 15) == 0, "buffers must be 16-byte aligned");
  // Captured graphs bake in the bound buffers: a re-bind invalidates them.
  if (!l->graphs.empty()) {
    ACME_HIP_TRY(hipDeviceSynchronize());
    for (auto& g : l->graphs) (void)hipGraphExecDestroy(g.exec);
    l->graphs.clear();
  }
  l->params = params;
  l->target = target;
  l->grads = grads;
  l->m = adam_m;
  l->v = adam_v;
  return ACME_OK;
}

int64_t ac_num_steps(const acme_actor_critic* l) { return l ? l->num_steps : 0; }
int ac_set_num_steps(acme_actor_critic* l, int64_t n) {
  ACME_CHECK_ARG(l && n >= 0, "bad argument");
  ACME_HIP_TRY(hipDeviceSynchronize());
  ACME_HIP_TRY(hipMemcpy(l->dev_step, &n, sizeof(n), hipMemcpyHostToDevice));
  l->num_steps = n;
  return ACME_OK;
}

// acme_d4pg_step and acme_ddpg_step (the batch and output types are the same).
int d4pg_step(acme_actor_critic* l, const acme_d4pg_batch* batch, const acme_d4pg_outputs* out,
              void* stream) {
  ACME_CHECK_ARG(l && batch, "null argument");
  ACME_CHECK_ARG(l->head != Head::kMpo, "an MPO learner steps through acme_mpo_step");
  ACME_CHECK_ARG(l->head != Head::kMpoCategorical, "a DMPO learner steps through acme_dmpo_step");
  ACME_CHECK_ARG(l->head != Head::kCrr, "a CRR learner steps through acme_crr_step");
  const bool copy = l->num_steps % l->cfg.target_update_period == 0;
  const void* key[kGraphKeys] = {batch->o_tm1, batch->a_tm1, batch->r_t, batch->d_t,
                                 batch->o_t, out ? out->critic_loss : nullptr,
                                 out ? out->policy_loss : nullptr};
  return run_step(l, "acme_d4pg", batch, key, copy ? 1 : 0, stream,
                  [&](hipStream_t s) { return d4pg_step_impl(l, batch, out, copy, s); });
}

// acme_d4pg_policy and acme_ddpg_policy.
int d4pg_policy(acme_actor_critic* l, const float* obs, int64_t rows, int32_t use_target,
                float* actions, void* stream) {
  ACME_CHECK_ARG(l && obs && actions, "null argument");
  ACME_CHECK_ARG(l->params, "acme_d4pg_bind must be called first");
  ACME_CHECK_ARG(rows >= 0, "negative row count");
  hipStream_t st = as_stream(stream);
  const int B = l->cfg.max_batch;
  for (int64_t r0 = 0; r0 < rows; r0 += B) {
    const int n = (int)std::min<int64_t>(B, rows - r0);
    const float* o = obs + r0 * l->cfg.obs_dim;
    const NetIn in[2] = {{use_target ? l->target : l->params, o, nullptr, o, nullptr, n, n,
                          &l->ptg},
                         {l->params, o, nullptr, o, nullptr, n, 0, &l->ptg}};
    float* const out[2] = {actions + r0 * l->cfg.act_dim, nullptr};
    int rc = policy_forward_pair(l, in, out, st);
    if (rc != ACME_OK) return rc;
  }
  return ACME_OK;
}

// The workspace buffers each head kind shows to tests and diagnostics.
int ac_debug_buffer(const acme_actor_critic* l, const char* name, const float** out,
                    int64_t* count) {
  ACME_CHECK_ARG(l && name && out && count, "null argument");
  const int64_t B = l->cfg.max_batch, A = l->cfg.act_dim, K = l->cfg.num_atoms;
  if (l->head == Head::kCategorical) {
    const DebugItem items[] = {
        {"p_a", l->pon.out, B * A},          {"t_a", l->ptg.out, B * A},
        {"c_logits", l->con.out, 2 * B * K}, {"t_logits", l->ctg.out, B * K},
        {"dlogits", l->dlogits, 2 * B * K},  {"dqda", l->dqda, B * A},
        {"du", l->du, B * A},                {"norms", l->norms, 2},
        {"losses", l->loss_tmp, 2},
    };
    return find_debug_buffer(items, name, out, count);
  }
  if (l->head == Head::kScalar) {
    const DebugItem items[] = {
        {"p_a", l->pon.out, B * A}, {"t_a", l->ptg.out, B * A},
        {"c_q", l->con.out, 2 * B}, {"t_q", l->ctg.out, B},
        {"td", l->td, B},           {"dq", l->dq, 2 * B},
        {"dqda", l->dqda, B * A},   {"du", l->du, B * A},
        {"norms", l->norms, 2},     {"losses", l->loss_tmp, 2},
    };
    return find_debug_buffer(items, name, out, count);
  }
  const auto& mb = l->mb;
  if (l->head == Head::kCrr) {
    // The step packs the R rows of the last batch densely: the online samples follow R rows.
    const int64_t R = l->crr_rows;
    const int64_t Ntd = l->ccfg.num_action_samples_td_learning;
    const int64_t Npw = l->ccfg.num_action_samples_policy_weight;
    const auto& cb = l->cb;
    const DebugItem items[] = {
        {"mean_on", l->pon.out, R * A}, {"std_on", mb.sd_on, R * A}, {"pre_on", l->pon.t, R * A},
        {"mean_t", l->ptg.out, R * A},  {"std_t", mb.sd_t, R * A},
        {"noise", mb.noise, (Ntd + Npw) * R * A}, {"actions", mb.act, (Ntd + Npw) * R * A},
        {"logits_tm1", l->con.out, R * K}, {"sampled_logits", l->ctg.out, Ntd * R * K},
        {"policy_sampled_logits", l->con.out + R * K, Npw * R * K},
        {"sampled_q", mb.sq, Ntd * R},  {"mixture", l->mixture, R * K},
        {"ce", l->ce, R},               {"dlogits", l->dlogits, R * K},
        {"q_tm1_mean", cb.q_mean, R},   {"v_estimate", cb.v_est, R},
        {"advantage", cb.adv, R},       {"coef", cb.coef, R},        {"logp", cb.logp, R},
        {"dmean", mb.dmean, R * A},     {"dpre", mb.dpre, R * A},
        {"norms", l->norms, 2},         {"losses", l->loss_tmp, 3},
    };
    return find_debug_buffer(items, name, out, count);
  }
  const int64_t NB = B * l->mcfg.num_samples;
  if (l->head == Head::kMpoCategorical) {
    for (const char* scalar_only : {"q_tm1", "q_t", "td", "dq"})
      if (strcmp(name, scalar_only) == 0) {
        set_error("debug buffer '%s' is the scalar critic's: a DMPO learner has logits_tm1, "
                  "sampled_logits, mixture, dlogits and ce", name);
        return ACME_ERR_INVALID;
      }
    const DebugItem items[] = {
        {"mean_on", l->pon.out, B * A}, {"std_on", mb.sd_on, B * A}, {"pre_on", l->pon.t, B * A},
        {"mean_t", l->ptg.out, B * A},  {"std_t", mb.sd_t, B * A},   {"noise", mb.noise, NB * A},
        {"actions", mb.act, NB * A},    {"cost", mb.cost, NB},       {"sampled_q", mb.sq, NB},
        {"weights", mb.w, NB},          {"penalty_weights", mb.pw, NB},
        {"logits_tm1", l->con.out, B * K}, {"sampled_logits", l->ctg.out, NB * K},
        {"mixture", l->mixture, B * K}, {"dlogits", l->dlogits, B * K}, {"ce", l->ce, B},
        {"dmean", mb.dmean, B * A},     {"dpre", mb.dpre, B * A},
        {"norms", l->norms, 2},         {"losses", l->loss_tmp, 2},
        {"stats", mb.stats, ACME_MPO_NUM_STATS},
        {"kl_mean_rel", mb.klm_rel, A}, {"kl_stddev_rel", mb.kls_rel, A},
    };
    return find_debug_buffer(items, name, out, count);
  }
  const DebugItem items[] = {
      {"mean_on", l->pon.out, B * A}, {"std_on", mb.sd_on, B * A}, {"pre_on", l->pon.t, B * A},
      {"mean_t", l->ptg.out, B * A},  {"std_t", mb.sd_t, B * A},   {"noise", mb.noise, NB * A},
      {"actions", mb.act, NB * A},    {"cost", mb.cost, NB},       {"sampled_q", l->ctg.out, NB},
      {"weights", mb.w, NB},          {"penalty_weights", mb.pw, NB},
      {"q_tm1", l->con.out, B},       {"q_t", mb.qt, B},           {"td", l->td, B},
      {"dq", l->dq, B},               {"dmean", mb.dmean, B * A},  {"dpre", mb.dpre, B * A},
      {"norms", l->norms, 2},         {"losses", l->loss_tmp, 2},
      {"stats", mb.stats, ACME_MPO_NUM_STATS},
      {"kl_mean_rel", mb.klm_rel, A}, {"kl_stddev_rel", mb.kls_rel, A},
  };
  return find_debug_buffer(items, name, out, count);
}

// The bodies behind the acme_mpo_* and acme_dmpo_* exports that only those two kinds have.

// What acme_mpo_create checks of the fields that MPO adds to the shared configuration.
int check_mpo_config(const acme_mpo_config* cfg) {
  ACME_CHECK_ARG(cfg->num_samples >= 1 && cfg->num_samples <= ACME_MPO_MAX_SAMPLES,
                 "num_samples must be in [1, %d]", ACME_MPO_MAX_SAMPLES);
  // The target critic runs max_batch * num_samples rows through the GEMM engine and the
  // LayerNorm row kernels, which take what D4PG's 2 * 65536 rows ask of them.
  ACME_CHECK_ARG(cfg->max_batch >= 1 &&
                     (int64_t)cfg->max_batch * cfg->num_samples <= ACME_MPO_MAX_ROWS,
                 "max_batch * num_samples must be in [1, %d]", ACME_MPO_MAX_ROWS);
  ACME_CHECK_ARG(cfg->target_policy_update_period >= 1 && cfg->target_critic_update_period >= 1,
                 "target update periods must be >= 1");
  ACME_CHECK_ARG(cfg->epsilon > 0.f && cfg->epsilon_mean > 0.f && cfg->epsilon_stddev > 0.f &&
                     cfg->epsilon_penalty > 0.f,
                 "the KL bounds (epsilon*) must be positive");
  ACME_CHECK_ARG(cfg->init_scale > 0.f && cfg->min_scale >= 0.f,
                 "init_scale must be positive and min_scale non-negative");
  return ACME_OK;
}

int mpo_init_duals(acme_actor_critic* l) {
  ACME_CHECK_ARG(l && has_duals(l->head), "not an MPO or DMPO learner");
  ACME_CHECK_ARG(l->params, "acme_mpo_bind must be called first");
  ACME_HIP_TRY(hipDeviceSynchronize());
  const acme_mpo_config& mc = l->mcfg;
  const std::pair<int, float> init[] = {{l->t_temp, mc.init_log_temperature},
                                        {l->t_amean, mc.init_log_alpha_mean},
                                        {l->t_astd, mc.init_log_alpha_stddev},
                                        {l->t_ptemp, mc.init_log_temperature}};
  for (const auto& it : init) {
    if (it.first < 0) continue;
    const Tensor& t = l->tensors[it.first];
    const std::vector<float> v((size_t)t.numel, it.second);
    ACME_HIP_TRY(hipMemcpy(l->params + t.offset, v.data(), v.size() * sizeof(float),
                           hipMemcpyHostToDevice));
  }
  return ACME_OK;
}

// acme_mpo_step (head = Head::kMpo) and acme_dmpo_step (Head::kMpoCategorical): a handle of
// the other kind is refused with the name of its own entry.
int mpo_step(acme_actor_critic* l, Head head, const acme_mpo_batch* batch,
             const acme_mpo_outputs* out, void* stream) {
  ACME_CHECK_ARG(l && batch, "null argument");
  if (l->head != head) {
    set_error(l->head == Head::kMpo               ? "an MPO learner steps through acme_mpo_step"
              : l->head == Head::kMpoCategorical ? "a DMPO learner steps through acme_dmpo_step"
              : l->head == Head::kCrr            ? "a CRR learner steps through acme_crr_step"
              : head == Head::kMpo                ? "not an MPO learner"
                                                  : "not a DMPO learner");
    return ACME_ERR_INVALID;
  }
  const int copy = (l->num_steps % l->mcfg.target_policy_update_period == 0 ? 1 : 0) |
                   (l->num_steps % l->mcfg.target_critic_update_period == 0 ? 2 : 0);
  const void* key[kGraphKeys] = {batch->o_tm1, batch->a_tm1, batch->r_t, batch->d_t,
                                 batch->o_t, batch->noise,
                                 out ? out->critic_loss : nullptr,
                                 out ? out->policy_loss : nullptr,
                                 out ? out->stats : nullptr,
                                 out ? out->kl_mean_rel : nullptr,
                                 out ? out->kl_stddev_rel : nullptr};
  if (head == Head::kMpo)
    return run_step(l, "acme_mpo", batch, key, copy, stream,
                    [&](hipStream_t s) { return mpo_step_impl(l, batch, out, copy, s); });
  return run_step(l, "acme_dmpo", batch, key, copy, stream,
                  [&](hipStream_t s) { return dmpo_step_impl(l, batch, out, copy, s); });
}

int mpo_policy(acme_actor_critic* l, const float* obs, int64_t rows, int32_t use_target,
               float* mean_out, float* stddev_out, void* stream) {
  ACME_CHECK_ARG(l && obs && mean_out && stddev_out, "null argument");
  ACME_CHECK_ARG(has_gauss_head(l->head), "not a learner with a Gaussian policy head");
  ACME_CHECK_ARG(l->params, "acme_mpo_bind must be called first");
  ACME_CHECK_ARG(rows >= 0, "negative row count");
  hipStream_t st = as_stream(stream);
  const int B = l->cfg.max_batch, A = l->cfg.act_dim;
  const NetDesc& pd = l->pol;
  const float* prm = use_target ? l->target : l->params;
  for (int64_t r0 = 0; r0 < rows; r0 += B) {
    const int n = (int)std::min<int64_t>(B, rows - r0);
    const float* o = obs + r0 * l->cfg.obs_dim;
    const NetIn in[2] = {{prm, o, nullptr, o, nullptr, n, n, &l->ptg},
                         {l->params, o, nullptr, o, nullptr, n, 0, &l->ptg}};
    int rc = lnmlp_forward_pair(l, pd, in, l->cfg.obs_dim, 0, "mpo_policy_ln", st);
    if (rc != ACME_OK) return rc;
    GaussHeadPair g;
    set_gauss_head(l, g, 0, prm, l->ptg.h[pd.nl - 1], n, mean_out + r0 * A, nullptr,
                   stddev_out + r0 * A);
    g.a[1] = g.a[0];
    gauss_head_kernel<<<dim3((unsigned)ceil_div(n, 4), 1), 256, 0, st>>>(g);
    ACME_LAUNCH_CHECK();
  }
  return ACME_OK;
}

// The bodies behind the acme_crr_* exports that only that kind has.

// What acme_crr_create checks of the fields that CRR adds to the shared configuration.
int check_crr_config(const acme_crr_config* cfg) {
  const int ntd = cfg->num_action_samples_td_learning;
  const int npw = cfg->num_action_samples_policy_weight;
  ACME_CHECK_ARG(ntd >= 1 && ntd <= ACME_MPO_MAX_SAMPLES,
                 "num_action_samples_td_learning must be in [1, %d]", ACME_MPO_MAX_SAMPLES);
  ACME_CHECK_ARG(npw >= 1 && npw <= ACME_MPO_MAX_SAMPLES,
                 "num_action_samples_policy_weight must be in [1, %d]", ACME_MPO_MAX_SAMPLES);
  // The online critic runs max_batch * (1 + N_pw) rows, the target critic max_batch * N_td.
  ACME_CHECK_ARG(cfg->max_batch >= 1 &&
                     (int64_t)cfg->max_batch * (1 + std::max(ntd, npw)) <= ACME_MPO_MAX_ROWS,
                 "max_batch * (1 + max(num_action_samples_td_learning, "
                 "num_action_samples_policy_weight)) must be in [1, %d]", ACME_MPO_MAX_ROWS);
  ACME_CHECK_ARG(cfg->baseline_reduce_function >= ACME_CRR_REDUCE_MEAN &&
                     cfg->baseline_reduce_function <= ACME_CRR_REDUCE_MIN,
                 "baseline_reduce_function must be mean (0), max (1) or min (2)");
  ACME_CHECK_ARG(cfg->policy_improvement_modes >= ACME_CRR_MODE_EXP &&
                     cfg->policy_improvement_modes <= ACME_CRR_MODE_ALL,
                 "policy_improvement_modes must be exp (0), binary (1) or all (2)");
  ACME_CHECK_ARG(cfg->beta > 0.f && cfg->ratio_upper_bound > 0.f,
                 "beta and ratio_upper_bound must be positive");
  ACME_CHECK_ARG(cfg->sequence_length >= 2, "sequence_length must be >= 2");
  ACME_CHECK_ARG(cfg->init_scale > 0.f && cfg->min_scale >= 0.f,
                 "init_scale must be positive and min_scale non-negative");
  return ACME_OK;
}

// The learner configuration of a CRR config: the categorical critic, the action range unused.
acme_d4pg_config crr_core_config(const acme_crr_config* cfg) {
  acme_d4pg_config c;
  memset(&c, 0, sizeof(c));
  c.obs_dim = cfg->obs_dim; c.act_dim = cfg->act_dim; c.max_batch = cfg->max_batch;
  c.num_policy_layers = cfg->num_policy_layers;
  c.num_critic_layers = cfg->num_critic_layers;
  memcpy(c.policy_sizes, cfg->policy_sizes, sizeof(c.policy_sizes));
  memcpy(c.critic_sizes, cfg->critic_sizes, sizeof(c.critic_sizes));
  c.num_atoms = cfg->num_atoms; c.vmin = cfg->vmin; c.vmax = cfg->vmax;
  for (int j = 0; j < ACME_D4PG_MAX_ACT; ++j) {
    c.action_min[j] = -1.f;
    c.action_max[j] = 1.f;
  }
  c.discount = cfg->discount; c.target_update_period = cfg->target_update_period;
  c.policy_learning_rate = cfg->policy_learning_rate;
  c.critic_learning_rate = cfg->critic_learning_rate;
  c.adam_beta1 = cfg->adam_beta1; c.adam_beta2 = cfg->adam_beta2;
  c.adam_epsilon = cfg->adam_epsilon; c.clipping = cfg->clipping;
  c.layer_norm_epsilon = cfg->layer_norm_epsilon;
  return c;
}

int crr_step(acme_actor_critic* l, const acme_crr_batch* batch, const acme_crr_outputs* out,
             void* stream) {
  ACME_CHECK_ARG(l && batch, "null argument");
  if (l->head != Head::kCrr) {
    set_error(l->head == Head::kMpo               ? "an MPO learner steps through acme_mpo_step"
              : l->head == Head::kMpoCategorical ? "a DMPO learner steps through acme_dmpo_step"
                                                 : "not a CRR learner");
    return ACME_ERR_INVALID;
  }
  const int T = l->ccfg.sequence_length;
  ACME_CHECK_ARG(batch->batch % (T - 1) == 0,
                 "batch %lld is not a multiple of sequence_length - 1 = %d",
                 (long long)batch->batch, T - 1);
  // The copy follows the update; the flag keys the graph as the other kinds' does.
  const bool copy = l->num_steps % l->cfg.target_update_period == 0;
  const void* key[kGraphKeys] = {batch->o_tm1, batch->a_tm1, batch->r_t, batch->d_t,
                                 batch->o_t, batch->noise,
                                 out ? out->critic_loss : nullptr,
                                 out ? out->policy_loss : nullptr,
                                 out ? out->policy_loss_coef : nullptr};
  const int rc = run_step(l, "acme_crr", batch, key, copy ? 1 : 0, stream,
                          [&](hipStream_t s) { return crr_step_impl(l, batch, out, copy, s); });
  if (rc == ACME_OK) l->crr_rows = batch->batch;
  return rc;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ D4PG

int acme_d4pg_create(const acme_d4pg_config* cfg, acme_d4pg** out) {
  ACME_CHECK_ARG(cfg && out, "null argument");
  return create_learner(cfg, Head::kCategorical, nullptr, out);
}
int acme_d4pg_destroy(acme_d4pg* l) { return ac_destroy(l); }
int64_t acme_d4pg_flat_size(const acme_d4pg* l) { return ac_flat_size(l); }
int64_t acme_d4pg_policy_size(const acme_d4pg* l) { return ac_policy_size(l); }
int32_t acme_d4pg_num_tensors(const acme_d4pg* l) { return ac_num_tensors(l); }
int acme_d4pg_tensor_info(const acme_d4pg* l, int32_t i, int64_t* offset, int64_t* numel,
                          int32_t* ndim, int64_t* shape4, const char** name) {
  return tensor_info<acme_actor_critic>(l, i, offset, numel, ndim, shape4, name);
}
int acme_d4pg_bind(acme_d4pg* l, float* params, float* target, float* grads, float* adam_m,
                   float* adam_v) {
  return ac_bind(l, params, target, grads, adam_m, adam_v);
}
int acme_d4pg_step(acme_d4pg* l, const acme_d4pg_batch* batch, const acme_d4pg_outputs* out,
                   void* stream) {
  return d4pg_step(l, batch, out, stream);
}
int acme_d4pg_policy(acme_d4pg* l, const float* obs, int64_t rows, int32_t use_target,
                     float* actions, void* stream) {
  return d4pg_policy(l, obs, rows, use_target, actions, stream);
}
int64_t acme_d4pg_num_steps(const acme_d4pg* l) { return ac_num_steps(l); }
int acme_d4pg_set_num_steps(acme_d4pg* l, int64_t n) { return ac_set_num_steps(l, n); }
int acme_d4pg_debug_buffer(const acme_d4pg* l, const char* name, const float** out,
                           int64_t* count) {
  return ac_debug_buffer(l, name, out, count);
}

// ------------------------------------------------------------------ DDPG
// The shared learner with the scalar head (DDPGLearner._step,
// acme/agents/tf/ddpg/learning.py:143-237).

int acme_ddpg_create(const acme_ddpg_config* cfg, acme_ddpg** out) {
  ACME_CHECK_ARG(cfg && out, "null argument");
  const acme_d4pg_config c = scalar_head_config(cfg, cfg->target_update_period);
  return create_learner(&c, Head::kScalar, nullptr, out);
}
int acme_ddpg_destroy(acme_ddpg* l) { return ac_destroy(l); }
int64_t acme_ddpg_flat_size(const acme_ddpg* l) { return ac_flat_size(l); }
int64_t acme_ddpg_policy_size(const acme_ddpg* l) { return ac_policy_size(l); }
int32_t acme_ddpg_num_tensors(const acme_ddpg* l) { return ac_num_tensors(l); }
int acme_ddpg_tensor_info(const acme_ddpg* l, int32_t i, int64_t* offset, int64_t* numel,
                          int32_t* ndim, int64_t* shape4, const char** name) {
  return tensor_info<acme_actor_critic>(l, i, offset, numel, ndim, shape4, name);
}
int acme_ddpg_bind(acme_ddpg* l, float* params, float* target, float* grads, float* adam_m,
                   float* adam_v) {
  return ac_bind(l, params, target, grads, adam_m, adam_v);
}
int acme_ddpg_step(acme_ddpg* l, const acme_ddpg_batch* batch, const acme_ddpg_outputs* out,
                   void* stream) {
  return d4pg_step(l, batch, out, stream);
}
int acme_ddpg_policy(acme_ddpg* l, const float* obs, int64_t rows, int32_t use_target,
                     float* actions, void* stream) {
  return d4pg_policy(l, obs, rows, use_target, actions, stream);
}
int64_t acme_ddpg_num_steps(const acme_ddpg* l) { return ac_num_steps(l); }
int acme_ddpg_set_num_steps(acme_ddpg* l, int64_t n) { return ac_set_num_steps(l, n); }
int acme_ddpg_debug_buffer(const acme_ddpg* l, const char* name, const float** out,
                           int64_t* count) {
  return ac_debug_buffer(l, name, out, count);
}

// ------------------------------------------------------------------ MPO
// The shared learner with the Gaussian policy head and the MPO loss (MPOLearner._step,
// acme/agents/tf/mpo/learning.py:145-260).

int acme_mpo_create(const acme_mpo_config* cfg, acme_mpo** out) {
  ACME_CHECK_ARG(cfg && out, "null argument");
  const int rc = check_mpo_config(cfg);
  if (rc != ACME_OK) return rc;
  // target_update_period is unused: MPO has its own two.
  const acme_d4pg_config c = scalar_head_config(cfg, 1);
  return create_learner(&c, Head::kMpo, cfg, out);
}
int acme_mpo_destroy(acme_mpo* l) { return ac_destroy(l); }
int64_t acme_mpo_flat_size(const acme_mpo* l) { return ac_flat_size(l); }
int64_t acme_mpo_policy_size(const acme_mpo* l) { return ac_policy_size(l); }
int64_t acme_mpo_dual_offset(const acme_mpo* l) { return l ? l->critic_end : 0; }
int32_t acme_mpo_num_tensors(const acme_mpo* l) { return ac_num_tensors(l); }
int acme_mpo_tensor_info(const acme_mpo* l, int32_t i, int64_t* offset, int64_t* numel,
                         int32_t* ndim, int64_t* shape4, const char** name) {
  return tensor_info<acme_actor_critic>(l, i, offset, numel, ndim, shape4, name);
}
int acme_mpo_bind(acme_mpo* l, float* params, float* target, float* grads, float* adam_m,
                  float* adam_v) {
  return ac_bind(l, params, target, grads, adam_m, adam_v);
}

int acme_mpo_init_duals(acme_mpo* l) { return mpo_init_duals(l); }
int acme_mpo_step(acme_mpo* l, const acme_mpo_batch* batch, const acme_mpo_outputs* out,
                  void* stream) {
  return mpo_step(l, Head::kMpo, batch, out, stream);
}
int acme_mpo_policy(acme_mpo* l, const float* obs, int64_t rows, int32_t use_target,
                    float* mean_out, float* stddev_out, void* stream) {
  return mpo_policy(l, obs, rows, use_target, mean_out, stddev_out, stream);
}
int64_t acme_mpo_num_steps(const acme_mpo* l) { return ac_num_steps(l); }
int acme_mpo_set_num_steps(acme_mpo* l, int64_t n) { return ac_set_num_steps(l, n); }
int acme_mpo_debug_buffer(const acme_mpo* l, const char* name, const float** out,
                          int64_t* count) {
  return ac_debug_buffer(l, name, out, count);
}

// ------------------------------------------------------------------ DMPO
// The shared learner with MPO's policy side and D4PG's categorical critic
// (DistributionalMPOLearner._step, acme/agents/tf/dmpo/learning.py:147-276).

int acme_dmpo_create(const acme_dmpo_config* cfg, acme_dmpo** out) {
  ACME_CHECK_ARG(cfg && out, "null argument");
  const int rc = check_mpo_config(&cfg->mpo);
  if (rc != ACME_OK) return rc;
  acme_d4pg_config c = scalar_head_config(&cfg->mpo, 1);
  c.num_atoms = cfg->num_atoms; c.vmin = cfg->vmin; c.vmax = cfg->vmax;
  return create_learner(&c, Head::kMpoCategorical, &cfg->mpo, out);
}
int acme_dmpo_destroy(acme_dmpo* l) { return ac_destroy(l); }
int64_t acme_dmpo_flat_size(const acme_dmpo* l) { return ac_flat_size(l); }
int64_t acme_dmpo_policy_size(const acme_dmpo* l) { return ac_policy_size(l); }
int64_t acme_dmpo_dual_offset(const acme_dmpo* l) { return l ? l->critic_end : 0; }
int32_t acme_dmpo_num_tensors(const acme_dmpo* l) { return ac_num_tensors(l); }
int acme_dmpo_tensor_info(const acme_dmpo* l, int32_t i, int64_t* offset, int64_t* numel,
                          int32_t* ndim, int64_t* shape4, const char** name) {
  return tensor_info<acme_actor_critic>(l, i, offset, numel, ndim, shape4, name);
}
int acme_dmpo_bind(acme_dmpo* l, float* params, float* target, float* grads, float* adam_m,
                   float* adam_v) {
  return ac_bind(l, params, target, grads, adam_m, adam_v);
}
int acme_dmpo_init_duals(acme_dmpo* l) { return mpo_init_duals(l); }
int acme_dmpo_step(acme_dmpo* l, const acme_mpo_batch* batch, const acme_mpo_outputs* out,
                   void* stream) {
  return mpo_step(l, Head::kMpoCategorical, batch, out, stream);
}
int acme_dmpo_policy(acme_dmpo* l, const float* obs, int64_t rows, int32_t use_target,
                     float* mean_out, float* stddev_out, void* stream) {
  return mpo_policy(l, obs, rows, use_target, mean_out, stddev_out, stream);
}
int64_t acme_dmpo_num_steps(const acme_dmpo* l) { return ac_num_steps(l); }
int acme_dmpo_set_num_steps(acme_dmpo* l, int64_t n) { return ac_set_num_steps(l, n); }
int acme_dmpo_debug_buffer(const acme_dmpo* l, const char* name, const float** out,
                           int64_t* count) {
  return ac_debug_buffer(l, name, out, count);
}

// ------------------------------------------------------------------ CRR
// The shared learner with the Gaussian policy head, DMPO's categorical critic and the
// advantage-weighted behaviour-cloning loss (RCRRLearner._step with stateless networks,
// acme/agents/tf/crr/recurrent_learning.py:197-377).

int acme_crr_create(const acme_crr_config* cfg, acme_crr** out) {
  ACME_CHECK_ARG(cfg && out, "null argument");
  const int rc = check_crr_config(cfg);
  if (rc != ACME_OK) return rc;
  const acme_d4pg_config c = crr_core_config(cfg);
  return create_learner(&c, Head::kCrr, nullptr, out, cfg);
}
int acme_crr_destroy(acme_crr* l) { return ac_destroy(l); }
int64_t acme_crr_flat_size(const acme_crr* l) { return ac_flat_size(l); }
int64_t acme_crr_policy_size(const acme_crr* l) { return ac_policy_size(l); }
int32_t acme_crr_num_tensors(const acme_crr* l) { return ac_num_tensors(l); }
int acme_crr_tensor_info(const acme_crr* l, int32_t i, int64_t* offset, int64_t* numel,
                         int32_t* ndim, int64_t* shape4, const char** name) {
  return tensor_info<acme_actor_critic>(l, i, offset, numel, ndim, shape4, name);
}
int acme_crr_bind(acme_crr* l, float* params, float* target, float* grads, float* adam_m,
                  float* adam_v) {
  return ac_bind(l, params, target, grads, adam_m, adam_v);
}
int acme_crr_step(acme_crr* l, const acme_crr_batch* batch, const acme_crr_outputs* out,
                  void* stream) {
  return crr_step(l, batch, out, stream);
}
int acme_crr_policy(acme_crr* l, const float* obs, int64_t rows, int32_t use_target,
                    float* mean_out, float* stddev_out, void* stream) {
  return mpo_policy(l, obs, rows, use_target, mean_out, stddev_out, stream);
}
int64_t acme_crr_num_steps(const acme_crr* l) { return ac_num_steps(l); }
int acme_crr_set_num_steps(acme_crr* l, int64_t n) { return ac_set_num_steps(l, n); }
int acme_crr_debug_buffer(const acme_crr* l, const char* name, const float** out,
                          int64_t* count) {
  return ac_debug_buffer(l, name, out, count);
}

}  // extern "C"
