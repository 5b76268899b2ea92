// R2D2 on vector observations for MI355X: R2D2Learner._step
// (acme/agents/tf/r2d2/learning.py:112-200) for the network of the reference's own R2D2 test
// (acme/agents/tf/r2d2/agent_test.py:28-45), snt.DeepRNN([Flatten, snt.LSTM(H),
// snt.nets.MLP(hidden + [A])]), behind the C ABI (include/acme_hip.h, acme_r2d2_mlp_*).
// Exact f32 throughout.
//
// One step = three launches on one stream, whatever T and the depth are:
//   r2d2_mlp_unroll_kernel, one workgroup per tile of 16 sequences.  The tile's 16 rows are the
//     M dimension of v_mfma_f32_16x16x4_f32.  The online AND the target network are unrolled
//     together: the step's observation tile is loaded once, each network has its own h, c,
//     gates / layer buffers and q row in LDS (row stride % 64 == 4: the 16 rows x 4 columns of
//     an MFMA row operand fall on all 64 banks; the gates' buffer and the MLP's two ping-pong
//     buffers share their floats, the gates being dead once the cell has run).  Every phase
//     between two barriers does the work of both networks: with 4 waves each wave takes its
//     column tiles of the online and then of the target network; with 8 waves (512 threads)
//     waves 0-3 take the online network and waves 4-7 the target, in lockstep through the same
//     barriers (which, and why).  The burn-in (t < burn_in) runs the LSTM only
//     and stores nothing but the state it ends in.  From t = burn_in on the MLP head runs too
//     and each (t, row) is reduced to q[a_t], the online row's greedy index and the bootstrap
//     term sum_j 1[j = greedy] h^-1(tq_j) in an LDS table; only the online activations the
//     backward needs go to a global workspace that this workgroup alone touches.  Then the
//     loss of the tile's sequences in r2d2_loss_kernel's f32 operation order (r2d2_transforms.h:
//     the same transforms), the priorities, and the backward through time for
//     t = T-1..burn_in: one-hot dq -> the MLP's dz -> dh -> dgates -> (dc, dh_prev), the deltas
//     to the workspace; the gradient into the burn-in's final state is dropped.
//   r2d2_mlp_wgrad_kernel, one workgroup per 16 x 16 tile of a weight tensor: dW = a^T dz over
//     the (T - burn_in) B suffix rows, the four waves taking interleaved groups of four rows and
//     summed in wave order through LDS; W_h's a is h of the step before (h0 at t = 0); a bias
//     (column sums of dz) rides with its tensor's first row of tiles.
//   r2d2_mlp_apply_kernel: the loss summed over the sequences in order, snt.Adam at
//     t = num_steps + 1 (no clipping), then target <- online when the copy is due.
// No float atomic anywhere: every sum has a fixed order, so a step repeats bit for bit, and a
// step at (B, T) below the created maxima computes what a learner created at (B, T) computes.
//
// Weights are the MFMA B operands.  The unroll reads them either through L2 or, when both
// networks' flat buffers fit beside the tile, from copies staged in LDS at the start of the
// launch.  The acting step (one launch) reads each weight once: always through L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "learner_common.h"
#include "profiler.h"

// No packed f32 arithmetic in this file's kernels, and a barrier that inlines into them: see
// mlp_model.hip and DESIGN.md 4.5.
#ifdef __HIP_DEVICE_COMPILE__
#define ACME_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define ACME_NO_PK_F32
#endif
#define ACME_DEV __device__ ACME_NO_PK_F32 __forceinline__
#define ACME_R2D2_TX_ATTR ACME_NO_PK_F32
#include "r2d2_transforms.h"
#include "epsilon_greedy.h"

using namespace acme;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

ACME_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int kTile = 16;  // sequences of a workgroup: the MFMA's M
constexpr int kMaxL = ACME_R2D2_MLP_MAX_HIDDEN;
constexpr int kJobs = kMaxL + 3;              // weight tensors: W_i, W_h, the MLP's L + 1 layers
constexpr int kLdsBytes = 160 * 1024 - 1024;  // dynamic LDS a launch may ask for

// Shapes, and where the tensors start in the flat buffer.  MLP layer j maps hw[j] -> hw[j + 1]
// (hw[0] = H, hw[L + 1] = A), ReLU after every layer but the last.
struct Net {
  int D, L, H, A;
  int hw[kMaxL + 2];
  int wi, wh, bl;
  int w[kMaxL + 1], b[kMaxL + 1];
};

// The tile's LDS map, in floats.  Network 0 is the online one, 1 the target.
struct LdsMap {
  int obs, ldo;       // [16][D] the step's observations, shared by both networks
  int h[2], c[2], ldh;  // [16][H]; network 0's are dh and dc in the backward
  int reg[2];         // the gates [16][4H] (ldg), or the MLP's buffers X0, X1 [16][ldx] each
  int ldg, ldx, xsz;  // xsz = 16 ldx: X1 starts xsz floats after X0
  int q[2], ldq;      // [16][A] the MLP's output; network 0's is dq in the backward
  int tab;            // [3][L][16]: q[a] -> error, greedy index -> d loss / d q[a], bootstrap
  int wts;            // both flat parameter buffers, when staged
};

// What the unroll leaves for its own backward and for the weight-gradient launch, online
// network only.  Row of sequence b at step t: b * T + t.
struct Workspace {
  float* a[kMaxL];       // [R][hw[j + 1]] output of MLP layer j < L (after its ReLU)
  float* dz[kMaxL + 1];  // [R][hw[j + 1]] gradient at layer j's pre-activation (dz[L]: dq)
  float* gates;          // [R][4H] the gates' activations (i, f, g, o); dgates after the backward
  float *h, *c;          // [R][H], steps from burn_in - 1 on
  float *q, *tq;         // [R][A] suffix rows (debug buffers)
  float* g;              // [L][B] time-major d loss / d q[a] (debug buffer)
  double* loss_part;     // [B]: w_b * 0.5 sum_t errors^2
};

// Row stride of a tile buffer of `width` columns.
constexpr int lds_stride(int width) { return ((width + 63) & ~63) + 4; }

// D = A B + C on one wave: A is 16 x 4 (lane holds A[lane % 16][lane / 16]), B is 4 x 16 (lane
// holds B[lane / 16][lane % 16]), the lane's four results are D[4 (lane / 16) + r][lane % 16].
ACME_DEV f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc += X[16][K] W[K][ldw] column nc: X in LDS (columns past K count as zero whatever they
// hold: the buffers are shared), the W row clamped into its tensor.
ACME_DEV f32x4 tile_xw(f32x4 acc, const float* X, int ldx, int K, const float* W, int ldw, int nc,
                       int lm, int lq) {
  const float* xa = X + lm * ldx + lq;
  const float* wc = W + nc;
  const int K4 = (K + 3) & ~3;
  int k0 = 0;
  // Four steps' operands loaded before their MFMAs (the compiler does not unroll a loop around
  // a convergent operation by itself); the accumulation order is that of the plain loop.
  for (; k0 + 16 <= K4; k0 += 16) {
    float x[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 4 * u + lq;
      x[u] = k < K ? xa[k0 + 4 * u] : 0.f;
      w[u] = wc[min(k, K - 1) * ldw];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = mfma16(x[u], w[u], acc);
  }
  for (; k0 < K4; k0 += 4) {
    const int k = k0 + lq;
    acc = mfma16(k < K ? xa[k0] : 0.f, wc[min(k, K - 1) * ldw], acc);
  }
  return acc;
}

// acc += dZ[16][N] W[kc][N]^T: dZ in LDS (columns past N count as zero).
ACME_DEV f32x4 tile_zwt(f32x4 acc, const float* dZ, int ldz, int N, const float* W, int ldw,
                        int kc, int lm, int lq) {
  const float* za = dZ + lm * ldz + lq;
  const float* wr = W + kc * ldw;
  const int N4 = (N + 3) & ~3;
  int n0 = 0;
  for (; n0 + 16 <= N4; n0 += 16) {  // as tile_xw
    float z[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = n0 + 4 * u + lq;
      z[u] = n < N ? za[n0 + 4 * u] : 0.f;
      w[u] = wr[min(n, N - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = mfma16(z[u], w[u], acc);
  }
  for (; n0 < N4; n0 += 4) {
    const int n = n0 + lq;
    acc = mfma16(n < N ? za[n0] : 0.f, wr[min(n, N - 1)], acc);
  }
  return acc;
}

ACME_DEV float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// Where MLP layer j of network `net` reads and writes in LDS.
ACME_DEV float* layer_in(float* lds, const LdsMap& L, int net, int j, int* ld) {
  if (j == 0) {
    *ld = L.ldh;
    return lds + L.h[net];
  }
  *ld = L.ldx;
  return lds + L.reg[net] + ((j - 1) & 1) * L.xsz;
}
ACME_DEV float* layer_out(float* lds, const LdsMap& L, const Net& n, int net, int j, int* ld) {
  if (j == n.L) {
    *ld = L.ldq;
    return lds + L.q[net];
  }
  *ld = L.ldx;
  return lds + L.reg[net] + (j & 1) * L.xsz;
}

// The phases of one network step of a tile, for networks [0, nnets) on NW waves: the waves of
// network `net` are those with wave / 4 == net (NW = 8), or all four, one network after the
// other (NW = 4).  Every phase ends at a barrier of the caller's.  Tile row r is global row
// row0 + r * rs of the workspace; rows >= rows are stored nowhere.

// gates = obs W_i + h W_h + b into the network's gates buffer.
template <int NW>
ACME_DEV void gates_phase(float* lds, const LdsMap& L, const Net& n, const float* const* W,
                          int nnets) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lq = lane >> 4;
  const int N = 4 * n.H;
  for (int net = wave >> 2; net < nnets; net += NW / 4) {
    const float* Wn = W[net];
    float* gL = lds + L.reg[net];
    for (int nt = wave & 3; nt * 16 < N; nt += 4) {
      const int col = nt * 16 + lm, nc = min(col, N - 1);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_xw(acc, lds + L.obs, L.ldo, n.D, Wn + n.wi, N, nc, lm, lq);
      acc = tile_xw(acc, lds + L.h[net], L.ldh, n.H, Wn + n.wh, N, nc, lm, lq);
      if (col < N) {
        const float bn = Wn[n.bl + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) gL[(4 * lq + r) * L.ldg + col] = acc[r] + bn;
      }
    }
  }
}

// The cell of every network: h and c in LDS; keep: the online network's activations, c and h
// go to the workspace (keep_gates: the gates too; the step before the suffix needs h and c only).
template <int NW>
ACME_DEV void cell_phase(float* lds, const LdsMap& L, const Net& n, int nnets, int64_t row0,
                         int64_t rs, int rows, const Workspace* ws, bool keep, bool keep_gates) {
  const int H = n.H;
  for (int i = threadIdx.x; i < nnets * kTile * H; i += NW * 64) {
    const int net = i / (kTile * H), ii = i - net * kTile * H;
    const int r = ii / H, u = ii - r * H;
    const float* z = lds + L.reg[net] + r * L.ldg + u;
    float* cL = lds + L.c[net] + r * L.ldh + u;
    const float ig = sigmoidf(z[0]), fg = sigmoidf(z[H]);
    const float gg = tanhf(z[2 * H]), og = sigmoidf(z[3 * H]);
    const float cn = fg * *cL + ig * gg;
    const float hn = og * tanhf(cn);
    *cL = cn;
    lds[L.h[net] + r * L.ldh + u] = hn;
    if (keep && net == 0 && r < rows) {
      const int64_t row = row0 + r * rs;
      if (keep_gates) {
        float* g = ws->gates + row * 4 * H + u;
        g[0] = ig;
        g[H] = fg;
        g[2 * H] = gg;
        g[3 * H] = og;
      }
      ws->c[row * H + u] = cn;
      ws->h[row * H + u] = hn;
    }
  }
}

// MLP layer j of every network.  ws: the online network's hidden activations go to the
// workspace; qout[net] (optional): where the last layer's rows go in global memory.
template <int NW>
ACME_DEV void layer_phase(float* lds, const LdsMap& L, const Net& n, const float* const* W,
                          int nnets, int j, int64_t row0, int64_t rs, int rows,
                          const Workspace* ws, float* const* qout) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lq = lane >> 4;
  const int K = n.hw[j], N = n.hw[j + 1];
  for (int net = wave >> 2; net < nnets; net += NW / 4) {
    const float* Wn = W[net];
    int ldx, ldy;
    const float* X = layer_in(lds, L, net, j, &ldx);
    float* Y = layer_out(lds, L, n, net, j, &ldy);
    for (int nt = wave & 3; nt * 16 < N; nt += 4) {
      const int col = nt * 16 + lm;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_xw(acc, X, ldx, K, Wn + n.w[j], N, min(col, N - 1), lm, lq);
      if (col < N) {
        const float bn = Wn[n.b[j] + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * lq + r;
          const float z = acc[r] + bn;
          const float y = j < n.L ? (z > 0.f ? z : 0.f) : z;  // none after the last layer
          Y[row * ldy + col] = y;
          if (row < rows) {
            const int64_t o = (row0 + row * rs) * N + col;
            if (j < n.L) {
              if (ws && net == 0) ws->a[j][o] = y;
            } else if (qout && qout[net]) {
              qout[net][o] = y;
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------ launch 1: the unroll
struct UnrollArgs {
  const float* params;
  const float* target;
  int flat;
  Net net;
  LdsMap lds;
  Workspace ws;
  const float* obs;       // [B][T][D]
  const int32_t* action;  // [B][T]
  const float *reward, *discount;
  const float *h0, *c0;   // null: zeros
  int64_t state_stride;
  const double* probs;    // [B]
  int B, T, BI, n_step;
  float gamma, eta, one_minus_eta;
  double beta, n_replay;
  float* errors;  // [T - BI - 1][B]
  double* prio;   // [B]
};

template <bool WL, int NW>
__global__ void ACME_NO_PK_F32 __launch_bounds__(NW * 64) r2d2_mlp_unroll_kernel(const UnrollArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ double wred[NW];
  constexpr int NT = NW * 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lq = lane >> 4;
  const Net& n = a.net;
  const LdsMap& L = a.lds;
  const Workspace& ws = a.ws;
  const int D = n.D, H = n.H, A = n.A, T = a.T, BI = a.BI, B = a.B;
  const int Ls = T - BI, Tm = Ls - 1;
  const int b0 = blockIdx.x * kTile, rows = min(kTile, B - b0);
  const int64_t row0 = (int64_t)b0 * T;
  if (WL)
    for (int i = t; i < a.flat; i += NT) {
      lds[L.wts + i] = a.params[i];
      lds[L.wts + a.flat + i] = a.target[i];
    }
  const float* W[2] = {WL ? lds + L.wts : a.params, WL ? lds + L.wts + a.flat : a.target};
  // The core state of both networks (zeros without a stored state, and for the dead rows).
  for (int i = t; i < 2 * kTile * H; i += NT) {
    const int net = i / (kTile * H), ii = i - net * kTile * H;
    const int r = ii / H, u = ii - r * H;
    const bool on = r < rows && a.h0;
    lds[L.h[net] + r * L.ldh + u] = on ? a.h0[(b0 + r) * a.state_stride + u] : 0.f;
    lds[L.c[net] + r * L.ldh + u] = on ? a.c0[(b0 + r) * a.state_stride + u] : 0.f;
  }
  auto load_obs = [&](int s) {
    float* x0 = lds + L.obs;
    for (int i = t; i < kTile * D; i += NT) {
      const int r = i / D, k = i - r * D;
      x0[r * L.ldo + k] = r < rows ? a.obs[(row0 + (int64_t)r * T + s) * D + k] : 0.f;
    }
  };
  load_obs(0);
  {  // The importance weights' maximum over the batch: it depends on the probabilities alone.
    double wmx = 0.0;
    for (int i = t; i < B; i += NT) wmx = fmax(wmx, pow(1.0 / (a.n_replay * a.probs[i]), a.beta));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wmx = fmax(wmx, __shfl_xor(wmx, o, 64));
    if (lane == 0) wred[wave] = wmx;
  }
  block_sync();

  // ---- forward.  The table: tq[s][r] = q[a], tg[s][r] = the greedy index, tb[s][r] = the
  // bootstrap term of suffix step s.
  float* tq = lds + L.tab;
  float* tg = tq + kTile * Ls;
  float* tb = tg + kTile * Ls;
  float* qout[2] = {ws.q, ws.tq};
  for (int s = 0; s < T; ++s) {
    gates_phase<NW>(lds, L, n, W, 2);
    block_sync();
    cell_phase<NW>(lds, L, n, 2, row0 + s, T, rows, &ws, s >= BI - 1, s >= BI);
    if (s + 1 < T) load_obs(s + 1);  // the gates have read this step's
    block_sync();
    if (s < BI) continue;
    for (int j = 0; j <= n.L; ++j) {
      layer_phase<NW>(lds, L, n, W, 2, j, row0 + s, T, rows, &ws, qout);
      block_sync();
    }
    // One lane per row; the q rows are next written three barriers from here.
    if (t < kTile) {
#pragma clang fp contract(off)
      const float* qr = lds + L.q[0] + t * L.ldq;
      const float* tr = lds + L.q[1] + t * L.ldq;
      int best = 0;  // tf.argmax: the first maximum
      float bq = qr[0];
      for (int j = 1; j < A; ++j)
        if (qr[j] > bq) {
          bq = qr[j];
          best = j;
        }
      float boot = 0.f;  // summed in action order, as the reference's one-hot product
      for (int j = 0; j < A; ++j) boot = boot + (j == best ? 1.f : 0.f) * parabolic(tr[j]);
      int at = 0;
      if (t < rows) at = min(max(a.action[row0 + (int64_t)t * T + s], 0), A - 1);
      const int si = s - BI;
      tq[si * kTile + t] = qr[at];
      tg[si * kTile + t] = __int_as_float(best);
      tb[si * kTile + t] = boot;
    }
  }
  block_sync();

  // ---- the loss of the tile's sequences, r2d2_loss_kernel's operations: 16 lanes per sequence
  // over the Tm loss steps; the error replaces q[a], d loss / d q[a] the greedy index.
  if (t < 256) {
#pragma clang fp contract(off)
    const int r = t >> 4, k = t & 15;
    if (r < rows) {
      const int b = b0 + r;
      double wmx = wred[0];
      for (int i = 1; i < NW; ++i) wmx = fmax(wmx, wred[i]);
      const float w = (float)(pow(1.0 / (a.n_replay * a.probs[b]), a.beta) / wmx);
      const float inv_b = div_rn(1.f, (float)B);
      const int64_t base = (int64_t)b * T + BI;
      for (int s = k; s < Tm; s += 16) {
        // The bootstrap of step min(s + n - 1, Tm - 1) is the term of the suffix step after it.
        float target = tb[(min(s + a.n_step - 1, Tm - 1) + 1) * kTile + r];
        for (int i = a.n_step - 1; i >= 0; --i) {
          const int kk = s + i;
          const float rw = kk < Tm ? a.reward[base + kk] : 0.f;
          const float pc = kk < Tm ? a.discount[base + kk] * a.gamma : 1.f;
          target = rw + pc * target;
        }
        const bool finite = isfinite(target);
        if (!finite) target = 0.f;
        const float err = finite ? tq[s * kTile + r] - hyperbolic(target) : 0.f;
        const float g = (w * err) * inv_b;
        tq[s * kTile + r] = err;
        tg[s * kTile + r] = g;
        a.errors[(int64_t)s * B + b] = err;
        ws.g[(int64_t)s * B + b] = g;
      }
      if (k == 0) {  // the last suffix row carries no loss term
        tg[Tm * kTile + r] = 0.f;
        ws.g[(int64_t)Tm * B + b] = 0.f;
      }
    }
  }
  // dh and dc of the step after the last: zero.
  for (int i = t; i < kTile * H; i += NT) {
    const int r = i / H, u = i - r * H;
    lds[L.h[0] + r * L.ldh + u] = 0.f;
    lds[L.c[0] + r * L.ldh + u] = 0.f;
  }
  block_sync();
  if (t < rows) {
#pragma clang fp contract(off)
    // compute_priority (learning.py:230-236): f32 max and in-order f32 mean of |errors|; the
    // sequence's loss in f64, in time order.
    const int b = b0 + t;
    double wmx = wred[0];
    for (int i = 1; i < NW; ++i) wmx = fmax(wmx, wred[i]);
    const float w = (float)(pow(1.0 / (a.n_replay * a.probs[b]), a.beta) / wmx);
    double sq = 0.0;
    float mx = 0.f, sm = 0.f;
    for (int s = 0; s < Tm; ++s) {
      const float err = tq[s * kTile + t], e = fabsf(err);
      sq += (double)err * (double)err;
      mx = fmaxf(mx, e);
      sm = sm + e;
    }
    const float mean = div_rn(sm, (float)Tm);
    a.prio[b] = (double)(a.eta * mx + a.one_minus_eta * mean);
    ws.loss_part[b] = 0.5 * sq * (double)w;
  }

  // ---- backward through time, the online network on every wave.
  const float* Wo = W[0];
  float* hL = lds + L.h[0];
  float* cL = lds + L.c[0];
  float* gL = lds + L.reg[0];
  float* qL = lds + L.q[0];
  for (int s = T - 1; s >= BI; --s) {
    const int si = s - BI;
    const int64_t r0 = row0 + s;
    for (int i = t; i < kTile * A; i += NT) {
      const int r = i / A, j = i - r * A;
      float v = 0.f;
      if (r < rows) {
        const int at = min(max(a.action[r0 + (int64_t)r * T], 0), A - 1);
        v = j == at ? tg[si * kTile + r] : 0.f;
        ws.dz[n.L][(r0 + (int64_t)r * T) * A + j] = v;
      }
      qL[r * L.ldq + j] = v;
    }
    block_sync();
    // The MLP: the delta at layer j - 1's output = (delta at layer j's output) W_j^T, masked by
    // that layer's ReLU; below layer 0 it is dh, added to the dh from the step after.
    for (int j = n.L; j >= 0; --j) {
      const int K = n.hw[j], N = n.hw[j + 1];
      int ldz, ldx;
      const float* dZ = layer_out(lds, L, n, 0, j, &ldz);
      float* X = layer_in(lds, L, 0, j, &ldx);
      for (int kt = wave; kt * 16 < K; kt += NW) {
        const int k = kt * 16 + lm;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = tile_zwt(acc, dZ, ldz, N, Wo + n.w[j], N, min(k, K - 1), lm, lq);
        if (k < K) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 4 * lq + r;
            if (j == 0) {
              X[row * ldx + k] += acc[r];
            } else {
              const int64_t o = (r0 + (int64_t)row * T) * K + k;
              const float v = row < rows && ws.a[j - 1][o] > 0.f ? acc[r] : 0.f;
              X[row * ldx + k] = v;
              if (row < rows) ws.dz[j - 1][o] = v;
            }
          }
        }
      }
      block_sync();
    }
    // The cell: dgates over the gates' activations, dc for the step before.
    for (int i = t; i < kTile * H; i += NT) {
      const int r = i / H, u = i - r * H;
      float di = 0.f, df = 0.f, dg = 0.f, dout = 0.f, dcp = 0.f;
      if (r < rows) {
        const int64_t row = r0 + (int64_t)r * T;
        float* g = ws.gates + row * 4 * H + u;
        const float ig = g[0], fg = g[H], gg = g[2 * H], og = g[3 * H];
        const float cn = ws.c[row * H + u];
        const float cp = s > 0 ? ws.c[(row - 1) * H + u]
                               : (a.c0 ? a.c0[(b0 + r) * a.state_stride + u] : 0.f);
        const float dh = hL[r * L.ldh + u];
        const float tc = tanhf(cn);
        const float dc = dh * og * (1.f - tc * tc) + cL[r * L.ldh + u];
        di = dc * gg * ig * (1.f - ig);
        df = dc * cp * fg * (1.f - fg);
        dg = dc * ig * (1.f - gg * gg);
        dout = dh * tc * og * (1.f - og);
        dcp = dc * fg;
        g[0] = di;
        g[H] = df;
        g[2 * H] = dg;
        g[3 * H] = dout;
      }
      float* z = gL + r * L.ldg + u;
      z[0] = di;
      z[H] = df;
      z[2 * H] = dg;
      z[3 * H] = dout;
      cL[r * L.ldh + u] = dcp;
    }
    block_sync();
    if (s == BI) break;  // the gradient into the burn-in's final state is dropped
    // dh for the step before = dgates W_h^T.
    for (int kt = wave; kt * 16 < H; kt += NW) {
      const int k = kt * 16 + lm;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_zwt(acc, gL, L.ldg, 4 * H, Wo + n.wh, 4 * H, min(k, H - 1), lm, lq);
      if (k < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) hL[(4 * lq + r) * L.ldh + k] = acc[r];
      }
    }
    block_sync();
  }
}

// ------------------------------------------------------------------ launch 2: weight gradients
// dW[M][N] = a^T dz over the suffix rows: k-th row is sequence k / Ls at step BI + k % Ls.
// shift: a's row is h of the step before (h0, or zeros without one, at t = 0).
struct WJob {
  const float* a;
  const float* dz;
  float *gw, *gb;  // gb: null when another job of the same dz writes the bias
  int lda, ldz, M, N, shift;
  int tile0, ntn;  // first block of the job, tiles along N
};

struct WgradArgs {
  WJob job[kJobs];
  int njobs, RL, Ls, T, BI;
  const float* h0;
  int64_t state_stride;
};

__global__ void ACME_NO_PK_F32 __launch_bounds__(256) r2d2_mlp_wgrad_kernel(const WgradArgs a) {
  __shared__ float part[4][4][64];
  __shared__ float bpart[4][16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lq = lane >> 4;
  int ji = 0;
  while (ji + 1 < a.njobs && (int)blockIdx.x >= a.job[ji + 1].tile0) ++ji;
  const WJob& jb = a.job[ji];
  const int tl = blockIdx.x - jb.tile0, mt = tl / jb.ntn, nt = tl - mt * jb.ntn;
  const int mi = mt * 16 + lm, ni = nt * 16 + lm;
  const bool mon = mi < jb.M, non = ni < jb.N;
  const int mc = min(mi, jb.M - 1), nc = min(ni, jb.N - 1);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float bs = 0.f;
  // Four of the wave's row groups per pass, their loads before their MFMAs; rows past RL are
  // clamped for the load and count as zero.
  for (int k0 = 4 * wave; k0 < a.RL; k0 += 64) {
    float av[4], zv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kr = k0 + 16 * u + lq, kk = min(kr, a.RL - 1);
      const bool on = kr < a.RL;
      const int b = kk / a.Ls, s = a.BI + kk - b * a.Ls;
      const int64_t row = (int64_t)b * a.T + s;
      float x = 0.f;
      if (on && mon) {
        if (!jb.shift) x = jb.a[row * jb.lda + mc];
        else if (s > 0) x = jb.a[(row - 1) * jb.lda + mc];
        else if (a.h0) x = a.h0[b * a.state_stride + mc];
      }
      av[u] = x;
      zv[u] = on && non ? jb.dz[row * jb.ldz + nc] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc = mfma16(av[u], zv[u], acc);
      bs += zv[u];
    }
  }
  // The four waves' partials in wave order; the bias: the four row groups of a wave in order.
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][r][lane] = acc[r];
  bs = ((__shfl(bs, lm, 64) + __shfl(bs, lm + 16, 64)) + __shfl(bs, lm + 32, 64)) +
       __shfl(bs, lm + 48, 64);
  if (lane < 16) bpart[wave][lane] = bs;
  block_sync();
  if (wave != 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float v = ((part[0][r][lane] + part[1][r][lane]) + part[2][r][lane]) + part[3][r][lane];
    const int m = mt * 16 + 4 * lq + r;
    if (m < jb.M && non) jb.gw[(int64_t)m * jb.N + ni] = v;
  }
  if (jb.gb && mt == 0 && lane < 16 && non)
    jb.gb[ni] = ((bpart[0][lane] + bpart[1][lane]) + bpart[2][lane]) + bpart[3][lane];
}

// ------------------------------------------------------------------ launch 3: loss, Adam, target
struct ApplyArgs {
  float* p;
  const float* g;
  float *m, *v;
  float* target;  // null: no copy due
  int64_t n4;
  const double* loss_part;
  int B;
  float lr, b1, omb1, b2, omb2, bc1, bc2, eps;
  float* loss;
};

__global__ void ACME_NO_PK_F32 __launch_bounds__(256) r2d2_mlp_apply_kernel(const ApplyArgs a) {
  const int t = threadIdx.x;
  if (blockIdx.x == 0 && t == 0) {  // the mean over the sequences, in order
    double s = 0.0;
    for (int b = 0; b < a.B; ++b) s += a.loss_part[b];
    a.loss[0] = (float)(s / (double)a.B);
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < a.n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 gg = reinterpret_cast<const f32x4*>(a.g)[i];
    f32x4 mm = reinterpret_cast<const f32x4*>(a.m)[i];
    f32x4 vv = reinterpret_cast<const f32x4*>(a.v)[i];
    f32x4 pp = reinterpret_cast<const f32x4*>(a.p)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // adam_update4's operations, snt.Adam's order
      const float gj = gg[j];
      const float mj = __fadd_rn(__fmul_rn(a.b1, mm[j]), __fmul_rn(a.omb1, gj));
      const float vj = __fadd_rn(__fmul_rn(a.b2, vv[j]), __fmul_rn(a.omb2, __fmul_rn(gj, gj)));
      const float mh = __fdiv_rn(mj, a.bc1);
      const float vh = __fdiv_rn(vj, a.bc2);
      const float den = __fadd_rn(__fsqrt_rn(vh), a.eps);
      mm[j] = mj;
      vv[j] = vj;
      pp[j] = __fsub_rn(pp[j], __fdiv_rn(__fmul_rn(a.lr, mh), den));
    }
    reinterpret_cast<f32x4*>(a.m)[i] = mm;
    reinterpret_cast<f32x4*>(a.v)[i] = vv;
    reinterpret_cast<f32x4*>(a.p)[i] = pp;
    if (a.target) reinterpret_cast<f32x4*>(a.target)[i] = pp;  // after the update
  }
}

// ------------------------------------------------------------------ acting: one launch
struct QStepArgs {
  const float* params;  // the network to act with
  Net net;
  LdsMap lds;
  const float *obs, *h, *c;
  int64_t state_stride;
  int rows;
  double epsilon;
  uint64_t seed, step;
  float* q;          // each optional
  int32_t* actions;
  float *h_out, *c_out;
};

__global__ void ACME_NO_PK_F32 __launch_bounds__(256) r2d2_mlp_q_step_kernel(const QStepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const Net& n = a.net;
  const LdsMap& L = a.lds;
  const int D = n.D, H = n.H, A = n.A;
  const int b0 = blockIdx.x * kTile, rows = min(kTile, a.rows - b0);
  const float* W[2] = {a.params, a.params};
  for (int i = t; i < kTile * H; i += 256) {
    const int r = i / H, u = i - r * H;
    lds[L.h[0] + r * L.ldh + u] = r < rows ? a.h[(b0 + r) * a.state_stride + u] : 0.f;
    lds[L.c[0] + r * L.ldh + u] = r < rows ? a.c[(b0 + r) * a.state_stride + u] : 0.f;
  }
  for (int i = t; i < kTile * D; i += 256) {
    const int r = i / D, k = i - r * D;
    lds[L.obs + r * L.ldo + k] = r < rows ? a.obs[(int64_t)(b0 + r) * D + k] : 0.f;
  }
  block_sync();
  gates_phase<4>(lds, L, n, W, 1);
  block_sync();
  cell_phase<4>(lds, L, n, 1, 0, 0, rows, nullptr, false, false);
  block_sync();
  for (int i = t; i < rows * H; i += 256) {  // every row's state was read before the first barrier
    const int r = i / H, u = i - r * H;
    if (a.h_out) a.h_out[(int64_t)(b0 + r) * H + u] = lds[L.h[0] + r * L.ldh + u];
    if (a.c_out) a.c_out[(int64_t)(b0 + r) * H + u] = lds[L.c[0] + r * L.ldh + u];
  }
  float* qout[2] = {a.q, nullptr};
  for (int j = 0; j <= n.L; ++j) {
    layer_phase<4>(lds, L, n, W, 1, j, b0, 1, rows, nullptr, qout);
    block_sync();
  }
  if (!a.actions) return;
  // One wave per row: lane l holds q[l] (A <= 64), acme_epsilon_greedy's rule.
  for (int r = wave; r < rows; r += 4) {
    float qv[kActSlots];
#pragma unroll
    for (int i = 0; i < kActSlots; ++i) qv[i] = 0.f;
    qv[0] = lane < A ? lds[L.q[0] + r * L.ldq + lane] : 0.f;
    const int action = select_action(qv, A, lane, (uint32_t)(b0 + r), a.epsilon, a.seed, a.step);
    if (lane == 0) a.actions[b0 + r] = action;
  }
}

}  // namespace

struct acme_r2d2_mlp {
  acme_r2d2_mlp_config cfg;
  std::vector<Tensor> tensors;
  int64_t flat = 0;
  std::vector<void*> allocs;
  float *params = nullptr, *target = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  int64_t num_steps = 0;
  Net net;
  LdsMap lds;
  Workspace ws;
  int t_wi, t_wh, t_bl, t_w[kMaxL + 1], t_b[kMaxL + 1];
  int lds_step = 0, lds_act = 0;  // dynamic LDS bytes of the two fused kernels
  bool weights_lds = false;       // the unroll stages both flat buffers in LDS
  bool wide = false;              // the unroll runs 8 waves: the target network on its own four
  bool lds_allowed = false;       // the kernels' dynamic LDS sizes are set (first call)
  float* err_tmp = nullptr;       // outputs the caller did not ask for
  double* prio_tmp = nullptr;
  float* loss_tmp = nullptr;
  int64_t last_batch = 0, last_T = 0;
};

namespace {

static_assert(kActSlots * 64 >= ACME_R2D2_MLP_MAX_ACTIONS, "select_action holds a q row");

int check_config(const acme_r2d2_mlp_config* c) {
  ACME_CHECK_ARG(c, "null config");
  ACME_CHECK_ARG(c->obs_dim >= 1 && c->obs_dim <= ACME_R2D2_MLP_MAX_WIDTH,
                 "obs_dim must be in [1, %d], got %d", ACME_R2D2_MLP_MAX_WIDTH, c->obs_dim);
  ACME_CHECK_ARG(c->num_hidden >= 1 && c->num_hidden <= kMaxL,
                 "num_hidden must be in [1, %d], got %d", kMaxL, c->num_hidden);
  for (int i = 0; i < c->num_hidden; ++i)
    ACME_CHECK_ARG(c->hidden[i] >= 1 && c->hidden[i] <= ACME_R2D2_MLP_MAX_WIDTH,
                   "hidden[%d] must be in [1, %d], got %d", i, ACME_R2D2_MLP_MAX_WIDTH,
                   c->hidden[i]);
  ACME_CHECK_ARG(c->lstm_size >= 1 && c->lstm_size <= ACME_R2D2_MLP_MAX_LSTM,
                 "lstm_size must be in [1, %d], got %d", ACME_R2D2_MLP_MAX_LSTM, c->lstm_size);
  ACME_CHECK_ARG(c->num_actions >= 1 && c->num_actions <= ACME_R2D2_MLP_MAX_ACTIONS,
                 "num_actions must be in [1, %d], got %d", ACME_R2D2_MLP_MAX_ACTIONS,
                 c->num_actions);
  ACME_CHECK_ARG(c->max_batch >= 1 && c->max_batch <= ACME_R2D2_MLP_MAX_ROWS,
                 "max_batch must be in [1, %d], got %d", ACME_R2D2_MLP_MAX_ROWS, c->max_batch);
  ACME_CHECK_ARG(c->max_sequence_length >= 2 && c->max_sequence_length <= ACME_R2D2_MLP_MAX_T,
                 "max_sequence_length must be in [2, %d], got %d", ACME_R2D2_MLP_MAX_T,
                 c->max_sequence_length);
  ACME_CHECK_ARG(c->burn_in_length >= 0 && c->burn_in_length <= c->max_sequence_length - 2,
                 "burn_in_length must be in [0, max_sequence_length - 2 = %d], got %d",
                 c->max_sequence_length - 2, c->burn_in_length);
  ACME_CHECK_ARG(c->n_step >= 1, "n_step must be >= 1, got %d", c->n_step);
  ACME_CHECK_ARG(c->target_update_period >= 1, "target_update_period must be >= 1, got %d",
                 c->target_update_period);
  ACME_CHECK_ARG(c->max_replay_size >= 1, "max_replay_size must be >= 1");
  ACME_CHECK_ARG(c->learning_rate >= 0.f && std::isfinite(c->learning_rate),
                 "learning_rate must be finite and >= 0");
  ACME_CHECK_ARG(c->adam_beta1 >= 0.f && c->adam_beta1 < 1.f, "adam_beta1 must be in [0, 1)");
  ACME_CHECK_ARG(c->adam_beta2 >= 0.f && c->adam_beta2 < 1.f, "adam_beta2 must be in [0, 1)");
  ACME_CHECK_ARG(c->adam_epsilon > 0.f, "adam_epsilon must be > 0");
  return ACME_OK;
}

// The LDS map at the limits, in bytes: per row the observations (260 floats), and per network
// h and c (2 x 132), the larger of the gates (516) and the MLP's two buffers (2 x 260) and the
// q row (68); then the table's three arrays of 16 x 128 floats.
constexpr int kRegAtLimits =
    std::max(lds_stride(4 * ACME_R2D2_MLP_MAX_LSTM), 2 * lds_stride(ACME_R2D2_MLP_MAX_WIDTH));
static_assert(4 * kTile * (lds_stride(ACME_R2D2_MLP_MAX_WIDTH) +
                           2 * (2 * lds_stride(ACME_R2D2_MLP_MAX_LSTM) + kRegAtLimits +
                                lds_stride(ACME_R2D2_MLP_MAX_ACTIONS)) +
                           3 * ACME_R2D2_MLP_MAX_T) <= kLdsBytes,
              "a tile of both networks at every limit fits the LDS of one workgroup");

int init_learner(acme_r2d2_mlp* l) {
  const acme_r2d2_mlp_config& c = l->cfg;
  Net& n = l->net;
  n.D = c.obs_dim; n.L = c.num_hidden; n.H = c.lstm_size; n.A = c.num_actions;
  const int D = n.D, H = n.H, A = n.A;
  for (int j = 0; j < kMaxL + 2; ++j) n.hw[j] = 0;
  n.hw[0] = H;
  for (int j = 0; j < n.L; ++j) n.hw[j + 1] = c.hidden[j];
  n.hw[n.L + 1] = A;
  auto off = [&](int t) { return (int)l->tensors[t].offset; };
  n.wi = off(l->t_wi = add_tensor(l, "lstm/w_i", {D, 4 * H}));
  n.wh = off(l->t_wh = add_tensor(l, "lstm/w_h", {H, 4 * H}));
  n.bl = off(l->t_bl = add_tensor(l, "lstm/b", {4 * H}));
  int xmax = 1;
  for (int j = 0; j <= kMaxL; ++j) {
    l->t_w[j] = l->t_b[j] = -1;
    n.w[j] = n.b[j] = 0;
  }
  for (int j = 0; j <= n.L; ++j) {
    const std::string p = "mlp/linear_" + std::to_string(j);
    n.w[j] = off(l->t_w[j] = add_tensor(l, p + "/w", {n.hw[j], n.hw[j + 1]}));
    n.b[j] = off(l->t_b[j] = add_tensor(l, p + "/b", {n.hw[j + 1]}));
    if (j < n.L) xmax = std::max(xmax, n.hw[j + 1]);
  }

  LdsMap& m = l->lds;
  int at = 0;
  auto take = [&](int floats) {
    const int o = at;
    at += floats;
    return o;
  };
  m.ldo = lds_stride(D); m.ldh = lds_stride(H); m.ldg = lds_stride(4 * H);
  m.ldx = lds_stride(xmax); m.ldq = lds_stride(A);
  m.xsz = kTile * m.ldx;
  m.obs = take(kTile * m.ldo);
  for (int k = 0; k < 2; ++k) {  // network 0 first: the acting step's map is its prefix
    m.h[k] = take(kTile * m.ldh);
    m.c[k] = take(kTile * m.ldh);
    m.reg[k] = take(std::max(kTile * m.ldg, 2 * m.xsz));
    m.q[k] = take(kTile * m.ldq);
    if (k == 0) l->lds_act = 4 * at;
  }
  m.tab = at;
  at += 3 * kTile * (c.max_sequence_length - c.burn_in_length);
  m.wts = at;
  l->lds_step = 4 * at;
  // Weights in LDS when both flat buffers fit beside the tile (ACME_V_R2D2_MLP_W: 0 never, 1
  // whenever they fit; unset: the measured default), and the target network on four waves of
  // its own (ACME_V_R2D2_MLP_WAVES: 4 or 8; unset: the measured default).  DESIGN.md 4.4.
  l->weights_lds = tune_variant("R2D2_MLP_W", -1) != 0 && l->lds_step + 8 * l->flat <= kLdsBytes;
  if (l->weights_lds) l->lds_step += 8 * (int)l->flat;
  l->wide = tune_variant("R2D2_MLP_WAVES", 8) == 8;

  const int64_t R = (int64_t)c.max_batch * c.max_sequence_length;
  Workspace& w = l->ws;
  int rc;
  for (int j = 0; j < kMaxL; ++j) w.a[j] = nullptr;
  for (int j = 0; j <= kMaxL; ++j) w.dz[j] = nullptr;
  for (int j = 0; j <= n.L; ++j) {
    if (j < n.L && (rc = dev_alloc(l, &w.a[j], R * n.hw[j + 1]))) return rc;
    if ((rc = dev_alloc(l, &w.dz[j], R * n.hw[j + 1]))) return rc;
  }
  if ((rc = dev_alloc(l, &w.gates, R * 4 * H)) || (rc = dev_alloc(l, &w.h, R * H)) ||
      (rc = dev_alloc(l, &w.c, R * H)) || (rc = dev_alloc(l, &w.q, R * A)) ||
      (rc = dev_alloc(l, &w.tq, R * A)) || (rc = dev_alloc(l, &w.g, R)) ||
      (rc = dev_alloc(l, &w.loss_part, c.max_batch)) || (rc = dev_alloc(l, &l->err_tmp, R)) ||
      (rc = dev_alloc(l, &l->prio_tmp, c.max_batch)) || (rc = dev_alloc(l, &l->loss_tmp, 1)))
    return rc;
  return ACME_OK;
}

template <bool WL, int NW>
int allow_unroll(int bytes) {
  ACME_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(r2d2_mlp_unroll_kernel<WL, NW>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return ACME_OK;
}

int allow_lds(acme_r2d2_mlp* l) {  // on the device the handle is first used on
  if (l->lds_allowed) return ACME_OK;
  int rc;
  if (l->weights_lds)
    rc = l->wide ? allow_unroll<true, 8>(l->lds_step) : allow_unroll<true, 4>(l->lds_step);
  else
    rc = l->wide ? allow_unroll<false, 8>(l->lds_step) : allow_unroll<false, 4>(l->lds_step);
  if (rc != ACME_OK) return rc;
  ACME_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(r2d2_mlp_q_step_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, l->lds_act));
  l->lds_allowed = true;
  return ACME_OK;
}

int step_impl(acme_r2d2_mlp* l, const acme_sequence_batch* bt, const double* probs,
              const acme_r2d2_outputs* out, hipStream_t st) {
  const acme_r2d2_mlp_config& c = l->cfg;
  const Net& n = l->net;
  const int B = (int)bt->batch, T = (int)bt->sequence_length, BI = c.burn_in_length;
  const int Ls = T - BI, RL = B * Ls;
  const int D = n.D, H = n.H;
  const int tiles = (int)ceil_div(B, kTile);
  if (int rc = allow_lds(l)) return rc;
  double mac_lstm = (double)D * 4 * H + (double)H * 4 * H, mac_mlp = 0.0;
  for (int j = 0; j <= n.L; ++j) mac_mlp += (double)n.hw[j] * n.hw[j + 1];
  const bool state = c.store_lstm_state != 0;
  {
    ACME_PROF_PEAK("r2d2_mlp_unroll", st,
                   2.0 * (2.0 * B * T * mac_lstm + 2.0 * RL * mac_mlp) +
                       2.0 * RL * ((double)H * 4 * H + mac_mlp),
                   0.0, kPeakF32MfmaTflops);
    UnrollArgs a;
    a.params = l->params; a.target = l->target; a.flat = (int)l->flat;
    a.net = n; a.lds = l->lds; a.ws = l->ws;
    a.lds.wts = l->lds.tab + 3 * kTile * Ls;  // the table is sized by this step's T
    a.obs = static_cast<const float*>(bt->observation);
    a.action = bt->action; a.reward = bt->reward; a.discount = bt->discount;
    a.h0 = state ? bt->h0 : nullptr; a.c0 = state ? bt->c0 : nullptr;
    a.state_stride = bt->state_stride;
    a.probs = probs;
    a.B = B; a.T = T; a.BI = BI; a.n_step = c.n_step;
    a.gamma = c.discount;
    a.eta = (float)c.max_priority_weight;
    a.one_minus_eta = (float)(1.0 - c.max_priority_weight);
    a.beta = c.importance_sampling_exponent;
    a.n_replay = (double)c.max_replay_size;
    a.errors = out && out->errors ? out->errors : l->err_tmp;
    a.prio = out && out->priorities ? out->priorities : l->prio_tmp;
    const size_t smem = (size_t)l->lds_step;
    if (l->weights_lds) {
      if (l->wide) r2d2_mlp_unroll_kernel<true, 8><<<(unsigned)tiles, 512, smem, st>>>(a);
      else r2d2_mlp_unroll_kernel<true, 4><<<(unsigned)tiles, 256, smem, st>>>(a);
    } else {
      if (l->wide) r2d2_mlp_unroll_kernel<false, 8><<<(unsigned)tiles, 512, smem, st>>>(a);
      else r2d2_mlp_unroll_kernel<false, 4><<<(unsigned)tiles, 256, smem, st>>>(a);
    }
    ACME_LAUNCH_CHECK();
  }
  {
    ACME_PROF_PEAK("r2d2_mlp_wgrad", st, 2.0 * RL * (mac_lstm + mac_mlp), 0.0, kPeakF32MfmaTflops);
    WgradArgs a;
    a.njobs = 0; a.RL = RL; a.Ls = Ls; a.T = T; a.BI = BI;
    a.h0 = state ? bt->h0 : nullptr; a.state_stride = bt->state_stride;
    int tile0 = 0;
    auto add = [&](const float* x, int lda, int M, const float* dz, int N, int tw, int tb,
                   int shift) {
      WJob& j = a.job[a.njobs++];
      j.a = x; j.lda = lda; j.M = M; j.dz = dz; j.ldz = N; j.N = N; j.shift = shift;
      j.gw = Pm(l, l->grads, tw);
      j.gb = tb >= 0 ? Pm(l, l->grads, tb) : nullptr;
      j.tile0 = tile0; j.ntn = (int)ceil_div(N, 16);
      tile0 += (int)ceil_div(M, 16) * j.ntn;
    };
    add(static_cast<const float*>(bt->observation), D, D, l->ws.gates, 4 * H, l->t_wi, l->t_bl, 0);
    add(l->ws.h, H, H, l->ws.gates, 4 * H, l->t_wh, -1, 1);
    for (int j = 0; j <= n.L; ++j)
      add(j ? l->ws.a[j - 1] : l->ws.h, n.hw[j], n.hw[j], l->ws.dz[j], n.hw[j + 1], l->t_w[j],
          l->t_b[j], 0);
    for (int j = a.njobs; j < kJobs; ++j) a.job[j] = a.job[0];
    r2d2_mlp_wgrad_kernel<<<(unsigned)tile0, 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  {
    ACME_PROF("r2d2_mlp_apply", st, 0.0, 8.0 * 4.0 * (double)l->flat);
    const float t = (float)(l->num_steps + 1);
    ApplyArgs a;
    a.p = l->params; a.g = l->grads; a.m = l->m; a.v = l->v;
    // learning.py:185-189: the copy is due on the pre-increment count, after the update.
    a.target = l->num_steps % c.target_update_period == 0 ? l->target : nullptr;
    a.n4 = l->flat / 4;  // tensors start at multiples of 64 floats
    a.loss_part = l->ws.loss_part; a.B = B;
    a.lr = c.learning_rate;
    a.b1 = c.adam_beta1; a.omb1 = 1.f - c.adam_beta1;
    a.b2 = c.adam_beta2; a.omb2 = 1.f - c.adam_beta2;
    a.bc1 = 1.f - powf(c.adam_beta1, t); a.bc2 = 1.f - powf(c.adam_beta2, t);
    a.eps = c.adam_epsilon;
    a.loss = out && out->loss ? out->loss : l->loss_tmp;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(a.n4, 256), 1024);
    r2d2_mlp_apply_kernel<<<std::max(grid, 1u), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  return ACME_OK;
}

}  // namespace

extern "C" {

int acme_r2d2_mlp_create(const acme_r2d2_mlp_config* cfg, acme_r2d2_mlp** out) {
  ACME_CHECK_ARG(out, "null output handle");
  int rc = check_config(cfg);
  if (rc != ACME_OK) return rc;
  acme_r2d2_mlp* l = new acme_r2d2_mlp();
  l->cfg = *cfg;
  rc = init_learner(l);
  if (rc != ACME_OK) {
    acme_r2d2_mlp_destroy(l);
    return rc;
  }
  *out = l;
  return ACME_OK;
}

int acme_r2d2_mlp_destroy(acme_r2d2_mlp* l) {
  if (!l) return ACME_OK;
  // An actor's last q step may still be queued.
  (void)hipDeviceSynchronize();
  for (void* p : l->allocs) (void)hipFree(p);
  delete l;
  return ACME_OK;
}

int64_t acme_r2d2_mlp_flat_size(const acme_r2d2_mlp* l) { return l ? l->flat : 0; }
int32_t acme_r2d2_mlp_num_tensors(const acme_r2d2_mlp* l) {
  return l ? (int32_t)l->tensors.size() : 0;
}

int acme_r2d2_mlp_tensor_info(const acme_r2d2_mlp* l, int32_t i, int64_t* offset, int64_t* numel,
                              int32_t* ndim, int64_t* shape4, const char** name) {
  return tensor_info(l, i, offset, numel, ndim, shape4, name);
}

int acme_r2d2_mlp_bind(acme_r2d2_mlp* l, float* params, float* target, float* grads,
                       float* adam_m, float* adam_v) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(params && target && grads && adam_m && adam_v, "null buffer");
  l->params = params;
  l->target = target;
  l->grads = grads;
  l->m = adam_m;
  l->v = adam_v;
  return ACME_OK;
}

int acme_r2d2_mlp_step(acme_r2d2_mlp* l, const acme_sequence_batch* b,
                       const double* probabilities, const acme_r2d2_outputs* out, void* stream) {
  ACME_CHECK_ARG(l && b && probabilities, "null argument");
  ACME_CHECK_ARG(l->params, "acme_r2d2_mlp_step before acme_r2d2_mlp_bind");
  ACME_CHECK_ARG(b->batch >= 1 && b->batch <= l->cfg.max_batch,
                 "batch must be in [1, max_batch = %d], got %lld", l->cfg.max_batch,
                 (long long)b->batch);
  ACME_CHECK_ARG(b->sequence_length >= l->cfg.burn_in_length + 2 &&
                     b->sequence_length <= l->cfg.max_sequence_length,
                 "sequence_length must be in [burn_in_length + 2 = %d, %d], got %lld",
                 l->cfg.burn_in_length + 2, l->cfg.max_sequence_length,
                 (long long)b->sequence_length);
  ACME_CHECK_ARG(b->observation && b->action && b->reward && b->discount, "null batch field");
  ACME_CHECK_ARG(!l->cfg.store_lstm_state ||
                     (b->h0 && b->c0 && b->state_stride >= l->cfg.lstm_size),
                 "the core state needs h0, c0 and state_stride >= lstm_size = %d",
                 l->cfg.lstm_size);
  const int rc = step_impl(l, b, probabilities, out, as_stream(stream));
  if (rc != ACME_OK) return rc;
  l->last_batch = b->batch;
  l->last_T = b->sequence_length;
  ++l->num_steps;
  return ACME_OK;
}

int acme_r2d2_mlp_q_step(acme_r2d2_mlp* l, const float* obs, const float* h, const float* c,
                         int64_t state_stride, int64_t rows, int32_t use_target, double epsilon,
                         uint64_t seed, uint64_t step_counter, float* q, int32_t* actions,
                         float* h_out, float* c_out, void* stream) {
  ACME_CHECK_ARG(l && obs && h && c, "null argument");
  ACME_CHECK_ARG(l->params, "acme_r2d2_mlp_q_step before acme_r2d2_mlp_bind");
  ACME_CHECK_ARG(rows >= 1 && rows <= l->cfg.max_batch,
                 "rows must be in [1, max_batch = %d], got %lld", l->cfg.max_batch,
                 (long long)rows);
  ACME_CHECK_ARG(epsilon >= 0.0 && epsilon <= 1.0, "epsilon must be in [0, 1]");  // NaN fails
  ACME_CHECK_ARG(state_stride >= l->cfg.lstm_size,
                 "state_stride must be >= lstm_size = %d, got %lld", l->cfg.lstm_size,
                 (long long)state_stride);
  ACME_CHECK_ARG(state_stride == l->cfg.lstm_size || (h_out != h && c_out != c),
                 "a state output may alias its input only with state_stride == lstm_size");
  if (int rc = allow_lds(l)) return rc;
  hipStream_t st = as_stream(stream);
  ACME_PROF("r2d2_mlp_q_step", st, 0.0, 0.0);
  QStepArgs a;
  a.params = use_target ? l->target : l->params;
  a.net = l->net; a.lds = l->lds;
  a.obs = obs; a.h = h; a.c = c; a.state_stride = state_stride; a.rows = (int)rows;
  a.epsilon = epsilon; a.seed = seed; a.step = step_counter;
  a.q = q; a.actions = actions; a.h_out = h_out; a.c_out = c_out;
  r2d2_mlp_q_step_kernel<<<(unsigned)ceil_div(rows, kTile), 256, (size_t)l->lds_act, st>>>(a);
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

int64_t acme_r2d2_mlp_num_steps(const acme_r2d2_mlp* l) { return l ? l->num_steps : 0; }

int acme_r2d2_mlp_set_num_steps(acme_r2d2_mlp* l, int64_t n) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(n >= 0, "num_steps must be >= 0, got %lld", (long long)n);
  l->num_steps = n;
  return ACME_OK;
}

int acme_r2d2_mlp_debug_buffer(const acme_r2d2_mlp* l, const char* name, const float** out,
                               int64_t* count) {
  ACME_CHECK_ARG(l && name && out && count, "null argument");
  const int64_t B = l->last_batch, T = l->last_T, R = B * T;
  const int64_t H = l->net.H, A = l->net.A;
  const DebugItem items[] = {
      {"q", l->ws.q, R * A},
      {"target_q", l->ws.tq, R * A},
      {"g", l->ws.g, (T - l->cfg.burn_in_length) * B},
      {"h", l->ws.h, R * H},
  };
  return find_debug_buffer(items, name, out, count);
}

}  // extern "C"
