// IMPALA on vector observations for MI355X: IMPALALearner._step
// (acme/agents/tf/impala/learning.py:97-169) for the network of examples/bsuite/run_impala.py,
// snt.DeepRNN([Flatten, snt.nets.MLP(hidden), snt.LSTM(H), PolicyValueHead(A)]), behind the C
// ABI (include/acme_hip.h, acme_impala_mlp_*).  Exact f32 throughout.
//
// One step = three launches on one stream, whatever T and the depth are:
//   impala_mlp_unroll_kernel, one 256-thread workgroup per tile of 16 sequences.  The tile's 16
//     rows are the M dimension of v_mfma_f32_16x16x4_f32; the four waves split each layer's
//     16-column output tiles.  For t = 0..T-1: MLP, gates = x W_i + h W_h + b, cell, both heads,
//     with h, c and the step's layer boundaries in LDS (row stride % 64 == 4: the 16 rows x 4
//     columns of an MFMA row operand fall on all 64 banks) and what the backward needs in a
//     global workspace only this workgroup touches.  Then, per row, log pi / log mu -> the
//     clipped importance weight; the V-trace backward scan, one lane per sequence, on values
//     staged in LDS; d loss / d(logits, value) with the divisor (T-1) B; and the backward
//     through time for t = T-1..0: heads -> dh -> dgates -> (dc, dh_prev) -> dx -> the MLP's dz,
//     the deltas written over the same LDS buffers and to the workspace.
//   impala_mlp_wgrad_kernel, one workgroup per 16 x 16 tile of a weight tensor: dW = a^T dz over
//     the R = B T rows, the four waves taking interleaved groups of four rows and summed in wave
//     order through LDS; the bias (column sums of dz) rides with the tensor's first row of
//     tiles; the block's sum of squares goes to its own slot.
//   impala_mlp_apply_kernel: the norm and the loss partials summed in a fixed order,
//     tf.clip_by_global_norm, snt.Adam at t = num_steps + 1, the four metrics.
// No float atomic anywhere: every sum has a fixed order, so a step repeats bit for bit, and a
// step at (B, T) below the created maxima computes what a learner created at (B, T) computes
// (row indices depend on the step's own B and T only).
//
// Weights are the MFMA B operands.  The unroll reads them either through L2 or, when the
// whole flat buffer fits beside the tile, from a copy staged in LDS at the start of the launch
// (which, and why).  The policy step reads each weight once: always through L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "learner_common.h"
#include "profiler.h"

using namespace acme;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// No packed f32 arithmetic in this file's kernels, and a barrier that inlines into them: see
// mlp_model.hip and DESIGN.md 4.5.
#ifdef __HIP_DEVICE_COMPILE__
#define ACME_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define ACME_NO_PK_F32
#endif
#define ACME_DEV __device__ ACME_NO_PK_F32 __forceinline__

ACME_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int kTile = 16;  // sequences of a workgroup: the MFMA's M
constexpr int kMaxL = ACME_IMPALA_MLP_MAX_HIDDEN;
constexpr int kJobs = kMaxL + 4;              // weight tensors: MLP layers, W_i, W_h, two heads
constexpr int kLdsBytes = 160 * 1024 - 1024;  // dynamic LDS a launch may ask for

// Shapes, and where the tensors start in the flat buffer.
struct Net {
  int D, L, H, A;
  int width[kMaxL + 1];  // width[0] = D, width[j + 1] = hidden[j]
  int w[kMaxL], b[kMaxL];
  int wi, wh, bl, wp, bp, wv, bv;
};

// The tile's LDS map, in floats.  x[j] is the input of MLP layer j (x[L]: the LSTM's input).
struct LdsMap {
  int x[kMaxL + 1], ldx[kMaxL + 1];
  int h, c, ldh;  // [16][H] each; dh and dc in the backward
  int g, ldg;     // [16][4H] gate pre-activations; dgates in the backward
  int pv, ldpv;   // [16][A + 1] logits and value; their gradients in the backward
  int act;        // floats up to here are zeroed at the start of a launch
  int scan;       // [4][16 T]: value, reward -> vs, discount -> advantage, clipped rho
  int wts;        // the flat parameter buffer, when staged
};

// What the unroll leaves for its own backward and for the weight-gradient launch.  Row of
// sequence b at step t: b * T + t.
struct Workspace {
  float* a[kMaxL];   // [R][width[j + 1]] output of MLP layer j (after its ReLU)
  float* dz[kMaxL];  // [R][width[j + 1]] gradient at that layer's pre-activation
  float* gates;      // [R][4H] the gates' activations (i, f, g, o); dgates after the backward
  float *h, *c;      // [R][H]
  float *pv, *dpv;   // [R][A + 1]
  float *vs, *adv;   // [(T - 1) B] time-major
  float* loss_part;  // [tiles][4]: policy-gradient, critic and entropy sums of the tile
};

// Row stride of a tile buffer of `width` columns: the columns up to the next multiple of 64
// exist and stay zero, so the k loops have no branch.
constexpr int lds_stride(int width) { return ((width + 63) & ~63) + 4; }

// A B operand [K][N] in the flat buffer.  The heads are two tensors side by side: column
// n < n1 is tensor `off` (row stride ld), column n1 the one-column tensor `off2`.
struct WMat {
  int off, ld, n1, off2;
};
ACME_DEV int widx(const WMat& m, int k, int n) { return n < m.n1 ? m.off + k * m.ld + n : m.off2 + k; }

// D = A B + C on one wave: A is 16 x 4 (lane holds A[lane % 16][lane / 16]), B is 4 x 16 (lane
// holds B[lane / 16][lane % 16]), the lane's four results are D[4 (lane / 16) + r][lane % 16].
ACME_DEV f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc += X[16][K] W[K][nc]: X in LDS (zero past K), the W index clamped into its tensor.
ACME_DEV f32x4 tile_xw(f32x4 acc, const float* X, int ldx, int K, const float* W, const WMat& m,
                       int nc, int lm, int lq) {
  const float* xa = X + lm * ldx + lq;
  const int K4 = (K + 3) & ~3;
  int k0 = 0;
  // Four steps' operands loaded before their MFMAs (the compiler does not unroll a loop around
  // a convergent operation by itself); the accumulation order is that of the plain loop.
  for (; k0 + 16 <= K4; k0 += 16) {
    float x[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[u] = xa[k0 + 4 * u];
      w[u] = W[widx(m, min(k0 + 4 * u + lq, K - 1), nc)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = mfma16(x[u], w[u], acc);
  }
  for (; k0 < K4; k0 += 4) acc = mfma16(xa[k0], W[widx(m, min(k0 + lq, K - 1), nc)], acc);
  return acc;
}

// acc += dZ[16][N] W[kc][N]^T: dZ in LDS (zero past N).
ACME_DEV f32x4 tile_zwt(f32x4 acc, const float* dZ, int ldz, int N, const float* W, const WMat& m,
                        int kc, int lm, int lq) {
  const float* za = dZ + lm * ldz + lq;
  const int N4 = (N + 3) & ~3;
  int n0 = 0;
  for (; n0 + 16 <= N4; n0 += 16) {  // as tile_xw
    float z[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      z[u] = za[n0 + 4 * u];
      w[u] = W[widx(m, kc, min(n0 + 4 * u + lq, N - 1))];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = mfma16(z[u], w[u], acc);
  }
  for (; n0 < N4; n0 += 4) acc = mfma16(za[n0], W[widx(m, kc, min(n0 + lq, N - 1))], acc);
  return acc;
}

ACME_DEV float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// One network step of a tile: MLP -> cell -> heads.  Tile row r is global row row0 + r * rs of
// `obs` and of the workspace (ws == nullptr: the policy step stores nothing); rows >= rows are
// fed zeros and stored nowhere.  On return h, c and pv in LDS are the step's.
ACME_DEV void forward_step(float* lds, const LdsMap& L, const Net& n, const float* W,
                           const float* obs, int64_t row0, int64_t rs, int rows,
                           const Workspace* ws) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lq = lane >> 4;
  const int D = n.D, H = n.H, A = n.A;
  {
    float* x0 = lds + L.x[0];
    for (int i = t; i < kTile * D; i += 256) {
      const int r = i / D, k = i - r * D;
      x0[r * L.ldx[0] + k] = r < rows ? obs[(row0 + r * rs) * D + k] : 0.f;
    }
  }
  block_sync();
  for (int j = 0; j < n.L; ++j) {
    const int K = n.width[j], N = n.width[j + 1];
    const float* X = lds + L.x[j];
    float* Y = lds + L.x[j + 1];
    const int ldy = L.ldx[j + 1];
    const WMat m{n.w[j], N, N, 0};
    for (int nt = wave; nt * 16 < N; nt += 4) {
      const int col = nt * 16 + lm;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_xw(acc, X, L.ldx[j], K, W, m, min(col, N - 1), lm, lq);
      if (col < N) {
        const float bn = W[n.b[j] + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * lq + r;
          const float z = acc[r] + bn;
          const float y = j + 1 < n.L ? (z > 0.f ? z : 0.f) : z;  // none after the last layer
          Y[row * ldy + col] = y;
          if (ws && row < rows) ws->a[j][(row0 + row * rs) * N + col] = y;
        }
      }
    }
    block_sync();
  }
  float* hL = lds + L.h;
  float* cL = lds + L.c;
  float* gL = lds + L.g;
  {
    const int N = 4 * H;
    const WMat mi{n.wi, N, N, 0}, mh{n.wh, N, N, 0};
    for (int nt = wave; nt * 16 < N; nt += 4) {
      const int col = nt * 16 + lm, nc = min(col, N - 1);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_xw(acc, lds + L.x[n.L], L.ldx[n.L], n.width[n.L], W, mi, nc, lm, lq);
      acc = tile_xw(acc, hL, L.ldh, H, W, mh, nc, lm, lq);
      if (col < N) {
        const float bn = W[n.bl + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) gL[(4 * lq + r) * L.ldg + col] = acc[r] + bn;
      }
    }
  }
  block_sync();
  for (int i = t; i < kTile * H; i += 256) {
    const int r = i / H, u = i - r * H;
    const float* z = gL + r * L.ldg + u;
    const float ig = sigmoidf(z[0]), fg = sigmoidf(z[H]);
    const float gg = tanhf(z[2 * H]), og = sigmoidf(z[3 * H]);
    const float cn = fg * cL[r * L.ldh + u] + ig * gg;
    const float hn = og * tanhf(cn);
    cL[r * L.ldh + u] = cn;
    hL[r * L.ldh + u] = hn;
    if (ws && r < rows) {
      const int64_t row = row0 + r * rs;
      float* g = ws->gates + row * 4 * H + u;
      g[0] = ig;
      g[H] = fg;
      g[2 * H] = gg;
      g[3 * H] = og;
      ws->c[row * H + u] = cn;
      ws->h[row * H + u] = hn;
    }
  }
  block_sync();
  {
    const int N = A + 1;
    float* pv = lds + L.pv;
    const WMat m{n.wp, A, A, n.wv};
    for (int nt = wave; nt * 16 < N; nt += 4) {
      const int col = nt * 16 + lm;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_xw(acc, hL, L.ldh, H, W, m, min(col, N - 1), lm, lq);
      if (col < N) {
        const float bn = col < A ? W[n.bp + col] : W[n.bv];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * lq + r;
          pv[row * L.ldpv + col] = acc[r] + bn;
          if (ws && row < rows) ws->pv[(row0 + row * rs) * N + col] = acc[r] + bn;
        }
      }
    }
  }
  block_sync();
}

// ------------------------------------------------------------------ launch 1: the unroll
struct UnrollArgs {
  const float* params;
  int flat;
  Net net;
  LdsMap lds;
  Workspace ws;
  const float* obs;       // [B][T][D]
  const int32_t* action;  // [B][T]
  const float *reward, *discount, *mu;
  const float *h0, *c0;
  int64_t state_stride;
  int B, T;
  float gamma, entropy_cost, baseline_cost, max_abs_reward;
};

// log softmax(z)[act] of a row of A logits.
ACME_DEV float log_prob(const float* z, int A, int act) {
  float m = z[0];
  for (int j = 1; j < A; ++j) m = fmaxf(m, z[j]);
  float s = 0.f;
  for (int j = 0; j < A; ++j) s += expf(z[j] - m);
  return z[act] - m - logf(s);
}

template <bool WL>
__global__ void ACME_NO_PK_F32 __launch_bounds__(256) impala_mlp_unroll_kernel(const UnrollArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[4][3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lq = lane >> 4;
  const Net& n = a.net;
  const LdsMap& L = a.lds;
  const Workspace& ws = a.ws;
  const int H = n.H, A = n.A, W1 = A + 1, T = a.T;
  const int b0 = blockIdx.x * kTile, rows = min(kTile, a.B - b0);
  for (int i = t; i < L.act; i += 256) lds[i] = 0.f;
  if (WL)
    for (int i = t; i < a.flat; i += 256) lds[L.wts + i] = a.params[i];
  const float* W = WL ? lds + L.wts : a.params;
  float* hL = lds + L.h;
  float* cL = lds + L.c;
  float* gL = lds + L.g;
  float* pvL = lds + L.pv;
  block_sync();
  for (int i = t; i < kTile * H; i += 256) {
    const int r = i / H, u = i - r * H;
    if (r < rows) {
      hL[r * L.ldh + u] = a.h0[(b0 + r) * a.state_stride + u];
      cL[r * L.ldh + u] = a.c0[(b0 + r) * a.state_stride + u];
    }
  }
  for (int s = 0; s < T; ++s)  // its first barrier orders the state above
    forward_step(lds, L, n, W, a.obs, (int64_t)b0 * T + s, T, rows, &ws);

  // ---- V-trace.  Per row: the value, the clipped reward, gamma * discount and
  // min(1, pi(a) / mu(a)) into LDS; then one lane per sequence scans backwards.
  float* sv = lds + L.scan;
  float* sr = sv + kTile * T;
  float* sg = sr + kTile * T;
  float* sc = sg + kTile * T;
  for (int i = t; i < kTile * T; i += 256) {
    const int r = i / T, s = i - r * T;
    float v = 0.f, rw = 0.f, g = 0.f, c = 0.f;
    if (r < rows) {
      const int64_t row = (int64_t)(b0 + r) * T + s;
      const float* z = ws.pv + row * W1;
      v = z[A];
      if (s < T - 1) {
        const int act = min(max(a.action[row], 0), A - 1);  // never an index outside the row
        const float lrho = log_prob(z, A, act) - log_prob(a.mu + row * A, A, act);
        c = fminf(1.f, expf(lrho));
        rw = fminf(fmaxf(a.reward[row], -a.max_abs_reward), a.max_abs_reward);
        g = a.gamma * a.discount[row];
      }
    }
    sv[i] = v;
    sr[i] = rw;
    sg[i] = g;
    sc[i] = c;
  }
  block_sync();
  if (t < rows) {  // trfl.vtrace_from_importance_weights, both thresholds 1
    const int base = t * T;
    const float boot = sv[base + T - 1];
    float acc = 0.f, vs_next = boot, v1 = boot;
    for (int s = T - 2; s >= 0; --s) {
      const float v = sv[base + s], r = sr[base + s], g = sg[base + s], c = sc[base + s];
      acc = c * (r + g * v1 - v) + g * c * acc;
      const float vs = acc + v;
      const float adv = c * (r + g * vs_next - v);
      ws.vs[(int64_t)s * a.B + b0 + t] = vs;
      ws.adv[(int64_t)s * a.B + b0 + t] = adv;
      sr[base + s] = vs;
      sg[base + s] = adv;
      vs_next = vs;
      v1 = v;
    }
  }
  block_sync();
  // ---- d loss / d(logits, value), vs and the advantages as constants; zero at t = T - 1.
  {
    const float invN = 1.f / (float)((T - 1) * a.B);
    float s_pg = 0.f, s_cr = 0.f, s_en = 0.f;
    for (int i = t; i < kTile * T; i += 256) {
      const int r = i / T, s = i - r * T;
      if (r >= rows) continue;
      const int64_t row = (int64_t)(b0 + r) * T + s;
      float* d = ws.dpv + row * W1;
      if (s == T - 1) {
        for (int j = 0; j < W1; ++j) d[j] = 0.f;
        continue;
      }
      const float* z = ws.pv + row * W1;
      float m = z[0];
      for (int j = 1; j < A; ++j) m = fmaxf(m, z[j]);
      float se = 0.f;
      for (int j = 0; j < A; ++j) se += expf(z[j] - m);
      const float lse = m + logf(se);
      float ent = 0.f;
      for (int j = 0; j < A; ++j) {
        const float lp = z[j] - lse;
        ent -= expf(lp) * lp;
      }
      const int act = min(max(a.action[row], 0), A - 1);
      const float adv = sg[i], vs = sr[i], v = sv[i];
      for (int j = 0; j < A; ++j) {
        const float lp = z[j] - lse, pi = expf(lp);
        const float oh = j == act ? 1.f : 0.f;
        d[j] = (-(oh - pi) * adv + a.entropy_cost * pi * (lp + ent)) * invN;
      }
      d[A] = a.baseline_cost * (-2.f) * (vs - v) * invN;
      s_pg += -(z[act] - lse) * adv;
      s_cr += (vs - v) * (vs - v);
      s_en += -ent;
    }
    s_pg = wave_sum(s_pg);
    s_cr = wave_sum(s_cr);
    s_en = wave_sum(s_en);
    if (lane == 0) {
      red[wave][0] = s_pg;
      red[wave][1] = s_cr;
      red[wave][2] = s_en;
    }
  }
  // dh and dc of the step after the last: zero.
  for (int i = t; i < kTile * H; i += 256) {
    const int r = i / H, u = i - r * H;
    hL[r * L.ldh + u] = 0.f;
    cL[r * L.ldh + u] = 0.f;
  }
  block_sync();
  if (t < 3)
    ws.loss_part[blockIdx.x * 4 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];

  // ---- backward through time.
  const WMat mhead{n.wp, A, A, n.wv};
  const WMat mwh{n.wh, 4 * H, 4 * H, 0}, mwi{n.wi, 4 * H, 4 * H, 0};
  for (int s = T - 1; s >= 0; --s) {
    const int64_t row0 = (int64_t)b0 * T + s;
    for (int i = t; i < kTile * W1; i += 256) {
      const int r = i / W1, j = i - r * W1;
      pvL[r * L.ldpv + j] = r < rows ? ws.dpv[(row0 + (int64_t)r * T) * W1 + j] : 0.f;
    }
    block_sync();
    // dh = d(logits, value) [W_p | W_v]^T + dh from the step after.
    for (int kt = wave; kt * 16 < H; kt += 4) {
      const int k = kt * 16 + lm;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_zwt(acc, pvL, L.ldpv, W1, W, mhead, min(k, H - 1), lm, lq);
      if (k < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) hL[(4 * lq + r) * L.ldh + k] += acc[r];
      }
    }
    block_sync();
    // The cell: dgates over the gates' activations, dc for the step before.
    for (int i = t; i < kTile * H; i += 256) {
      const int r = i / H, u = i - r * H;
      float di = 0.f, df = 0.f, dg = 0.f, dout = 0.f, dcp = 0.f;
      if (r < rows) {
        const int64_t row = row0 + (int64_t)r * T;
        float* g = ws.gates + row * 4 * H + u;
        const float ig = g[0], fg = g[H], gg = g[2 * H], og = g[3 * H];
        const float cn = ws.c[row * H + u];
        const float cp = s > 0 ? ws.c[(row - 1) * H + u] : a.c0[(b0 + r) * a.state_stride + u];
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
    // dh for the step before = dgates W_h^T; dx = dgates W_i^T, the MLP's last delta.
    for (int kt = wave; kt * 16 < H; kt += 4) {
      const int k = kt * 16 + lm;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_zwt(acc, gL, L.ldg, 4 * H, W, mwh, min(k, H - 1), lm, lq);
      if (k < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) hL[(4 * lq + r) * L.ldh + k] = acc[r];
      }
    }
    {
      const int K = n.width[n.L];
      float* X = lds + L.x[n.L];
      for (int kt = wave; kt * 16 < K; kt += 4) {
        const int k = kt * 16 + lm;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = tile_zwt(acc, gL, L.ldg, 4 * H, W, mwi, min(k, K - 1), lm, lq);
        if (k < K) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 4 * lq + r;
            X[row * L.ldx[n.L] + k] = acc[r];
            if (row < rows) ws.dz[n.L - 1][(row0 + (int64_t)row * T) * K + k] = acc[r];
          }
        }
      }
    }
    block_sync();
    // MLP: the delta at layer j - 1's output = (delta at layer j's output) W_j^T, masked.
    for (int j = n.L - 1; j >= 1; --j) {
      const int K = n.width[j], N = n.width[j + 1];
      float* X = lds + L.x[j];
      const WMat m{n.w[j], N, N, 0};
      for (int kt = wave; kt * 16 < K; kt += 4) {
        const int k = kt * 16 + lm;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = tile_zwt(acc, lds + L.x[j + 1], L.ldx[j + 1], N, W, m, min(k, K - 1), lm, lq);
        if (k < K) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 4 * lq + r;
            const int64_t o = (row0 + (int64_t)row * T) * K + k;
            const float v = row < rows && ws.a[j - 1][o] > 0.f ? acc[r] : 0.f;
            X[row * L.ldx[j] + k] = v;
            if (row < rows) ws.dz[j - 1][o] = v;
          }
        }
      }
      block_sync();
    }
  }
}

// ------------------------------------------------------------------ launch 2: weight gradients
// dW[M][N] = a[R][M]^T dz[R][N].  shift: a's row m is h of the step before (h0 at t = 0).
struct WJob {
  const float* a;
  const float* dz;
  float *gw, *gb;  // gb: null when another job of the same dz writes the bias
  int lda, ldz, M, N, shift;
  int tile0, ntn;  // first block of the job, tiles along N
};

struct WgradArgs {
  WJob job[kJobs];
  int njobs, R, T, H;
  const float* h0;
  int64_t state_stride;
  double* npart;  // [gridDim.x]
};

__global__ void ACME_NO_PK_F32 __launch_bounds__(256) impala_mlp_wgrad_kernel(const WgradArgs a) {
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
  // Four of the wave's row groups per pass, their loads before their MFMAs; rows past R are
  // clamped for the load and count as zero.
  for (int k0 = 4 * wave; k0 < a.R; k0 += 64) {
    float av[4], zv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kr = k0 + 16 * u + lq, row = min(kr, a.R - 1);
      const bool on = kr < a.R;
      const float* ar;
      if (jb.shift) {
        const int b = row / a.T;
        ar = row - b * a.T == 0 ? a.h0 + b * a.state_stride : jb.a + (int64_t)(row - 1) * jb.lda;
      } else {
        ar = jb.a + (int64_t)row * jb.lda;
      }
      av[u] = on && mon ? ar[mc] : 0.f;
      zv[u] = on && non ? jb.dz[(int64_t)row * jb.ldz + nc] : 0.f;
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
  double ss = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float v = ((part[0][r][lane] + part[1][r][lane]) + part[2][r][lane]) + part[3][r][lane];
    const int m = mt * 16 + 4 * lq + r;
    if (m < jb.M && non) {
      jb.gw[(int64_t)m * jb.N + ni] = v;
      ss += (double)v * (double)v;
    }
  }
  if (jb.gb && mt == 0 && lane < 16 && non) {
    const float v = ((bpart[0][lane] + bpart[1][lane]) + bpart[2][lane]) + bpart[3][lane];
    jb.gb[ni] = v;
    ss += (double)v * (double)v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) a.npart[blockIdx.x] = ss;
}

// ------------------------------------------------------------------ launch 3: clip + Adam
struct ApplyArgs {
  float* p;
  const float* g;
  float *m, *v;
  int64_t n4;
  const double* npart;
  int nparts;
  const float* loss_part;
  int tiles;
  float inv_n, entropy_cost, baseline_cost, clip_norm;
  float lr, b1, omb1, b2, omb2, bc1, bc2, eps;
  float *metrics, *norm;
};

__global__ void ACME_NO_PK_F32 __launch_bounds__(256) impala_mlp_apply_kernel(const ApplyArgs a) {
  __shared__ double red[4];
  __shared__ float scale_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // Every block sums the same partials in the same order.
  double ss = 0.0;
  for (int i = t; i < a.nparts; i += 256) ss += a.npart[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) red[wave] = ss;
  block_sync();
  if (t == 0) {
    const float G = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
    // tf.clip_by_global_norm: t * clip_norm * min(1 / G, 1 / clip_norm).
    scale_s = G > 0.f ? a.clip_norm * fminf(1.f / G, 1.f / a.clip_norm) : 1.f;
    if (blockIdx.x == 0) {
      *a.norm = G;
      float s[3];
      for (int k = 0; k < 3; ++k) {
        s[k] = a.loss_part[k];
        for (int q = 1; q < a.tiles; ++q) s[k] += a.loss_part[q * 4 + k];
        s[k] *= a.inv_n;
      }
      a.metrics[0] = s[0] + a.baseline_cost * s[1] + a.entropy_cost * s[2];
      a.metrics[1] = s[1];
      a.metrics[2] = s[2];
      a.metrics[3] = s[0];
    }
  }
  block_sync();
  const float sc = scale_s;
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < a.n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 gg = reinterpret_cast<const f32x4*>(a.g)[i];
    f32x4 mm = reinterpret_cast<const f32x4*>(a.m)[i];
    f32x4 vv = reinterpret_cast<const f32x4*>(a.v)[i];
    f32x4 pp = reinterpret_cast<const f32x4*>(a.p)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // adam_update4's operations, snt.Adam's order
      const float gj = __fmul_rn(gg[j], sc);
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
  }
}

// ------------------------------------------------------------------ acting: one launch
struct PolicyArgs {
  const float* params;
  Net net;
  LdsMap lds;
  const float *obs, *h, *c;
  int rows;
  float *logits, *values, *h_out, *c_out;  // each optional
};

__global__ void ACME_NO_PK_F32 __launch_bounds__(256) impala_mlp_policy_kernel(const PolicyArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int t = threadIdx.x;
  const Net& n = a.net;
  const LdsMap& L = a.lds;
  const int H = n.H, A = n.A;
  const int b0 = blockIdx.x * kTile, rows = min(kTile, a.rows - b0);
  for (int i = t; i < L.act; i += 256) lds[i] = 0.f;
  block_sync();
  float* hL = lds + L.h;
  float* cL = lds + L.c;
  for (int i = t; i < kTile * H; i += 256) {
    const int r = i / H, u = i - r * H;
    if (r < rows) {
      hL[r * L.ldh + u] = a.h[(int64_t)(b0 + r) * H + u];
      cL[r * L.ldh + u] = a.c[(int64_t)(b0 + r) * H + u];
    }
  }
  forward_step(lds, L, n, a.params, a.obs, b0, 1, rows, nullptr);
  const float* pv = lds + L.pv;
  for (int i = t; i < rows * H; i += 256) {
    const int r = i / H, u = i - r * H;
    if (a.h_out) a.h_out[(int64_t)(b0 + r) * H + u] = hL[r * L.ldh + u];
    if (a.c_out) a.c_out[(int64_t)(b0 + r) * H + u] = cL[r * L.ldh + u];
  }
  for (int i = t; i < rows * (A + 1); i += 256) {
    const int r = i / (A + 1), j = i - r * (A + 1);
    const float v = pv[r * L.ldpv + j];
    if (j < A) {
      if (a.logits) a.logits[(int64_t)(b0 + r) * A + j] = v;
    } else if (a.values) {
      a.values[b0 + r] = v;
    }
  }
}

}  // namespace

struct acme_impala_mlp {
  acme_impala_mlp_config cfg;
  std::vector<Tensor> tensors;
  int64_t flat = 0;
  std::vector<void*> allocs;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  int64_t num_steps = 0;
  Net net;
  LdsMap lds;
  Workspace ws;
  int t_w[kMaxL], t_b[kMaxL], t_wi, t_wh, t_bl, t_wp, t_bp, t_wv, t_bv;
  int lds_step = 0, lds_policy = 0;  // dynamic LDS bytes of the two fused kernels
  bool weights_lds = false;          // the unroll stages the flat buffer in LDS
  bool lds_allowed = false;          // the kernels' dynamic LDS sizes are set (first call)
  double* npart = nullptr;           // [wgrad blocks]
  int wgrad_blocks = 0;
  float* tmp = nullptr;  // [4] metrics the caller did not ask for, [4] the gradient norm
  int64_t last_batch = 0, last_T = 0;
};

namespace {

int check_config(const acme_impala_mlp_config* c) {
  ACME_CHECK_ARG(c, "null config");
  ACME_CHECK_ARG(c->obs_dim >= 1 && c->obs_dim <= ACME_IMPALA_MLP_MAX_WIDTH,
                 "obs_dim must be in [1, %d], got %d", ACME_IMPALA_MLP_MAX_WIDTH, c->obs_dim);
  ACME_CHECK_ARG(c->num_hidden >= 1 && c->num_hidden <= kMaxL,
                 "num_hidden must be in [1, %d], got %d", kMaxL, c->num_hidden);
  for (int i = 0; i < c->num_hidden; ++i)
    ACME_CHECK_ARG(c->hidden[i] >= 1 && c->hidden[i] <= ACME_IMPALA_MLP_MAX_WIDTH,
                   "hidden[%d] must be in [1, %d], got %d", i, ACME_IMPALA_MLP_MAX_WIDTH,
                   c->hidden[i]);
  ACME_CHECK_ARG(c->lstm_size >= 1 && c->lstm_size <= ACME_IMPALA_MLP_MAX_LSTM,
                 "lstm_size must be in [1, %d], got %d", ACME_IMPALA_MLP_MAX_LSTM, c->lstm_size);
  ACME_CHECK_ARG(c->num_actions >= 1 && c->num_actions <= ACME_IMPALA_MLP_MAX_ACTIONS,
                 "num_actions must be in [1, %d], got %d", ACME_IMPALA_MLP_MAX_ACTIONS,
                 c->num_actions);
  ACME_CHECK_ARG(c->max_batch >= 1 && c->max_batch <= ACME_IMPALA_MLP_MAX_ROWS,
                 "max_batch must be in [1, %d], got %d", ACME_IMPALA_MLP_MAX_ROWS, c->max_batch);
  ACME_CHECK_ARG(c->max_sequence_length >= 2 && c->max_sequence_length <= ACME_IMPALA_MLP_MAX_T,
                 "max_sequence_length must be in [2, %d], got %d", ACME_IMPALA_MLP_MAX_T,
                 c->max_sequence_length);
  ACME_CHECK_ARG(c->learning_rate >= 0.f && std::isfinite(c->learning_rate),
                 "learning_rate must be finite and >= 0");
  ACME_CHECK_ARG(c->adam_beta1 >= 0.f && c->adam_beta1 < 1.f, "adam_beta1 must be in [0, 1)");
  ACME_CHECK_ARG(c->adam_beta2 >= 0.f && c->adam_beta2 < 1.f, "adam_beta2 must be in [0, 1)");
  ACME_CHECK_ARG(c->adam_epsilon > 0.f, "adam_epsilon must be > 0");
  ACME_CHECK_ARG(c->max_gradient_norm > 0.f, "max_gradient_norm must be > 0");
  ACME_CHECK_ARG(c->max_abs_reward > 0.f, "max_abs_reward must be > 0");
  return ACME_OK;
}

// The LDS map at the limits, in bytes: the activations (4 x 260 + 2 x 132 + 516 + 132 floats per
// row, 16 rows) and the scan's four arrays of 16 x 128 floats.
static_assert(4 * kTile * (4 * lds_stride(ACME_IMPALA_MLP_MAX_WIDTH) +
                           2 * lds_stride(ACME_IMPALA_MLP_MAX_LSTM) +
                           lds_stride(4 * ACME_IMPALA_MLP_MAX_LSTM) +
                           lds_stride(ACME_IMPALA_MLP_MAX_ACTIONS + 1) +
                           4 * ACME_IMPALA_MLP_MAX_T) <= kLdsBytes,
              "a tile at every limit fits the LDS of one workgroup");

int init_learner(acme_impala_mlp* l) {
  const acme_impala_mlp_config& c = l->cfg;
  Net& n = l->net;
  n.D = c.obs_dim; n.L = c.num_hidden; n.H = c.lstm_size; n.A = c.num_actions;
  n.width[0] = c.obs_dim;
  for (int j = 0; j < kMaxL; ++j) {
    l->t_w[j] = l->t_b[j] = -1;
    n.w[j] = n.b[j] = 0;
    n.width[j + 1] = j < n.L ? c.hidden[j] : 0;
  }
  auto off = [&](int t) { return (int)l->tensors[t].offset; };
  for (int j = 0; j < n.L; ++j) {
    const std::string p = "mlp/linear_" + std::to_string(j);
    n.w[j] = off(l->t_w[j] = add_tensor(l, p + "/w", {n.width[j], n.width[j + 1]}));
    n.b[j] = off(l->t_b[j] = add_tensor(l, p + "/b", {n.width[j + 1]}));
  }
  const int H = n.H, A = n.A, X = n.width[n.L];
  n.wi = off(l->t_wi = add_tensor(l, "lstm/w_i", {X, 4 * H}));
  n.wh = off(l->t_wh = add_tensor(l, "lstm/w_h", {H, 4 * H}));
  n.bl = off(l->t_bl = add_tensor(l, "lstm/b", {4 * H}));
  n.wp = off(l->t_wp = add_tensor(l, "policy_value_network/linear/w", {H, A}));
  n.bp = off(l->t_bp = add_tensor(l, "policy_value_network/linear/b", {A}));
  n.wv = off(l->t_wv = add_tensor(l, "policy_value_network/linear_1/w", {H, 1}));
  n.bv = off(l->t_bv = add_tensor(l, "policy_value_network/linear_1/b", {1}));

  LdsMap& m = l->lds;
  int at = 0;
  auto take = [&](int width, int* ld) {
    const int o = at;
    *ld = lds_stride(width);
    at += kTile * *ld;
    return o;
  };
  for (int j = 0; j <= kMaxL; ++j) m.x[j] = m.ldx[j] = 0;
  for (int j = 0; j <= n.L; ++j) m.x[j] = take(n.width[j], &m.ldx[j]);
  m.h = take(H, &m.ldh);
  m.c = take(H, &m.ldh);
  m.g = take(4 * H, &m.ldg);
  m.pv = take(A + 1, &m.ldpv);
  m.act = at;
  l->lds_policy = 4 * at;
  m.scan = at;
  at += 4 * kTile * c.max_sequence_length;
  m.wts = at;
  l->lds_step = 4 * at;
  // Weights in LDS when the flat buffer fits beside the tile (ACME_V_IMPALA_MLP_W: 0 never,
  // 1 whenever it fits; unset: the measured default).
  const int want = tune_variant("IMPALA_MLP_W", -1);
  l->weights_lds = want != 0 && l->lds_step + 4 * l->flat <= kLdsBytes;
  if (l->weights_lds) l->lds_step += 4 * (int)l->flat;

  const int64_t R = (int64_t)c.max_batch * c.max_sequence_length;
  const int64_t tiles = ceil_div(c.max_batch, kTile);
  Workspace& w = l->ws;
  int rc;
  for (int j = 0; j < kMaxL; ++j) w.a[j] = w.dz[j] = nullptr;
  for (int j = 0; j < n.L; ++j)
    if ((rc = dev_alloc(l, &w.a[j], R * n.width[j + 1])) ||
        (rc = dev_alloc(l, &w.dz[j], R * n.width[j + 1])))
      return rc;
  if ((rc = dev_alloc(l, &w.gates, R * 4 * H)) || (rc = dev_alloc(l, &w.h, R * H)) ||
      (rc = dev_alloc(l, &w.c, R * H)) || (rc = dev_alloc(l, &w.pv, R * (A + 1))) ||
      (rc = dev_alloc(l, &w.dpv, R * (A + 1))) || (rc = dev_alloc(l, &w.vs, R)) ||
      (rc = dev_alloc(l, &w.adv, R)) || (rc = dev_alloc(l, &w.loss_part, tiles * 4)) ||
      (rc = dev_alloc(l, &l->tmp, 8)))
    return rc;
  auto tiles_of = [](int M, int N) { return (int)(ceil_div(M, 16) * ceil_div(N, 16)); };
  l->wgrad_blocks = tiles_of(X, 4 * H) + tiles_of(H, 4 * H) + tiles_of(H, A) + tiles_of(H, 1);
  for (int j = 0; j < n.L; ++j) l->wgrad_blocks += tiles_of(n.width[j], n.width[j + 1]);
  return dev_alloc(l, &l->npart, l->wgrad_blocks);
}

int allow_lds(acme_impala_mlp* l) {  // on the device the handle is first used on
  if (l->lds_allowed) return ACME_OK;
  const void* step = l->weights_lds
                         ? reinterpret_cast<const void*>(impala_mlp_unroll_kernel<true>)
                         : reinterpret_cast<const void*>(impala_mlp_unroll_kernel<false>);
  ACME_HIP_TRY(hipFuncSetAttribute(step, hipFuncAttributeMaxDynamicSharedMemorySize, l->lds_step));
  ACME_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(impala_mlp_policy_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, l->lds_policy));
  l->lds_allowed = true;
  return ACME_OK;
}

int step_impl(acme_impala_mlp* l, const acme_sequence_batch* bt, float* metrics, hipStream_t st) {
  const acme_impala_mlp_config& c = l->cfg;
  const Net& n = l->net;
  const int B = (int)bt->batch, T = (int)bt->sequence_length, R = B * T;
  const int H = n.H, A = n.A, X = n.width[n.L];
  const int tiles = (int)ceil_div(B, kTile);
  if (int rc = allow_lds(l)) return rc;
  double mac = (double)X * 4 * H + (double)H * 4 * H + (double)H * (A + 1);
  for (int j = 0; j < n.L; ++j) mac += (double)n.width[j] * n.width[j + 1];
  {
    ACME_PROF_PEAK("impala_mlp_unroll", st, 4.0 * R * mac, 0.0, kPeakF32MfmaTflops);
    UnrollArgs a;
    a.params = l->params; a.flat = (int)l->flat;
    a.net = n; a.lds = l->lds; a.ws = l->ws;
    a.lds.scan = l->lds.act;
    a.lds.wts = l->lds.act + 4 * kTile * T;  // the scan's arrays are sized by this step's T
    a.obs = static_cast<const float*>(bt->observation);
    a.action = bt->action; a.reward = bt->reward; a.discount = bt->discount;
    a.mu = bt->behaviour_logits; a.h0 = bt->h0; a.c0 = bt->c0;
    a.state_stride = bt->state_stride;
    a.B = B; a.T = T;
    a.gamma = c.discount; a.entropy_cost = c.entropy_cost; a.baseline_cost = c.baseline_cost;
    a.max_abs_reward = c.max_abs_reward;
    if (l->weights_lds)
      impala_mlp_unroll_kernel<true><<<(unsigned)tiles, 256, (size_t)l->lds_step, st>>>(a);
    else
      impala_mlp_unroll_kernel<false><<<(unsigned)tiles, 256, (size_t)l->lds_step, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  {
    ACME_PROF_PEAK("impala_mlp_wgrad", st, 2.0 * R * mac, 0.0, kPeakF32MfmaTflops);
    WgradArgs a;
    a.njobs = 0; a.R = R; a.T = T; a.H = H;
    a.h0 = bt->h0; a.state_stride = bt->state_stride; a.npart = l->npart;
    int tile0 = 0;
    auto add = [&](const float* x, int lda, int M, const float* dz, int ldz, int N, int tw, int tb,
                   int shift) {
      WJob& j = a.job[a.njobs++];
      j.a = x; j.lda = lda; j.M = M; j.dz = dz; j.ldz = ldz; j.N = N; j.shift = shift;
      j.gw = Pm(l, l->grads, tw);
      j.gb = tb >= 0 ? Pm(l, l->grads, tb) : nullptr;
      j.tile0 = tile0; j.ntn = (int)ceil_div(N, 16);
      tile0 += (int)ceil_div(M, 16) * j.ntn;
    };
    for (int j = 0; j < n.L; ++j)
      add(j ? l->ws.a[j - 1] : static_cast<const float*>(bt->observation), n.width[j], n.width[j],
          l->ws.dz[j], n.width[j + 1], n.width[j + 1], l->t_w[j], l->t_b[j], 0);
    add(l->ws.a[n.L - 1], X, X, l->ws.gates, 4 * H, 4 * H, l->t_wi, l->t_bl, 0);
    add(l->ws.h, H, H, l->ws.gates, 4 * H, 4 * H, l->t_wh, -1, 1);
    add(l->ws.h, H, H, l->ws.dpv, A + 1, A, l->t_wp, l->t_bp, 0);
    add(l->ws.h, H, H, l->ws.dpv + A, A + 1, 1, l->t_wv, l->t_bv, 0);
    for (int j = a.njobs; j < kJobs; ++j) a.job[j] = a.job[0];
    impala_mlp_wgrad_kernel<<<(unsigned)tile0, 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  {
    ACME_PROF("impala_mlp_apply", st, 0.0, 7.0 * 4.0 * (double)l->flat);
    const float t = (float)(l->num_steps + 1);
    ApplyArgs a;
    a.p = l->params; a.g = l->grads; a.m = l->m; a.v = l->v;
    a.n4 = l->flat / 4;  // tensors start at multiples of 64 floats
    a.npart = l->npart; a.nparts = l->wgrad_blocks;
    a.loss_part = l->ws.loss_part; a.tiles = tiles;
    a.inv_n = 1.f / (float)((T - 1) * B);
    a.entropy_cost = c.entropy_cost; a.baseline_cost = c.baseline_cost;
    a.clip_norm = c.max_gradient_norm;
    a.lr = c.learning_rate;
    a.b1 = c.adam_beta1; a.omb1 = 1.f - c.adam_beta1;
    a.b2 = c.adam_beta2; a.omb2 = 1.f - c.adam_beta2;
    a.bc1 = 1.f - powf(c.adam_beta1, t); a.bc2 = 1.f - powf(c.adam_beta2, t);
    a.eps = c.adam_epsilon;
    a.metrics = metrics ? metrics : l->tmp;
    a.norm = l->tmp + 4;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(a.n4, 256), 1024);
    impala_mlp_apply_kernel<<<std::max(grid, 1u), 256, 0, st>>>(a);
    ACME_LAUNCH_CHECK();
  }
  return ACME_OK;
}

}  // namespace

extern "C" {

int acme_impala_mlp_create(const acme_impala_mlp_config* cfg, acme_impala_mlp** out) {
  ACME_CHECK_ARG(out, "null output handle");
  int rc = check_config(cfg);
  if (rc != ACME_OK) return rc;
  acme_impala_mlp* l = new acme_impala_mlp();
  l->cfg = *cfg;
  rc = init_learner(l);
  if (rc != ACME_OK) {
    acme_impala_mlp_destroy(l);
    return rc;
  }
  *out = l;
  return ACME_OK;
}

int acme_impala_mlp_destroy(acme_impala_mlp* l) {
  if (!l) return ACME_OK;
  // An actor-side network may be dropped with its last policy step still queued.
  (void)hipDeviceSynchronize();
  for (void* p : l->allocs) (void)hipFree(p);
  delete l;
  return ACME_OK;
}

int64_t acme_impala_mlp_flat_size(const acme_impala_mlp* l) { return l ? l->flat : 0; }
int32_t acme_impala_mlp_num_tensors(const acme_impala_mlp* l) {
  return l ? (int32_t)l->tensors.size() : 0;
}

int acme_impala_mlp_tensor_info(const acme_impala_mlp* l, int32_t i, int64_t* offset,
                                int64_t* numel, int32_t* ndim, int64_t* shape4,
                                const char** name) {
  return tensor_info(l, i, offset, numel, ndim, shape4, name);
}

int acme_impala_mlp_bind(acme_impala_mlp* l, float* params, float* grads, float* adam_m,
                         float* adam_v) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(params && grads && adam_m && adam_v, "null buffer");
  l->params = params;
  l->grads = grads;
  l->m = adam_m;
  l->v = adam_v;
  return ACME_OK;
}

int acme_impala_mlp_step(acme_impala_mlp* l, const acme_sequence_batch* b, float* metrics,
                         void* stream) {
  ACME_CHECK_ARG(l && b, "null argument");
  ACME_CHECK_ARG(l->params, "acme_impala_mlp_step before acme_impala_mlp_bind");
  ACME_CHECK_ARG(b->batch >= 1 && b->batch <= l->cfg.max_batch,
                 "batch must be in [1, max_batch = %d], got %lld", l->cfg.max_batch,
                 (long long)b->batch);
  ACME_CHECK_ARG(b->sequence_length >= 2 && b->sequence_length <= l->cfg.max_sequence_length,
                 "sequence_length must be in [2, max_sequence_length = %d], got %lld",
                 l->cfg.max_sequence_length, (long long)b->sequence_length);
  ACME_CHECK_ARG(b->observation && b->action && b->reward && b->discount &&
                     b->behaviour_logits && b->h0 && b->c0,
                 "null batch field");
  ACME_CHECK_ARG(b->state_stride >= l->cfg.lstm_size,
                 "state_stride must be >= lstm_size = %d, got %lld", l->cfg.lstm_size,
                 (long long)b->state_stride);
  const int rc = step_impl(l, b, metrics, as_stream(stream));
  if (rc != ACME_OK) return rc;
  l->last_batch = b->batch;
  l->last_T = b->sequence_length;
  ++l->num_steps;
  return ACME_OK;
}

int acme_impala_mlp_policy_step(acme_impala_mlp* l, const float* obs, const float* h,
                                const float* c, int64_t rows, float* logits, float* values,
                                float* h_out, float* c_out, void* stream) {
  ACME_CHECK_ARG(l && obs && h && c, "null argument");
  ACME_CHECK_ARG(l->params, "acme_impala_mlp_policy_step before acme_impala_mlp_bind");
  ACME_CHECK_ARG(rows >= 1 && rows <= l->cfg.max_batch,
                 "rows must be in [1, max_batch = %d], got %lld", l->cfg.max_batch,
                 (long long)rows);
  if (int rc = allow_lds(l)) return rc;
  hipStream_t st = as_stream(stream);
  ACME_PROF("impala_mlp_policy", st, 0.0, 0.0);
  PolicyArgs a;
  a.params = l->params; a.net = l->net; a.lds = l->lds;
  a.obs = obs; a.h = h; a.c = c; a.rows = (int)rows;
  a.logits = logits; a.values = values; a.h_out = h_out; a.c_out = c_out;
  impala_mlp_policy_kernel<<<(unsigned)ceil_div(rows, kTile), 256, (size_t)l->lds_policy, st>>>(a);
  ACME_LAUNCH_CHECK();
  return ACME_OK;
}

int64_t acme_impala_mlp_num_steps(const acme_impala_mlp* l) { return l ? l->num_steps : 0; }

int acme_impala_mlp_set_num_steps(acme_impala_mlp* l, int64_t n) {
  ACME_CHECK_ARG(l, "null learner");
  ACME_CHECK_ARG(n >= 0, "num_steps must be >= 0, got %lld", (long long)n);
  l->num_steps = n;
  return ACME_OK;
}

int acme_impala_mlp_debug_buffer(const acme_impala_mlp* l, const char* name, const float** out,
                                 int64_t* count) {
  ACME_CHECK_ARG(l && name && out && count, "null argument");
  const int64_t B = l->last_batch, T = l->last_T, R = B * T;
  const int64_t H = l->net.H, A = l->net.A;
  const DebugItem items[] = {
      {"pv", l->ws.pv, R * (A + 1)},   {"dpv", l->ws.dpv, R * (A + 1)},
      {"vs", l->ws.vs, (T - 1) * B},   {"pg_adv", l->ws.adv, (T - 1) * B},
      {"h", l->ws.h, R * H},           {"grad_norm", l->tmp + 4, 1},
  };
  return find_debug_buffer(items, name, out, count);
}

}  // extern "C"
