// ------------------------------------------------------------------ MPO
// The kernels only MPO's step has: the Gaussian policy head, the action sampling, the critic
// head over N sampled actions per state with the TD loss, the decoupled MPO loss
// (acme/tf/losses/mpo.py:145-430) with its backward, and the dual variables' finalize + Adam.
// DMPO's step adds one: the mixture of the sampled categorical distributions with the
// categorical loss (dmpo_mix_loss_kernel).
//
// A section of d4pg.hip kept in a file of its own: included there once, inside its anonymous
// namespace, after the device helpers it uses (wave_sum, wave_max, head_dot_row, act_bwd,
// kMaxWidth).  Not a stand-alone header.

constexpr int kMpoCols = 16 + 2 * ACME_D4PG_MAX_ACT;  // per-state sums of mpo_loss_kernel
enum {
  kMcLse = 0, kMcGap, kMcKl, kMcPLse, kMcPGap, kMcPKl, kMcCeMean, kMcCeStd, kMcQMin, kMcQMax,
  kMcSdMin, kMcSdMax, kMcSdCond,
  kMcKlMean = 16,                        // + d
  kMcKlStd = 16 + ACME_D4PG_MAX_ACT,     // + d
};
constexpr float kMinLogDual = -18.f;   // mpo.py:193-194
constexpr float kDualEps = 1e-8f;      // _MPO_FLOAT_EPSILON

__device__ __forceinline__ float softplusf(float x) {
  return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
// softplus(max(-18, log_dual)) + 1e-8 (mpo.py:195-205): the projection is an assign, which
// mpo_finalize_kernel performs; readers before it project on the fly.
__device__ __forceinline__ float dual_value(float log_dual) {
  return softplusf(fmaxf(log_dual, kMinLogDual)) + kDualEps;
}

// MultivariateNormalDiagHead (distributional.py:109-118): mean = h Wm + bm, stddev =
// softplus(h Ws + bs) * init_scale / softplus(0) + min_scale.  One wave per row, the online
// and the target evaluation in one launch (blockIdx.y).
struct GaussHeadArgs {
  const float *h, *wm, *bm, *ws, *bs;
  int rows;
  float *mean, *pre, *sd;  // [rows][A]
};
struct GaussHeadPair {
  GaussHeadArgs a[2];
  int H, A;
  float scale_mul, min_scale;  // init_scale / softplus(0)
};

__global__ void __launch_bounds__(256) gauss_head_kernel(const GaussHeadPair pr) {
  const GaussHeadArgs& a = pr.a[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;  // uniform per wave
  const float* h = a.h + (size_t)row * pr.H;
  const float m = head_dot_row(h, a.wm, pr.H, pr.A, lane);
  const float s = head_dot_row(h, a.ws, pr.H, pr.A, lane);
  if (lane < pr.A) {
    const size_t i = (size_t)row * pr.A + lane;
    const float pre = s + a.bs[lane];
    a.mean[i] = m + a.bm[lane];
    if (a.pre) a.pre[i] = pre;
    a.sd[i] = softplusf(pre) * pr.scale_mul + pr.min_scale;
  }
}

// Four standard normals from one Philox4x32-10 call (include/acme_hip.h, "Sampling noise").
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;  // (0, 1], exact
  const float u2 = (float)(b >> 8) * 0x1p-24f;         // [0, 1), exact
  const float rad = sqrtf(-2.f * logf(u1));
  float sn, cs;
  sincospif(2.f * u2, &sn, &cs);  // the angle 2 pi u2 without rounding 2 pi u2
  z0 = rad * cs;
  z1 = rad * sn;
}
__device__ __forceinline__ void philox_normals(uint64_t seed, uint64_t step, uint32_t idx,
                                               float (&z)[4], uint32_t tag = kMpoNoiseTag) {
  const u32x4 c = {idx, (uint32_t)step, (uint32_t)(step >> 32), tag};
  const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  box_muller(r.x, r.y, z[0], z[1]);
  box_muller(r.z, r.w, z[2], z[3]);
}

// a[n, b, :] = mean_t[b] + stddev_t[b] * eps[n, b, :] (learning.py:197), the out-of-bound
// cost -|a - clip(a, -1, 1)|_2 (mpo.py:233-234) and o_t tiled N times for the target critic's
// first layer.  One thread per (n, b) row; eps from `noise_in`, or generated with the step
// number read from the device (a captured graph replays with the current step).
struct MpoSampleArgs {
  const float *mean, *sd;  // target policy [B][A]
  const float* noise_in;   // [N B][A] or null
  const float* o_t;        // [B][od]
  const int64_t* dev_step;
  uint64_t seed;
  int B, N, A, od;
  float *noise, *act, *cost, *tiled;
};

__global__ void __launch_bounds__(256) mpo_sample_kernel(const MpoSampleArgs a) {
  const int rows = a.N * a.B;
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row < rows) {
    const int b = row % a.B;
    const uint64_t step = (uint64_t)*a.dev_step;
    const uint32_t e0 = (uint32_t)row * (uint32_t)a.A;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t cur = 0xffffffffu;
    float c2 = 0.f;
    for (int d = 0; d < a.A; ++d) {
      const uint32_t e = e0 + d;
      float ep;
      if (a.noise_in) {
        ep = a.noise_in[e];
      } else {
        if ((e >> 2) != cur) {
          cur = e >> 2;
          philox_normals(a.seed, step, cur, z);
        }
        const uint32_t k = e & 3u;
        ep = k == 0 ? z[0] : k == 1 ? z[1] : k == 2 ? z[2] : z[3];
      }
      const float act = a.mean[b * a.A + d] + a.sd[b * a.A + d] * ep;
      const float diff = act - fminf(fmaxf(act, -1.f), 1.f);
      c2 = fmaf(diff, diff, c2);
      a.noise[e] = ep;
      a.act[e] = act;
    }
    a.cost[row] = -sqrtf(c2);
  }
  const int total = rows * a.od, per = a.B * a.od;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256)
    a.tiled[i] = a.o_t[i % per];
}

// The scalar critic head over the target critic's N B rows and the online critic's B rows,
// the TD loss against q_t = mean_n sampled_q and the online head's input gradient
// (learning.py:201-217): ddpg_head_td_kernel's role without dpg rows.  One wave per state b.
struct MpoHeadTdArgs {
  const float *h, *w, *b;     // online critic: last hidden [B][H], head [H], [1]
  const float *th, *tw, *tb;  // target critic: [N B][H], [H], [1]
  const float *r, *d;         // [B]
  int B, N, H, act;
  float discount;
  float *q, *sq, *qt, *td, *dq, *loss;  // [B], [N B], [B], [B], [B], [B]
  float* dz;                            // [B][H]
};

__global__ void __launch_bounds__(256) mpo_head_td_kernel(const MpoHeadTdArgs a) {
  using f32x4 = gemm::f32x4;
  constexpr int kV = kMaxWidth / 256;  // float4 groups per lane
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;  // uniform per wave
  const int n4 = a.H / 4;
  const f32x4* __restrict__ h4 = reinterpret_cast<const f32x4*>(a.h + (size_t)b * a.H);
  const f32x4* __restrict__ w4 = reinterpret_cast<const f32x4*>(a.w);
  const f32x4* __restrict__ tw4 = reinterpret_cast<const f32x4*>(a.tw);
  f32x4 hv[kV], wv[kV], twv[kV];
#pragma unroll
  for (int u = 0; u < kV; ++u) {
    const int k = min(lane + 64 * u, n4 - 1);
    hv[u] = h4[k];
    wv[u] = w4[k];
    twv[u] = tw4[k];
  }
  const float tb = a.tb[0];
  float qsum = 0.f;
  for (int n = 0; n < a.N; ++n) {
    const size_t row = (size_t)n * a.B + b;
    const f32x4* __restrict__ th4 = reinterpret_cast<const f32x4*>(a.th + row * a.H);
    f32x4 thv[kV];
#pragma unroll
    for (int u = 0; u < kV; ++u) thv[u] = th4[min(lane + 64 * u, n4 - 1)];
    float tacc = 0.f;
#pragma unroll
    for (int u = 0; u < kV; ++u) {
      if (lane + 64 * u >= n4) break;
#pragma unroll
      for (int j = 0; j < 4; ++j) tacc = fmaf(thv[u][j], twv[u][j], tacc);
    }
    const float tq = wave_sum(tacc) + tb;
    if (lane == 0) a.sq[row] = tq;
    qsum += tq;  // in n order
  }
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < kV; ++u) {
    if (lane + 64 * u >= n4) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(hv[u][j], wv[u][j], acc);
  }
  const float q = wave_sum(acc) + a.b[0];
  const float qt = qsum / (float)a.N;
  const float pcont = a.discount * a.d[b];
  const float td = (a.r[b] + pcont * qt) - q;
  const float dq = -td / (float)a.B;
  if (lane == 0) {
    a.q[b] = q;
    a.qt[b] = qt;
    a.td[b] = td;
    a.dq[b] = dq;
    a.loss[b] = 0.5f * td * td;
  }
  f32x4* __restrict__ dz4 = reinterpret_cast<f32x4*>(a.dz + (size_t)b * a.H);
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

// The decoupled MPO loss of one state per wave (4 states per block): lane n < N holds sample
// n of the state, lane d < A dimension d of its two distributions.
//   weights: w = softmax_n(q / T), log-sum-exp max-subtracted; the same for the out-of-bound
//     cost with the penalty temperature; wsum = w + pw                     mpo.py:216-246, 318-354
//   cross entropies -sum_n wsum_n log N(a_n; mu_on, sd_t) and ... N(a_n; mu_t, sd_on)  :250-259
//   KL(target || fixed-stddev)_d = (mu_t - mu_on)^2 / (2 sd_t^2),
//   KL(target || fixed-mean)_d = log(sd_on / sd_t) + sd_t^2 / (2 sd_on^2) - 1/2        :262-271
//     (evaluated in a form that keeps its digits when sd_on is near sd_t, see below)
//   dloss / d mu_on, d sd_on -> d(pre-softplus scale) with stop_grad(alpha) on the KLs, and
//   the policy head's input gradient dz = act'(h) * (dmean Wm^T + dpre Ws^T).
// What the batch means and the dual gradients need is summed per block (LDS, fixed order)
// into part[block][kMpoCols]; mpo_finalize_kernel sums the blocks.
struct MpoLossArgs {
  const float *sq, *cost, *act;                       // [N B], [N B], [N B][A]
  const float *mu_on, *sd_on, *pre_on, *mu_t, *sd_t;  // [B][A]
  const float *log_temp, *log_amean, *log_astd, *log_ptemp;  // duals; log_ptemp null: no penalty
  int B, N, A, D, H, act_fn;
  float scale_mul;
  const float *h, *wm, *ws;  // online policy: last hidden [B][H], head weights [H][A]
  float *dmean, *dpre;       // [B][A]
  float* dz;                 // [B][H]
  float *w_out, *pw_out;     // [N B]
  float* part;               // [gridDim.x][kMpoCols]
};

// w = softmax over the wave's live lanes of x / temp; returns also the log-sum-exp, the gap
// lse - sum w x / temp (the part of d loss / d temp that depends on the state; both terms
// taken relative to the maximum, so a temperature at its floor, where x / temp is ~1e7, costs
// no digits) and the non-parametric KL sum w log(N w + 1e-8) (mpo.py:357-366).
__device__ __forceinline__ float tempered_weights(float x, bool on, float temp, int N, float& lse,
                                                  float& gap, float& kl) {
  const float tq = on ? x / temp : -INFINITY;
  const float mx = wave_max(tq);
  const float e = on ? expf(tq - mx) : 0.f;
  const float s = wave_sum(e);
  const float w = e / s;
  lse = mx + logf(s);
  gap = logf(s) - wave_sum(on ? w * (tq - mx) : 0.f);
  kl = wave_sum(on ? w * logf((float)N * w + 1e-8f) : 0.f);
  return w;
}

__global__ void __launch_bounds__(256) mpo_loss_kernel(const MpoLossArgs a) {
  constexpr int AM = ACME_D4PG_MAX_ACT;
  constexpr float kHalfLog2Pi = 0.91893853320467274178f;
  __shared__ float rows_s[4][kMpoCols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  if (b < a.B) {  // uniform per wave
    const bool on = lane < a.N;
    const size_t row = (size_t)min(lane, a.N - 1) * a.B + b;
    const float q = a.sq[row];
    float lse, gap, kl, plse = 0.f, pgap = 0.f, pkl = 0.f;
    const float w = tempered_weights(q, on, dual_value(a.log_temp[0]), a.N, lse, gap, kl);
    float wsum = w;
    if (a.log_ptemp) {
      const float pw = tempered_weights(a.cost[row], on, dual_value(a.log_ptemp[0]), a.N, plse,
                                        pgap, pkl);
      wsum += pw;
      if (on) a.pw_out[row] = pw;
    }
    if (on) a.w_out[row] = w;
    const float W = wave_sum(wsum);
    const float qmin = -wave_max(on ? -q : -INFINITY), qmax = wave_max(on ? q : -INFINITY);
    // Lane d: dimension d of the two distributions.
    const bool dn = lane < a.A;
    const size_t di = (size_t)b * a.A + min(lane, a.A - 1);
    const float mu_on = a.mu_on[di], sd_on = a.sd_on[di], pre_on = a.pre_on[di];
    const float mu_t = a.mu_t[di], sd_t = a.sd_t[di];
    // sum_n wsum (a - mu_on), wsum (a - mu_on)^2, wsum (a - mu_t)^2 of this lane's dimension.
    float s1 = 0.f, s1q = 0.f, s2q = 0.f;
    for (int d = 0; d < a.A; ++d) {
      const float m_on = __shfl(mu_on, d, 64), m_t = __shfl(mu_t, d, 64);
      const float av = a.act[row * a.A + d];
      const float x1 = av - m_on, x2 = av - m_t;
      const float wx1 = on ? wsum * x1 : 0.f;
      const float t1 = wave_sum(wx1), t1q = wave_sum(wx1 * x1);
      const float t2q = wave_sum(on ? wsum * x2 * x2 : 0.f);
      if (lane == d) {
        s1 = t1;
        s1q = t1q;
        s2q = t2q;
      }
    }
    float ce_m = 0.f, ce_s = 0.f, klm = 0.f, kls = 0.f, dmu = 0.f, dpr = 0.f;
    if (dn) {
      const float vt = sd_t * sd_t, von = sd_on * sd_on;
      ce_m = 0.5f * s1q / vt + W * (logf(sd_t) + kHalfLog2Pi);
      ce_s = 0.5f * s2q / von + W * (logf(sd_on) + kHalfLog2Pi);
      const float dm = mu_on - mu_t;
      klm = dm * dm / (2.f * vt);
      // log(sd_on / sd_t) + sd_t^2 / (2 sd_on^2) - 1/2 with u = sd_t / sd_on - 1 is
      // u + u^2 / 2 - log1p(u): near u = 0 (the regime epsilon_stddev = 1e-6 holds the policy
      // in) the written form loses everything below an ulp of 1/2, this one an ulp of u.
      const float u = (sd_t - sd_on) / sd_on;
      kls = (u - log1pf(u)) + 0.5f * u * u;
      const int j = a.D == 1 ? 0 : lane;
      const float am = dual_value(a.log_amean[j]), as = dual_value(a.log_astd[j]);
      const float invB = 1.f / (float)a.B;
      dmu = (am * dm - s1) / vt * invB;
      // d KL / d sd_on = 1 / sd_on - sd_t^2 / sd_on^3 = -u (2 + u) / sd_on.
      const float ds = ((W / sd_on - s2q / (von * sd_on)) - as * u * (2.f + u) / sd_on) * invB;
      dpr = ds * sigmoidf(pre_on) * a.scale_mul;
      a.dmean[di] = dmu;
      a.dpre[di] = dpr;
    }
    // Head input gradient of row b: every lane gets the row's dmean / dpre.
    float gm[AM], gs[AM];
#pragma unroll
    for (int d = 0; d < AM; ++d) {
      gm[d] = __shfl(dmu, d, 64);
      gs[d] = __shfl(dpr, d, 64);
    }
    for (int k = lane; k < a.H; k += 64) {
      float acc = 0.f;
#pragma unroll
      for (int d = 0; d < AM; ++d)
        if (d < a.A) acc = fmaf(gm[d], a.wm[(size_t)k * a.A + d], acc);
#pragma unroll
      for (int d = 0; d < AM; ++d)
        if (d < a.A) acc = fmaf(gs[d], a.ws[(size_t)k * a.A + d], acc);
      const size_t i = (size_t)b * a.H + k;
      a.dz[i] = act_bwd(a.act_fn, a.h[i], acc);
    }
    const float ce_mt = wave_sum(ce_m), ce_st = wave_sum(ce_s);
    const float sdmin = -wave_max(dn ? -sd_on : -INFINITY), sdmax = wave_max(dn ? sd_on : -INFINITY);
    if (lane == 0) {
      float* r = rows_s[wave];
      r[kMcLse] = lse; r[kMcGap] = gap; r[kMcKl] = kl;
      r[kMcPLse] = plse; r[kMcPGap] = pgap; r[kMcPKl] = pkl;
      r[kMcCeMean] = ce_mt; r[kMcCeStd] = ce_st;
      r[kMcQMin] = qmin; r[kMcQMax] = qmax;
      r[kMcSdMin] = sdmin; r[kMcSdMax] = sdmax; r[kMcSdCond] = sdmax / sdmin;
      r[13] = r[14] = r[15] = 0.f;
    }
    if (lane < AM) {
      rows_s[wave][kMcKlMean + lane] = klm;  // 0 for lanes >= A
      rows_s[wave][kMcKlStd + lane] = kls;
    }
  }
  __syncthreads();
  if (threadIdx.x < kMpoCols) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (blockIdx.x * 4 + r < a.B) s += rows_s[r][threadIdx.x];
    a.part[(size_t)blockIdx.x * kMpoCols + threadIdx.x] = s;
  }
}

// DMPO's critic loss (acme/agents/tf/dmpo/learning.py:212-232): the target critic's categorical
// head ran over the N sampled actions of each state; the bootstrap distribution of state b is
// the mixture of its N softmaxes.  d4pg_loss_kernel's layout: one wave per state b, four states
// per block, lane = atom, -inf past K.
//   for n = 0 .. N-1 over row n B + b of the target logits: p_n = softmax (max-subtracted),
//     sq[n B + b] = sum_j p_n[j] values[j] (the sampled q the MPO loss weighs), acc += p_n
//   mixture = acc / sum_j acc
//   categorical_loss_row against the online critic's row b: l2_project, ce[b], dlogits[b]
// The mixture form: the reference takes logsumexp_n(log_softmax_n) as logits (:215-217, without
// subtracting log N) and the loss softmaxes them again; exp(logsumexp_n log p_n) = sum_n p_n, so
// this accumulates sum_n p_n per lane in n order (a fixed order: graph and eager agree bit for
// bit) and normalises it once, with neither the log nor the second exp.
// One wave per state gives only B waves and a chain of N load -> butterfly rounds each, so the
// logits of the next kMixAhead samples are loaded before the current ones are reduced.
constexpr int kMixAhead = 4;
struct DmpoMixArgs {
  const float* c_logits;  // online critic [B][K]
  const float* t_logits;  // target critic over the samples [N B][K]
  const float *r, *d, *values;
  int B, N, K;
  float discount;
  float row_div;          // what the row gradients divide by (DMPO: B; CRR: R T / (T - 1))
  float *sq, *mix;        // [N B], [B][K]
  float *dlogits, *ce;    // [B][K], [B]
};

__global__ void __launch_bounds__(256) dmpo_mix_loss_kernel(const DmpoMixArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;  // uniform per wave
  const bool on = lane < a.K;
  const int col = min(lane, a.K - 1);
  const float vi = on ? a.values[lane] : 0.f;
  const float ql = on ? a.c_logits[(size_t)b * a.K + lane] : -INFINITY;
  // Sample n's logit of this lane (clamped indices: a load past N repeats the last row).
  auto load = [&](int n) {
    return a.t_logits[((size_t)min(n, a.N - 1) * a.B + b) * a.K + col];
  };
  float cur[kMixAhead], nxt[kMixAhead];
#pragma unroll
  for (int u = 0; u < kMixAhead; ++u) cur[u] = load(u);
  float acc = 0.f;
  for (int n0 = 0; n0 < a.N; n0 += kMixAhead) {
#pragma unroll
    for (int u = 0; u < kMixAhead; ++u) nxt[u] = load(n0 + kMixAhead + u);
#pragma unroll
    for (int u = 0; u < kMixAhead; ++u) {
      const int n = n0 + u;
      if (n >= a.N) break;  // uniform
      const RowSoftmax t = row_softmax(on ? cur[u] : -INFINITY, on);
      const float q = wave_sum(on ? t.p * vi : 0.f);
      if (lane == 0) a.sq[(size_t)n * a.B + b] = q;
      acc += t.p;  // in n order
    }
#pragma unroll
    for (int u = 0; u < kMixAhead; ++u) cur[u] = nxt[u];
  }
  const float pj = acc / wave_sum(acc);
  if (on) a.mix[(size_t)b * a.K + lane] = pj;
  const RowSoftmax q = row_softmax(ql, on);
  categorical_loss_row(ql, q, pj, vi, b, lane, a.r, a.d, a.values, a.row_div, a.K, a.discount,
                       a.dlogits, a.ce);
}

// Sums the loss kernel's block partials in a fixed order, then forms the batch means, the dual
// losses and their gradients through the softplus derivative, the reference's stats, and
// applies the duals' Adam (snt.Adam, clip_adam_kernel's operation order, t = the
// step count after this step) to the projected log-duals.  Runs before grad_sumsq advances
// *dev_step, so t = *dev_step + 1.
struct MpoFinalArgs {
  const float* part;
  int nblk, B, N, A, D, penal;
  float *p, *g, *m, *v;  // flat buffers
  int64_t o_temp, o_amean, o_astd, o_ptemp;
  float eps, eps_mean, eps_std, eps_pen;
  float lr, b1, b2, adam_eps;
  const int64_t* dev_step;
  float *stats, *klm_rel, *kls_rel, *ploss;
};

__device__ __forceinline__ void dual_adam(const MpoFinalArgs& a, int64_t i, float p, float g,
                                          float bc1, float bc2) {
  const float mj = __fadd_rn(__fmul_rn(a.b1, a.m[i]), __fmul_rn(1.f - a.b1, g));
  const float vj = __fadd_rn(__fmul_rn(a.b2, a.v[i]), __fmul_rn(1.f - a.b2, __fmul_rn(g, g)));
  const float den = __fadd_rn(__fsqrt_rn(__fdiv_rn(vj, bc2)), a.adam_eps);
  a.g[i] = g;
  a.m[i] = mj;
  a.v[i] = vj;
  a.p[i] = __fsub_rn(p, __fdiv_rn(__fmul_rn(a.lr, __fdiv_rn(mj, bc1)), den));
}

__global__ void __launch_bounds__(256) mpo_finalize_kernel(const MpoFinalArgs a) {
  __shared__ float red[4][64];
  __shared__ float tot[kMpoCols];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  float s = 0.f;
  if (col < kMpoCols)
    for (int i = grp; i < a.nblk; i += 4) s += a.part[(size_t)i * kMpoCols + col];
  red[grp][col] = s;
  __syncthreads();
  if (threadIdx.x < kMpoCols)
    tot[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) +
                       red[3][threadIdx.x];
  __syncthreads();
  // The duals are independent of each other: alpha pair j on lane j of wave 0, the temperature
  // on wave 1, the penalty temperature on wave 2 (one thread doing all of them in turn was
  // 15 us of dependent transcendental chains); thread 0 then adds their terms in a fixed order.
  __shared__ float alpha_s[4][ACME_D4PG_MAX_ACT];  // alpha_mean, alpha_stddev, KL term, dual loss
  __shared__ float temp_s[2][2];                   // temperature / penalty: value, loss
  const float invB = 1.f / (float)a.B;
  const float tf = (float)(*a.dev_step + 1);
  const float bc1 = 1.f - powf(a.b1, tf), bc2 = 1.f - powf(a.b2, tf);
  const float logN = logf((float)a.N);
  if (grp == 0 && col < a.D) {
    // Alphas (compute_parametric_kl_penalty_and_dual_loss), per dimension or on the summed KL.
    const int j = col;
    float klm = tot[kMcKlMean + j], kls = tot[kMcKlStd + j];
    if (a.D == 1)
      for (int d = 1; d < a.A; ++d) {
        klm += tot[kMcKlMean + d];
        kls += tot[kMcKlStd + d];
      }
    const float mklm = klm * invB, mkls = kls * invB;
    const float lm = fmaxf(a.p[a.o_amean + j], kMinLogDual);
    const float ls = fmaxf(a.p[a.o_astd + j], kMinLogDual);
    const float am = softplusf(lm) + kDualEps, as = softplusf(ls) + kDualEps;
    alpha_s[0][j] = am;
    alpha_s[1][j] = as;
    alpha_s[2][j] = am * mklm + as * mkls;
    alpha_s[3][j] = am * (a.eps_mean - mklm) + as * (a.eps_std - mkls);
    dual_adam(a, a.o_amean + j, lm, (a.eps_mean - mklm) * sigmoidf(lm), bc1, bc2);
    dual_adam(a, a.o_astd + j, ls, (a.eps_std - mkls) * sigmoidf(ls), bc1, bc2);
    a.klm_rel[j] = mklm / a.eps_mean;
    a.kls_rel[j] = mkls / a.eps_std;
  } else if ((grp == 1 || grp == 2) && col == 0) {
    // Temperatures (compute_weights_and_temperature_loss): loss = T (eps + mean lse - log N),
    // dloss / dT = that bracket - mean_b sum_n w q / T = eps - log N + mean_b gap.
    const bool pen = grp == 2;
    float T = 0.f, loss = 0.f;
    if (!pen || a.penal) {
      const int64_t o = pen ? a.o_ptemp : a.o_temp;
      const float eps = pen ? a.eps_pen : a.eps;
      const float lt = fmaxf(a.p[o], kMinLogDual);
      T = softplusf(lt) + kDualEps;
      loss = T * (eps + tot[pen ? kMcPLse : kMcLse] * invB - logN);
      dual_adam(a, o, lt, ((eps - logN) + tot[pen ? kMcPGap : kMcGap] * invB) * sigmoidf(lt), bc1,
                bc2);
    }
    temp_s[pen][0] = T;
    temp_s[pen][1] = loss;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float T = temp_s[0][0], loss_temp = temp_s[0][1] + temp_s[1][1];
  float loss_kl = 0.f, loss_alpha = 0.f, am_sum = 0.f, as_sum = 0.f;
  for (int j = 0; j < a.D; ++j) {
    am_sum += alpha_s[0][j];
    as_sum += alpha_s[1][j];
    loss_kl += alpha_s[2][j];
    loss_alpha += alpha_s[3][j];
  }
  const float loss = (tot[kMcCeMean] + tot[kMcCeStd]) * invB + loss_kl + loss_alpha + loss_temp;
  *a.ploss = loss;
  float* st = a.stats;
  st[ACME_MPO_STAT_DUAL_ALPHA_MEAN] = am_sum / (float)a.D;
  st[ACME_MPO_STAT_DUAL_ALPHA_STDDEV] = as_sum / (float)a.D;
  st[ACME_MPO_STAT_DUAL_TEMPERATURE] = T;
  st[ACME_MPO_STAT_LOSS_POLICY] = loss;
  st[ACME_MPO_STAT_LOSS_ALPHA] = loss_alpha;
  st[ACME_MPO_STAT_LOSS_TEMPERATURE] = loss_temp;
  st[ACME_MPO_STAT_KL_Q_REL] = tot[kMcKl] * invB / a.eps;
  st[ACME_MPO_STAT_PENALTY_KL_Q_REL] = a.penal ? tot[kMcPKl] * invB / a.eps_pen : 0.f;
  st[ACME_MPO_STAT_Q_MIN] = tot[kMcQMin] * invB;
  st[ACME_MPO_STAT_Q_MAX] = tot[kMcQMax] * invB;
  st[ACME_MPO_STAT_PI_STDDEV_MIN] = tot[kMcSdMin] * invB;
  st[ACME_MPO_STAT_PI_STDDEV_MAX] = tot[kMcSdMax] * invB;
  st[ACME_MPO_STAT_PI_STDDEV_COND] = tot[kMcSdCond] * invB;
}

