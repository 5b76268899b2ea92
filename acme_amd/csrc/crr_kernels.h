// ------------------------------------------------------------------ CRR
// The kernels only CRR's step has (acme/agents/tf/crr/recurrent_learning.py:197-377 for
// stateless networks): the draw of its two action sets and the advantage-weighted
// behaviour-cloning loss with its backward into the Gaussian head.  The policy head, the
// mixture of the sampled distributions and the categorical loss are MPO's and DMPO's
// (mpo_kernels.h).
//
// A section of d4pg.hip kept in a file of its own: included there once, inside its anonymous
// namespace, after mpo_kernels.h (philox_normals, sigmoidf, row_softmax, act_bwd).  Not a
// stand-alone header.

// Both action sets of a step in one launch, one thread per row of the concatenated
// [(N_td + N_pw) R][A] buffers:
//   rows [0, N_td R):               a = mean_t[b] + sd_t[b] eps at o_t, for the target critic
//                                   (:253-263), o_t tiled beside them
//   rows [N_td R, (N_td + N_pw) R): a = mean_on[b] + sd_on[b] eps at o_tm1, for the online
//                                   critic (:285-292), o_tm1 tiled
// eps from `noise_in`, or generated over the concatenated element index under kCrrNoiseTag
// with the step number read from the device (a captured graph replays with the current step).
struct CrrSampleArgs {
  const float *mean_t, *sd_t;    // target policy at o_t [R][A]
  const float *mean_on, *sd_on;  // online policy at o_tm1 [R][A]
  const float* noise_in;         // [(N_td + N_pw) R][A] or null
  const float *o_t, *o_tm1;      // [R][od]
  const int64_t* dev_step;
  uint64_t seed;
  int R, Ntd, Npw, A, od;
  float *noise, *act, *tiled;    // [(N_td + N_pw) R][A], the same, [(N_td + N_pw) R][od]
};

__global__ void __launch_bounds__(256) crr_sample_kernel(const CrrSampleArgs a) {
  const int split = a.Ntd * a.R, rows = split + a.Npw * a.R;
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row < rows) {
    const bool tgt = row < split;
    const int b = (tgt ? row : row - split) % a.R;
    const float* __restrict__ mean = tgt ? a.mean_t : a.mean_on;
    const float* __restrict__ sd = tgt ? a.sd_t : a.sd_on;
    const uint64_t step = (uint64_t)*a.dev_step;
    const uint32_t e0 = (uint32_t)row * (uint32_t)a.A;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t cur = 0xffffffffu;
    for (int d = 0; d < a.A; ++d) {
      const uint32_t e = e0 + d;
      float ep;
      if (a.noise_in) {
        ep = a.noise_in[e];
      } else {
        if ((e >> 2) != cur) {
          cur = e >> 2;
          philox_normals(a.seed, step, cur, z, kCrrNoiseTag);
        }
        const uint32_t k = e & 3u;
        ep = k == 0 ? z[0] : k == 1 ? z[1] : k == 2 ? z[2] : z[3];
      }
      a.noise[e] = ep;
      a.act[e] = mean[b * a.A + d] + sd[b * a.A + d] * ep;
    }
  }
  const int per = a.R * a.od, tsplit = split * a.od, total = rows * a.od;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256)
    a.tiled[i] = i < tsplit ? a.o_t[i % per] : a.o_tm1[(i - tsplit) % per];
}

// The policy loss of one state per wave (4 states per block), mpo_loss_kernel's layout: lane j
// < K atom j of the online critic's distributions, lane d < A dimension d of the online policy
// at o_tm1 (:279-329).
//   q_tm1_mean = sum_j softmax(logits[b])[j] values[j]
//   v_n = the same of the sampled row R + n R + b, n < N_pw (the logits of the next kMixAhead
//     samples are loaded before the current ones are reduced, as dmpo_mix_loss_kernel does);
//     V = mean / max / min over n, in n order
//   advantage = q_tm1_mean - V; coef = min(exp(advantage / beta), bound) | advantage > 0 | 1
//     (an overflowing exp is +inf, and the minimum is the bound)
//   logp = sum_d [-1/2 ((a - mu) / sd)^2 - log sd] - A/2 log 2 pi; row loss -logp coef
//   with g = coef / row_div (row_div = R T / (T - 1), coef behind a stop-gradient):
//     dmean = -g (a - mu) / sd^2, dsd = g (1 - z^2) / sd, dpre = dsd sigmoid(pre) scale_mul
//   the head's input gradient dz = act'(h) * (dmean Wm^T + dpre Ws^T).
// The row losses and coefficients are summed per block (LDS, fixed order) into loss_part /
// coef_part[block]; clip_adam_kernel sums the loss's blocks, crr_coef_mean_kernel the
// coefficient's.
struct CrrLossArgs {
  const float* logits;  // online critic [(1 + N_pw) R][K]
  const float* values;  // [K]
  const float *a_tm1, *mu, *sd, *pre;  // [R][A]
  int R, N, K, A, H, act_fn, reduce, mode;
  float beta, bound, scale_mul, row_div;
  const float *h, *wm, *ws;  // online policy: last hidden [R][H], head weights [H][A]
  float *q_mean, *v_est, *adv, *coef, *logp;  // [R]
  float *dmean, *dpre;                        // [R][A]
  float* dz;                                  // [R][H]
  float *loss_part, *coef_part;               // [gridDim.x]
};

__global__ void __launch_bounds__(256) crr_policy_loss_kernel(const CrrLossArgs a) {
  constexpr int AM = ACME_D4PG_MAX_ACT;
  constexpr float kHalfLog2Pi = 0.91893853320467274178f;
  __shared__ float rows_s[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  if (b < a.R) {  // uniform per wave
    const bool on = lane < a.K;
    const int col = min(lane, a.K - 1);
    const float vi = on ? a.values[lane] : 0.f;
    const float ql = on ? a.logits[(size_t)b * a.K + lane] : -INFINITY;
    // Lane d: dimension d of the action and of the distribution.
    const bool dn = lane < a.A;
    const size_t di = (size_t)b * a.A + min(lane, a.A - 1);
    const float av = a.a_tm1[di], mu = a.mu[di], sd = a.sd[di], pre = a.pre[di];
    // Sample n's logit of this lane (clamped indices: a load past N repeats the last row).
    auto load = [&](int n) {
      return a.logits[((size_t)(1 + min(n, a.N - 1)) * a.R + b) * a.K + col];
    };
    float cur[kMixAhead], nxt[kMixAhead];
#pragma unroll
    for (int u = 0; u < kMixAhead; ++u) cur[u] = load(u);
    float v = 0.f;
    for (int n0 = 0; n0 < a.N; n0 += kMixAhead) {
#pragma unroll
      for (int u = 0; u < kMixAhead; ++u) nxt[u] = load(n0 + kMixAhead + u);
#pragma unroll
      for (int u = 0; u < kMixAhead; ++u) {
        const int n = n0 + u;
        if (n >= a.N) break;  // uniform
        const RowSoftmax t = row_softmax(on ? cur[u] : -INFINITY, on);
        const float q = wave_sum(on ? t.p * vi : 0.f);
        // In n order.
        v = n == 0 ? q
            : a.reduce == ACME_CRR_REDUCE_MEAN ? v + q
            : a.reduce == ACME_CRR_REDUCE_MAX  ? fmaxf(v, q)
                                               : fminf(v, q);
      }
#pragma unroll
      for (int u = 0; u < kMixAhead; ++u) cur[u] = nxt[u];
    }
    if (a.reduce == ACME_CRR_REDUCE_MEAN) v = v / (float)a.N;
    const RowSoftmax qs = row_softmax(ql, on);
    const float qm = wave_sum(on ? qs.p * vi : 0.f);
    const float adv = qm - v;
    const float coef = a.mode == ACME_CRR_MODE_EXP      ? fminf(expf(adv / a.beta), a.bound)
                       : a.mode == ACME_CRR_MODE_BINARY ? (adv > 0.f ? 1.f : 0.f)
                                                        : 1.f;
    const float z = (av - mu) / sd;
    const float logp = wave_sum(dn ? -0.5f * z * z - logf(sd) : 0.f) - (float)a.A * kHalfLog2Pi;
    const float g = coef / a.row_div;
    float dmu = 0.f, dpr = 0.f;
    if (dn) {
      dmu = -g * z / sd;
      dpr = g * (1.f - z * z) / sd * sigmoidf(pre) * a.scale_mul;
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
    if (lane == 0) {
      a.q_mean[b] = qm;
      a.v_est[b] = v;
      a.adv[b] = adv;
      a.coef[b] = coef;
      a.logp[b] = logp;
      rows_s[wave][0] = -logp * coef;
      rows_s[wave][1] = coef;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (blockIdx.x * 4 + r < a.R) s += rows_s[r][threadIdx.x];
    (threadIdx.x == 0 ? a.loss_part : a.coef_part)[blockIdx.x] = s;
  }
}

// The logged mean coefficient: one wave sums the loss kernel's per-block coefficient sums
// (lane-strided partials, then a fixed shuffle tree: deterministic) and divides by row_div.
__global__ void __launch_bounds__(64) crr_coef_mean_kernel(const float* __restrict__ part, int n,
                                                           float row_div,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x;
  float t = 0.f;
  for (int i = lane; i < n; i += 64) t += part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  if (lane == 0) *out = t / row_div;
}
