// ------------------------------------------------------------------ ExpQ acting
// The exponentially Q-weighted acting policy (acme/tf/networks/stochastic.py:49-104) over the
// learners with a Gaussian policy head (MPO, DMPO, CRR): per observation, N actions
// a_n = mean + stddev eps_n from the policy, q_n from the critic at (o, a_n) (the categorical
// head's mean over the support, or the scalar head), p = softmax(q / beta) over the N samples,
// and one inverse-CDF draw of a uniform against the running sum of p in sample order.
//
// Two paths give the same index (and values within the forward bar of each other):
//   one launch  expq_act_fused_kernel: a 256-thread workgroup per observation.  The policy is
//               mat-vecs through LDS (bc_act_fused_kernel's column / k-group split), LayerNorm +
//               tanh after the first layer, ELU after the others, head_dot_row for the two head
//               rows.  The critic's first layer is z_obs = o W[:obs_dim] + b once, plus each
//               sample's rank-act_dim term; its hidden layers and the categorical head are 16-row
//               tiles on v_mfma_f32_16x16x4_f32 with X in LDS (stride % 64 == 4) and W streamed
//               from global / L2, the 16-column tiles dealt round-robin to the four waves; N > 16
//               runs as ceil(N / 16) sample tiles through the same two buffers.  Wave 0 selects.
//   layered     the policy forward of acme_*_policy, expq_sample_kernel (the draw, o tiled N
//               times), the critic over the rows x N rows on the GEMM engine, and
//               expq_select_kernel (head mean, softmax over N, draw, gather).
// No float atomics; every sum has a fixed order, so a call repeats bit for bit.
//
// Path limits, from profiles/expq/expq_time.json (MI355X, N = 16, device time per call, one
// launch / layered): every layer 64 wide 30 / 57 us, 128 wide 38 / 58 us, 256 wide 63 / 62-65 us
// (a tie), the headline networks (policy 256 x 3, critic 512 / 512 / 256) 106 / 68 us: one
// workgroup streaming a 512 x 512 layer from L2 is latency bound, so the one-launch path runs
// only when every layer is at most kExpqFusedMaxWidth = 128 wide.  At that width it takes 38 us
// from 1 to 256 rows (a workgroup per row) against 58, 66 and 79 us layered, so
// kExpqFusedMaxRows = 256, the most that was measured.  The EXPQ_ACT tuning key, read at
// creation, forces a path for such measurements: 1 layered, 2 one launch up to
// kExpqKernelMaxWidth at any row count.
//
// Generated noise: philox_normals under kExpqNoiseTag, element e = (row N + n) act_dim + d,
// counter index e / 4.  The uniform of a row is the first word of one more Philox call under the
// same tag at counter index ceil(rows N act_dim / 4) + row (past the noise's last counter), as
// (x >> 8) 2^-24 in [0, 1).
//
// A section of d4pg.hip kept in a file of its own: included there once, inside its anonymous
// namespace, after crr_kernels.h.  Not a stand-alone header.

// The fused kernel is compiled without packed f32 arithmetic, as the kernels of bc.hip and
// mlp_model.hip are (see there): a call must repeat bit for bit.
#ifdef __HIP_DEVICE_COMPILE__
#define ACME_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define ACME_NO_PK_F32
#endif

constexpr int kExpqFusedMaxWidth = ACME_EXPQ_FUSED_MAX_WIDTH;
constexpr int kExpqFusedMaxRows = ACME_EXPQ_FUSED_MAX_ROWS;
constexpr int kExpqKernelMaxWidth = 512;  // what the kernel's LDS is sized for (EXPQ_ACT = 2)
constexpr int kExpqTile = 16;  // critic rows of an MFMA tile

// Row stride of a tile's LDS buffer (mlp_model.hip's rule): stride % 64 == 4 spreads the 16 rows
// x 4 columns an MFMA row operand reads over all 64 banks.
constexpr int expq_stride(int width) { return ((width + 63) & ~63) + 4; }

// One network's tensors as the kernels read them.
struct ExpqNet {
  const float *w1, *b1, *scale, *offset;
  const float* w[ACME_D4PG_MAX_LAYERS];
  const float* b[ACME_D4PG_MAX_LAYERS];
  const float *ow, *ob;
  int nl, sizes[ACME_D4PG_MAX_LAYERS];
};

// Where the selection writes; everything but `action` is optional.
struct ExpqOut {
  float *action, *sampled, *q, *probs, *noise_out;
  int32_t* index;
};

// The fused kernel's LDS, in floats: two vectors of the policy's ping-pong, the k-group
// partials, z_obs, the sampled actions, (mean[16], sd[16], q[64], red[4] ...), two tiles.
struct ExpqLds {
  int vec, part, zobs, acts, misc, tile, total;
};
__host__ __device__ __forceinline__ ExpqLds expq_lds(int vw, int ld) {
  ExpqLds L;
  L.vec = 0;
  L.part = 2 * vw;
  L.zobs = L.part + 256;
  L.acts = L.zobs + vw;
  L.misc = L.acts + ACME_MPO_MAX_SAMPLES * ACME_D4PG_MAX_ACT;
  L.tile = L.misc + 128;
  L.total = L.tile + 2 * kExpqTile * ld;
  return L;
}

struct ExpqFusedArgs {
  const float* obs;  // [rows][od]
  int rows, od, A, N, K, categorical;  // K atoms
  ExpqNet pol, cri;
  const float *sw, *sb;  // the Gaussian head's scale layer
  const float* values;   // [K]
  float scale_mul, min_scale, eps, beta;
  uint64_t seed, step;
  const float *noise, *uniform;  // [rows][N][A], [rows], or null: generated
  uint32_t ubase;                // counter index of row 0's uniform
  int vw, ld;                    // LDS vector width, tile stride
  ExpqOut out;
};

// eps of element e: given, or generated.
__device__ __forceinline__ float expq_eps(const float* noise, uint64_t seed, uint64_t step,
                                          uint32_t e) {
  if (noise) return noise[e];
  float z[4];
  philox_normals(seed, step, e >> 2, z, kExpqNoiseTag);
  const uint32_t k = e & 3u;
  return k == 0 ? z[0] : k == 1 ? z[1] : k == 2 ? z[2] : z[3];
}

__device__ __forceinline__ float expq_uniform(const float* uniform, uint64_t seed, uint64_t step,
                                              uint32_t ubase, int row) {
  if (uniform) return uniform[row];
  const u32x4 c = {ubase + (uint32_t)row, (uint32_t)step, (uint32_t)(step >> 32), kExpqNoiseTag};
  const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (float)(r.x >> 8) * 0x1p-24f;
}

// q of one categorical row (lane = atom): the mean of softmax(logits) over the support.
__device__ __forceinline__ float expq_head_mean(float logit, float vi, bool on) {
  const RowSoftmax t = row_softmax(on ? logit : -INFINITY, on);
  return wave_sum(on ? t.p * vi : 0.f);
}

// The selection of one observation on one wave, lane n holding q_n: p = softmax(q / beta), the
// running sum of p in lane order, and the number of its entries <= u, clamped to N - 1.
__device__ __forceinline__ int expq_select(float qn, int N, float beta, float u, int lane,
                                           float& p) {
  const bool on = lane < N;
  const float x = on ? qn / beta : -INFINITY;
  const float m = wave_max(x);
  const float e = on ? expf(x - m) : 0.f;
  const float s = wave_sum(e);
  p = e / s;
  float c = 0.f, mine = 0.f;
  for (int n = 0; n < N; ++n) {  // in sample order
    c += __shfl(p, n, 64);
    if (lane == n) mine = c;
  }
  const int below = (int)__popcll(__ballot(on && mine <= u));
  return min(below, N - 1);
}

// The outputs of observation `row` from wave 0's lanes: q / probs of lane n < N, the chosen
// action from `acts` ([N][A], LDS or global).
__device__ __forceinline__ void expq_write(const ExpqOut& o, int row, int N, int A, int lane,
                                           float qn, float p, int idx, const float* acts) {
  if (lane < N) {
    if (o.q) o.q[(size_t)row * N + lane] = qn;
    if (o.probs) o.probs[(size_t)row * N + lane] = p;
  }
  if (lane < A) o.action[(size_t)row * A + lane] = acts[idx * A + lane];
  if (lane == 0 && o.index) o.index[row] = idx;
}

// ------------------------------------------------------------------ the one-launch kernel

// y[n] = act(x . W[:, n] + b[n]), n < N, for one row x [K] in LDS, on all 256 threads: thread t
// owns column c = t % CP of a pass of CP columns (CP = N rounded up to a power of two, at most
// 256) and k-group g = t / CP of G = 256 / CP; the G partials are summed in group order through
// `part`.  y is not x; the caller's data in y is complete when this returns.
__device__ ACME_NO_PK_F32 __forceinline__ void expq_matvec(const float* x, int K,
                                                            const float* __restrict__ w,
                                                            const float* __restrict__ b, int N,
                                                            int act, float* part, float* y, int t) {
  int CP = 1;
  while (CP < N && CP < 256) CP *= 2;
  const int G = 256 / CP, c = t & (CP - 1), g = t / CP;
  for (int n0 = 0; n0 < N; n0 += CP) {
    const int n = n0 + c;
    const bool on = n < N;
    const float* __restrict__ wcol = w + (on ? n : N - 1);
    float acc = 0.f;
#pragma unroll 8
    for (int k = g; k < K; k += G) acc = fmaf(x[k], wcol[(size_t)k * N], acc);
    part[t] = acc;
    __syncthreads();
    if (g == 0 && on) {
      float s = part[c];
      for (int q = 1; q < G; ++q) s += part[q * CP + c];
      y[n] = act_fwd(act, s + b[n]);
    }
    __syncthreads();
  }
}

// Sum of one value per thread over the block, fixed order; every thread gets it.
__device__ ACME_NO_PK_F32 __forceinline__ float expq_block_sum(float v, float* red, int t) {
  v = wave_sum(v);
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// z <- tanh(LayerNorm(z)) in place (tf.nn.moments: mean, then the mean of squared deviations),
// z [H] in LDS, on the whole block (thread i = t of 256, sums through `red`) or on one wave
// (i = lane of 64).
template <bool kBlock>
__device__ ACME_NO_PK_F32 __forceinline__ void expq_ln_tanh(float* z, int H,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ offset,
                                                             float eps, int i, float* red) {
  constexpr int nthr = kBlock ? 256 : 64;
  const float invH = 1.f / (float)H;
  float s = 0.f;
  for (int j = i; j < H; j += nthr) s += z[j];
  const float mean = (kBlock ? expq_block_sum(s, red, i) : wave_sum(s)) * invH;
  float q = 0.f;
  for (int j = i; j < H; j += nthr) {
    const float dv = z[j] - mean;
    q = fmaf(dv, dv, q);
  }
  const float rs = 1.f / sqrtf((kBlock ? expq_block_sum(q, red, i) : wave_sum(q)) * invH + eps);
  for (int j = i; j < H; j += nthr) z[j] = tanhf((z[j] - mean) * rs * scale[j] + offset[j]);
}

// D = A B + C on one wave: A is 16 x 4 (lane holds A[lane % 16][lane / 16]), B is 4 x 16 (lane
// holds B[lane / 16][lane % 16]), the lane's four results are D[4 (lane / 16) + r][lane % 16].
__device__ ACME_NO_PK_F32 __forceinline__ gemm::f32x4 expq_mfma16(float a, float b,
                                                                   gemm::f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Y = act(X W + b) for a 16-row tile X [16][K] in LDS (K a multiple of 4), W [K][N] streamed
// from global with its index clamped into the tensor, a wave per 16 output columns, the column
// tiles dealt round-robin to the four waves.  Eight k steps' weights are loaded before their
// MFMAs run.
__device__ ACME_NO_PK_F32 __forceinline__ void expq_tile_layer(const float* X, int ld, int K,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ bias,
                                                                int N, int act, float* Y,
                                                                int wave, int lane) {
  using f32x4 = gemm::f32x4;
  const int lm = lane & 15, lq = lane >> 4;
  for (int nt = wave; nt * 16 < N; nt += 4) {
    const int n = nt * 16 + lm;
    const float* __restrict__ wc = w + min(n, N - 1);
    const float* xa = X + lm * ld + lq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int k0 = 0;
    for (; k0 + 32 <= K; k0 += 32) {
      float wv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) wv[u] = wc[(size_t)(k0 + 4 * u + lq) * N];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = expq_mfma16(xa[k0 + 4 * u], wv[u], acc);
    }
    for (; k0 < K; k0 += 4)
      acc = expq_mfma16(xa[k0], wc[(size_t)min(k0 + lq, K - 1) * N], acc);
    if (n < N) {
      const float bn = bias[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) Y[(4 * lq + r) * ld + n] = act_fwd(act, acc[r] + bn);
    }
  }
}

__global__ void ACME_NO_PK_F32 __launch_bounds__(256)
    expq_act_fused_kernel(const ExpqFusedArgs a) {
  constexpr int AM = ACME_D4PG_MAX_ACT;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, row = blockIdx.x;
  const int od = a.od, A = a.A, N = a.N, ld = a.ld;
  const ExpqLds L = expq_lds(a.vw, ld);
  float* v0 = lds + L.vec;
  float* v1 = v0 + a.vw;
  float* part = lds + L.part;
  float* zobs = lds + L.zobs;
  float* acts = lds + L.acts;
  float* mean = lds + L.misc;
  float* sd = mean + AM;
  float* qs = sd + AM;
  float* red = qs + ACME_MPO_MAX_SAMPLES;
  float* X0 = lds + L.tile;
  float* X1 = X0 + kExpqTile * ld;
  for (int i = t; i < 2 * kExpqTile * ld; i += 256) X0[i] = 0.f;
  for (int k = t; k < od; k += 256) v0[k] = a.obs[(size_t)row * od + k];
  __syncthreads();
  const int C0 = a.cri.sizes[0];
  // The observation's part of the critic's first layer, once for all samples.
  expq_matvec(v0, od, a.cri.w1, a.cri.b1, C0, ACT_NONE, part, zobs, t);
  // The policy: LayerNorm first layer, ELU layers, the Gaussian head.
  float* h = v1;
  float* o = v0;
  expq_matvec(v0, od, a.pol.w1, a.pol.b1, a.pol.sizes[0], ACT_NONE, part, h, t);
  expq_ln_tanh<true>(h, a.pol.sizes[0], a.pol.scale, a.pol.offset, a.eps, t, red);
  __syncthreads();
  for (int i = 1; i < a.pol.nl; ++i) {
    expq_matvec(h, a.pol.sizes[i - 1], a.pol.w[i], a.pol.b[i], a.pol.sizes[i], ACT_ELU, part, o, t);
    float* s = h;
    h = o;
    o = s;
  }
  if (wave < 2) {  // uniform per wave
    const int Hp = a.pol.sizes[a.pol.nl - 1];
    const float d = head_dot_row(h, wave == 0 ? a.pol.ow : a.sw, Hp, A, lane);
    if (lane < A) {
      if (wave == 0)
        mean[lane] = d + a.pol.ob[lane];
      else
        sd[lane] = softplusf(d + a.sb[lane]) * a.scale_mul + a.min_scale;
    }
  }
  __syncthreads();
  for (int i = t; i < N * A; i += 256) {
    const int d = i % A;
    const uint32_t e = (uint32_t)row * (uint32_t)(N * A) + (uint32_t)i;
    const float ep = expq_eps(a.noise, a.seed, a.step, e);
    const float act = mean[d] + sd[d] * ep;
    acts[i] = act;
    if (a.out.sampled) a.out.sampled[e] = act;
    if (a.out.noise_out) a.out.noise_out[e] = ep;
  }
  __syncthreads();
  // The critic, 16 samples at a time.
  const float* __restrict__ wact = a.cri.w1 + (size_t)od * C0;
  const int cL = a.cri.nl - 1;
  for (int n0 = 0; n0 < N; n0 += kExpqTile) {
    const int valid = min(kExpqTile, N - n0);
    for (int j = t; j < C0; j += 256) {
      float wa[AM];
#pragma unroll
      for (int d = 0; d < AM; ++d) wa[d] = d < A ? wact[(size_t)d * C0 + j] : 0.f;
      const float zb = zobs[j];
      for (int r = 0; r < kExpqTile; ++r) {
        float z = 0.f;
        if (r < valid) {
          z = zb;
#pragma unroll
          for (int d = 0; d < AM; ++d)
            if (d < A) z = fmaf(acts[(n0 + r) * A + d], wa[d], z);
        }
        X0[r * ld + j] = z;
      }
    }
    __syncthreads();
    for (int r = wave; r < valid; r += 4)
      expq_ln_tanh<false>(X0 + r * ld, C0, a.cri.scale, a.cri.offset, a.eps, lane, nullptr);
    __syncthreads();
    float* X = X0;
    float* Y = X1;
    for (int i = 1; i <= cL + (a.categorical ? 1 : 0); ++i) {
      const bool head = i > cL;
      expq_tile_layer(X, ld, a.cri.sizes[i - 1], head ? a.cri.ow : a.cri.w[i],
                      head ? a.cri.ob : a.cri.b[i], head ? a.K : a.cri.sizes[i],
                      head ? ACT_NONE : ACT_ELU, Y, wave, lane);
      __syncthreads();
      float* s = X;
      X = Y;
      Y = s;
    }
    // X: the logits (categorical head) or the last hidden layer (scalar head).
    for (int r = wave; r < valid; r += 4) {
      float qv;
      if (a.categorical) {
        const bool on = lane < a.K;
        qv = expq_head_mean(on ? X[r * ld + lane] : 0.f, on ? a.values[lane] : 0.f, on);
      } else {
        qv = head_dot_row(X + r * ld, a.cri.ow, a.cri.sizes[cL], 1, lane) + a.cri.ob[0];
      }
      if (lane == 0) qs[n0 + r] = qv;
    }
    __syncthreads();
  }
  if (wave == 0) {
    const float u = expq_uniform(a.uniform, a.seed, a.step, a.ubase, row);
    const float qn = lane < N ? qs[lane] : 0.f;
    float p;
    const int idx = expq_select(qn, N, a.beta, u, lane, p);
    expq_write(a.out, row, N, A, lane, qn, p, idx, acts);
  }
}

// ------------------------------------------------------------------ the layered path's kernels

// The draw for `n_obs` observations from global row r0 on: critic row i = r N + n gets
// a = mean[r] + sd[r] eps and o[r] beside it (the form of crr_sample_kernel, which also tiles).
struct ExpqSampleArgs {
  const float *mean, *sd;  // [n_obs][A]
  const float* noise;      // [rows][N][A] or null
  const float* obs;        // [n_obs][od]
  uint64_t seed, step;
  int r0, n_obs, N, A, od;
  float *act, *tiled;           // [n_obs N][A], [n_obs N][od]
  float *sampled, *noise_out;   // [rows][N][A], optional
};

__global__ void __launch_bounds__(256) expq_sample_kernel(const ExpqSampleArgs a) {
  const int M = a.n_obs * a.N;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < M) {
    const int r = i / a.N;
    const uint32_t e0 = ((uint32_t)a.r0 * (uint32_t)a.N + (uint32_t)i) * (uint32_t)a.A;
    for (int d = 0; d < a.A; ++d) {
      const float ep = expq_eps(a.noise, a.seed, a.step, e0 + d);
      const float act = a.mean[r * a.A + d] + a.sd[r * a.A + d] * ep;
      a.act[(size_t)i * a.A + d] = act;
      if (a.sampled) a.sampled[e0 + d] = act;
      if (a.noise_out) a.noise_out[e0 + d] = ep;
    }
  }
  const int total = M * a.od;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < total; j += gridDim.x * 256) {
    const int ci = j / a.od, k = j - ci * a.od;
    a.tiled[j] = a.obs[(size_t)(ci / a.N) * a.od + k];
  }
}

// One wave per observation (4 per block): q_n of its N critic rows (the categorical head's
// mean from the logits, or the scalar head from the last hidden layer), then the selection.
struct ExpqSelectArgs {
  const float* x;  // categorical: logits [n_obs N][K]; scalar: last hidden layer [n_obs N][H]
  const float *ow, *ob;  // the scalar head
  const float* values;
  const float* act;  // [n_obs N][A]
  const float* uniform;
  uint64_t seed, step;
  uint32_t ubase;
  int r0, n_obs, N, A, K, H, categorical;
  float beta;
  ExpqOut out;
};

__global__ void __launch_bounds__(256) expq_select_kernel(const ExpqSelectArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.n_obs) return;  // uniform per wave
  const bool on = a.categorical && lane < a.K;
  const float vi = on ? a.values[lane] : 0.f;
  float qn = 0.f;
  for (int n = 0; n < a.N; ++n) {
    const size_t i = (size_t)r * a.N + n;
    float qv;
    if (a.categorical) {
      qv = expq_head_mean(on ? a.x[i * a.K + lane] : 0.f, vi, on);
    } else {
      qv = head_dot_row(a.x + i * a.H, a.ow, a.H, 1, lane) + a.ob[0];
      qv = __shfl(qv, 0, 64);
    }
    if (lane == n) qn = qv;
  }
  const int row = a.r0 + r;
  const float u = expq_uniform(a.uniform, a.seed, a.step, a.ubase, row);
  float p;
  const int idx = expq_select(qn, a.N, a.beta, u, lane, p);
  expq_write(a.out, row, a.N, a.A, lane, qn, p, idx, a.act + (size_t)r * a.N * a.A);
}
