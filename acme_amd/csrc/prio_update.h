// The replay table's one-launch priority update as a device-side body, so that it can run
// as its own kernel (replay.hip prio_update_fused_kernel) or as the leading workgroups of a
// launch already on the stream (UpdateRider below: the DQN step's write-back inside conv1's
// weight-gradient launch, gemm_p3.h launch_gemm_p3_rider; one launch and one kernel boundary
// fewer at the end of the step's critical path).
//
// Updates are partitioned over the workgroups by their ancestor at level h = nlevels - 2
// (owner = slot >> 6h, workgroup owner % G), so every update of a slot, and every touched
// node of levels 1..h, belongs to exactly one workgroup: it elects the last valid update per
// slot in LDS (largest j wins, Reverb's in-order application) and computes its leaves
// p^alpha and its nodes of levels 1..h.  The children of those nodes are loaded up front
// (one round of loads issued together right after the keys are resolved), the new values
// substituted in LDS and each node rescanned from LDS, so no store has to be read back.
// The top level (whose children many workgroups write) is rescanned by the LAST workgroup
// to finish: the level-h values are stored write-through (agent-scope atomic stores,
// drained before the workgroup counts itself) and read back by agent-scope atomic loads,
// the hand-off form that needs no L2 writeback or invalidate (cdna_hip_programming.md G16),
// so the update is one launch instead of two (round 4: a 10.2 us kernel + a 5.2 us
// one-workgroup launch for the top level).
//
// The partition decides only which workgroup computes a slot or a node, never a value: the
// result does not depend on the workgroup count G (tests/test_update_rider_gpu.py).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "detmath.h"
#include "kernels.h"
#include "rescale.h"

struct acme_replay;

namespace acme {

// The total of a wave's 64 values (the lane-63 value of the inclusive Hillis-Steele scan
// wave_scan64 of replay.hip) in every lane, with the same bits: lane 63 of the
// scan adds aligned blocks pairwise (round d: the block of d lanes ending at 63 - d to the one
// ending at 63), and so does this butterfly (each round adds the aligned neighbour block of
// the same size; f64 addition is commutative).  DPP moves for blocks of 1..8 lanes, a swizzle
// for 16 and two lane reads for 32 replace six rounds of LDS permutes.  The whole wave must
// be active (as for wave_scan64).
template <int Ctrl>
__device__ __forceinline__ double dpp_f64(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)u, Ctrl, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), Ctrl, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ double wave_total64(double x) {
  x = x + dpp_f64<0xB1>(x);   // quad_perm [1,0,3,2]: pairs
  x = x + dpp_f64<0x4E>(x);   // quad_perm [2,3,0,1]: quads
  x = x + dpp_f64<0x141>(x);  // row_half_mirror: blocks of 8
  x = x + dpp_f64<0x140>(x);  // row_mirror: blocks of 16
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const int lo = __builtin_amdgcn_ds_swizzle((int)(uint32_t)u, 0x401F);  // lane ^ 16
  const int hi = __builtin_amdgcn_ds_swizzle((int)(uint32_t)(u >> 32), 0x401F);
  x = x + __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
  const uint64_t v = __builtin_bit_cast(uint64_t, x);
  const uint32_t a0 = __builtin_amdgcn_readlane((int)(uint32_t)v, 31);
  const uint32_t a1 = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 31);
  const uint32_t b0 = __builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t b1 = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return __builtin_bit_cast(double, ((uint64_t)a1 << 32) | a0) +
         __builtin_bit_cast(double, ((uint64_t)b1 << 32) | b0);
}

constexpr int kFusedUpdateMax = 4096;
constexpr int kFusedUpdateBlocks = 256;  // update workgroups of the update's own launch
constexpr int kUpdPairs = 32;  // (level, node) pairs a workgroup prefetches; else read back
// The 512-update form (R = 2) as a rider: its update count and workgroup count.  Fewer
// workgroups hold conv1_wgrad's LDS allocation for less of the launch, and each takes more
// (level, node) pairs: at most 512 * h / G distinct ones on average, beyond kUpdPairs the
// read-back path.
constexpr int kUpdateRiderMax = 2 * 256;
constexpr int kUpdateRiderBlocks = 64;
constexpr int kUpdateRiderDefault = 1;  // ACME_V_UPDATE_RIDER when unset
struct FusedUpdateArgs {
  const uint64_t* upd_keys;
  const double* prios;
  int n;
  int64_t capacity;
  const uint64_t* keys;
  double alpha;
  double* raw_prio;
  double* level[8];
  int64_t top_nodes;  // nodes of level nlevels - 2 (the top level's entries that have children)
  int top_computed;   // readers compute the top level (computed_top_nodes > 0): not stored
  int nlevels;
  int groups = kFusedUpdateBlocks;  // update workgroups G (the rescale workgroup not counted)
  uint32_t* done;     // workgroups finished (the last one rescans the top; it resets the count)
  Gate gate;  // a learner step that was skipped writes no priority
  // job.s: the learner step's rescale, run by workgroup 0 (the update workgroups are 1..G).
  // With a step verdict (kRgStep) the update workgroups wait for it (StepGuard::vseq) and
  // write nothing when the step was skipped, for every reason the rescale decides
  // (overflow, underflow, a timed-out unroll, the sticky hold, another rank's skip).
  RescaleJob job;
  // Timing experiment (ACME_V_STAMPS=1 in the DQN learner, tools/update_stamps.py): thread 0 of
  // each workgroup stores s_memrealtime (100 MHz) at its phase boundaries, 8 slots per
  // workgroup: entry, keys resolved (workgroup 0: rescale done), node list, verdict, leaves,
  // levels, exit.
  uint64_t* stamps = nullptr;
};
// Waits (bounded) for the verdict with sequence number seq; true when that step is skipped
// (or the wait timed out: no priority is written, and the timeout is counted in
// g->vtimeout, which the host reads: acme_dqn_verdict_timeouts).  Workgroup 0 of the same
// launch publishes it and was dispatched first, so it is resident or done.
// `first`: thread 0's load of g->vseq issued earlier (its latency overlapped the caller's LDS
// work); polled again only when it did not yet hold this step's verdict.
__device__ __forceinline__ bool wait_verdict_skip(StepGuard* g, uint32_t seq, uint32_t first) {
  __shared__ uint32_t s_v;
  if (threadIdx.x == 0) {
    uint32_t v = first;
    for (int it = 0; it < (1 << 22) && (v >> 1) != (seq & 0x7fffffffu); ++it) {
      __builtin_amdgcn_s_sleep(2);
      v = __hip_atomic_load(&g->vseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const bool got = (v >> 1) == (seq & 0x7fffffffu);
    if (!got) atomicAdd(&g->vtimeout, 1u);
    s_v = got ? (v & 1u) : 1u;
  }
  __syncthreads();
  return s_v != 0u;
}
// A workgroup barrier that orders LDS only: outstanding global loads stay in flight across it
// (__syncthreads also waits for every vector memory operation of the wave).
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// A level-h value other workgroups' top rescan reads: write-through.
__device__ __forceinline__ void store_shared_level(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The body's LDS (carved from the pointer it is given, 16-byte aligned): the children rows,
// the update list, the node list and four counters.
template <int R>
struct UpdLds {
  static constexpr int kCh = 0;                                // double [kUpdPairs][64]
  static constexpr int kSlot = kCh + kUpdPairs * 64 * 8;       // int64 [R * 256]
  static constexpr int kNode = kSlot + R * 256 * 8;            // int64 [kUpdPairs]
  static constexpr int kNk = kNode + kUpdPairs * 8;            // int64 [kUpdPairs]
  static constexpr int kVal = kNk + kUpdPairs * 8;             // double [kUpdPairs]
  static constexpr int kLvl = kVal + kUpdPairs * 8;            // int [kUpdPairs]
  static constexpr int kCnt = kLvl + kUpdPairs * 4;            // int [4]: len, np, ovf, last
  static constexpr int kBytes = kCnt + 16;
};

// R: updates per thread the launch holds (n <= 256 R).  The small form (R = 2, up to 512
// updates: a DQN batch) takes 21 KB of LDS and few registers, so its workgroups fit beside
// the next step's target forward (gemm_p3c12_kernel, 117 KB of LDS per CU), which the
// early start runs at the same time on the side stream; at R = 16 (49 KB, 200 VGPRs) they
// waited for its blocks to retire (24 us in the two-stream trace against 12 us alone,
// profiles/r06/schedule/).
// wg: this workgroup's index among the launch's update roles, in dispatch order (0 is the
// rescale workgroup when a.job.s is set; then the G = a.groups update workgroups); every
// thread of a 256-thread workgroup calls, with UpdLds<R>::kBytes of LDS at `lds`.
template <int R>
__device__ __forceinline__ void prio_update_body(const FusedUpdateArgs& a, uint8_t* lds,
                                                 const int wg, const int G) {
  static_assert(R * 256 <= kFusedUpdateMax, "update capacity");
  using L = UpdLds<R>;
  double(*s_ch)[64] = reinterpret_cast<double(*)[64]>(lds + L::kCh);  // children of each prefetched node
  int64_t* s_slot = reinterpret_cast<int64_t*>(lds + L::kSlot);
  int64_t* s_node = reinterpret_cast<int64_t*>(lds + L::kNode);
  int64_t* s_nk = reinterpret_cast<int64_t*>(lds + L::kNk);  // node << 3 | level: one LDS read per match test
  double* s_val = reinterpret_cast<double*>(lds + L::kVal);
  int* s_lvl = reinterpret_cast<int*>(lds + L::kLvl);
  int* s_cnt = reinterpret_cast<int*>(lds + L::kCnt);
  int &s_len = s_cnt[0], &s_np = s_cnt[1], &s_ovf = s_cnt[2], &s_last = s_cnt[3];
  const int first = a.job.s ? 1 : 0;
  auto stamp = [&](int ph) {
    if (a.stamps && threadIdx.x == 0)
      a.stamps[8 * (int64_t)wg + ph] = __builtin_amdgcn_s_memrealtime();
  };
  stamp(0);
  if (a.job.s && wg == 0) {
    rescale_block(a.job);
    stamp(1);
    return;
  }
  const bool verdict = a.job.s && a.job.rg.g && a.job.rg.mode == kRgStep;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int bid = wg - first;
  const int h = a.nlevels >= 2 ? a.nlevels - 2 : 0;
  bool skip = !verdict && gate_skip(a.gate);
  if (tid == 0) s_len = 0;
  __syncthreads();
  // Round 1: every update's key and priority (all workgroups read all of them; L2-resident
  // after the first), its slot and owner; this workgroup's updates join the list in atomic
  // order, and the thread that read an update keeps it (key, priority, list entry) in
  // registers.  Its stale-key check shares round 2 with the children rows, and its leaf
  // p^alpha is computed while those loads are in flight (round 6: three dependent rounds of
  // global loads became two, and the f64 power left the critical path).
  uint64_t kv[R];
  double pr[R];
  int64_t sl[R];
  int my_e[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    my_e[i] = -1;
    kv[i] = 0;
    pr[i] = 0.0;
    sl[i] = 0;
  }
  if (!skip) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i * nt >= a.n) break;  // workgroup-uniform
      const int j = tid + i * nt;
      const int jc = j < a.n ? j : a.n - 1;
      kv[i] = a.upd_keys[jc];
      pr[i] = a.prios[jc];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i * nt >= a.n) break;
      const int j = tid + i * nt;
      const int64_t slot = (int64_t)(kv[i] % (uint64_t)a.capacity);
      // (G is a launch argument: a 32-bit unsigned remainder, not a 64-bit division.  The
      // owner only has to be the same in every workgroup.)
      if (j < a.n && (int)((uint32_t)(slot >> (6 * h)) % (uint32_t)G) == bid) {
        const int e = atomicAdd(&s_len, 1);
        s_slot[e] = slot;
        my_e[i] = e;
        sl[i] = slot;
      }
    }
  }
  __syncthreads();
  stamp(1);
  const int len = s_len;
  if (len > 0) {
    // The distinct nodes of levels 1..h this workgroup recomputes: a thread per (level,
    // update) keeps the node if no earlier update of the list has the same ancestor at that
    // level (a serial scan by one thread took up to 7 us on the workgroup with the most
    // updates, profiles/r05/update_stamps/).  The list's order is the threads' (atomic slot
    // order); every use below matches nodes by (level, node), so the result does not depend
    // on it.  A node whose updates all turn out stale is rescanned from unchanged children:
    // the same value it holds.
    if (tid == 0) {
      s_np = 0;
      s_ovf = 0;
    }
    __syncthreads();
    for (int idx = tid; idx < h * len; idx += nt) {
      const int l = 1 + idx / len, e = idx - (l - 1) * len;
      const int64_t node = s_slot[e] >> (6 * l);
      bool first = true;
      for (int f = 0; f < e && first; ++f) first = (s_slot[f] >> (6 * l)) != node;
      if (!first) continue;
      const int q = atomicAdd(&s_np, 1);
      if (q < kUpdPairs) {
        s_lvl[q] = l;
        s_node[q] = node;
        s_nk[q] = (node << 3) | l;
      } else {
        s_ovf = 1;
      }
    }
    __syncthreads();
    if (tid == 0 && s_np > kUpdPairs) s_np = kUpdPairs;  // (with s_ovf: the read-back path)
    __syncthreads();
    stamp(2);
    const int np = s_np;
    const bool pre = !s_ovf;
    // Round 2, one batch of loads: the stored key of each of this thread's updates (the stale
    // check) and each node's 64 children (a wave per node); the leaves computed meanwhile.
    // (Loops over a thread's updates stop at the workgroup-uniform count, so nothing is
    // evaluated for the unused register slots: the f64 power below for all 16 measured
    // 17 us.)
    uint64_t kt[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i * nt >= a.n) break;
      kt[i] = my_e[i] >= 0 ? a.keys[sl[i]] : 0;
    }
    if (pre) {
      for (int q = wave; q < np; q += nw)
        s_ch[q][lane] = a.level[s_lvl[q] - 1][s_node[q] * 64 + lane];
    }
    double leafv[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i * nt >= a.n) break;
      leafv[i] = 0.0;
      if (my_e[i] >= 0) leafv[i] = det_pow_priority(pr[i], a.alpha);
    }
    // Each entry repacked in place as slot << 13 | valid << 12 | j (the node list is built,
    // so s_slot's plain form is no longer read): the election below reads one word per entry.
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i * nt >= a.n) break;
      if (my_e[i] >= 0)  // valid: the key still lives in its slot (evicted since sampled: ignored)
        s_slot[my_e[i]] = (sl[i] << 13) | ((kt[i] == kv[i] ? 1 : 0) << 12) | (tid + i * nt);
    }
    __syncthreads();
    stamp(4);
    // The verdict's first poll now (thread 0), landing while the LDS work below runs: the
    // barriers below order LDS only, so they do not wait for it.
    uint32_t vfirst = 0;
    if (verdict && tid == 0)
      vfirst = __hip_atomic_load(&a.job.rg.g->vseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // Everything but the stores before the verdict: the last valid update of each slot wins
    // (substituted into its level-1 node's children) and, on the prefetched path, every
    // node's new value rescanned level by level in LDS.
    bool winv[R];
#pragma unroll
    for (int i = 0; i < R; ++i) winv[i] = false;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i * nt >= a.n) break;
      const int e = my_e[i];
      bool win = e >= 0 && kt[i] == kv[i];
      const int j = tid + i * nt;
      const int64_t me = (sl[i] << 1) | 1;  // same slot, valid
#pragma unroll 4
      for (int f = 0; f < len; ++f) {
        const int64_t x = s_slot[f];
        if ((x >> 12) == me && (int)(x & 4095) > j) win = false;
      }
      winv[i] = win;
    }
    // (The children rows were filled by wave q % nw before the barrier above, so the
    // substitutions below by any wave follow them: ADVICE r5's race.)
    if (pre) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        if (i * nt >= a.n) break;
        if (!winv[i]) continue;
        const int64_t k1 = ((sl[i] >> 6) << 3) | 1;
#pragma unroll 4
        for (int q = 0; q < np; ++q)
          if (s_nk[q] == k1) s_ch[q][sl[i] & 63] = leafv[i];
      }
    }
    lds_barrier();
    if (pre) {
      for (int l = 1; l <= h; ++l) {
        for (int q = wave; q < np; q += nw) {
          if (s_lvl[q] != l) continue;
          const double v = wave_total64(s_ch[q][lane]);
          if (lane == 63) s_val[q] = v;
        }
        lds_barrier();
        if (tid < np && s_lvl[tid] == l) {  // into the parent's children
          const int64_t kp = ((s_node[tid] >> 6) << 3) | (l + 1);
#pragma unroll 4
          for (int q = 0; q < np; ++q)
            if (s_nk[q] == kp) s_ch[q][s_node[tid] & 63] = s_val[tid];
        }
        lds_barrier();
      }
    }
    // The step's verdict (published by workgroup 0's rescale while this workgroup resolved
    // its keys, loaded and computed), before the first store.
    stamp(7);
    if (verdict) skip = wait_verdict_skip(a.job.rg.g, a.job.rg.seq, vfirst);
    stamp(3);
    if (!skip) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        if (i * nt >= a.n) break;
        if (!winv[i]) continue;
        a.raw_prio[sl[i]] = pr[i];
        if (h == 0 && !a.top_computed) store_shared_level(a.level[0] + sl[i], leafv[i]);
        else a.level[0][sl[i]] = leafv[i];
      }
      if (pre) {
        for (int q = tid; q < np; q += nt) {
          const int l = s_lvl[q];
          if (l == h && !a.top_computed) store_shared_level(a.level[l] + s_node[q], s_val[q]);
          else a.level[l][s_node[q]] = s_val[q];
        }
      } else {
        __syncthreads();
        for (int l = 1; l <= h; ++l) {  // read back what this workgroup stored (levels below are its own)
          for (int e = wave; e < len; e += nw) {
            const int64_t node = (s_slot[e] >> 13) >> (6 * l);
            const double v = wave_total64(a.level[l - 1][node * 64 + lane]);
            if (lane == 63) {
              if (l == h && !a.top_computed) store_shared_level(a.level[l] + node, v);
              else a.level[l][node] = v;
            }
          }
          __syncthreads();
        }
      }
      stamp(5);
    }
  }
  stamp(6);
  if (a.nlevels < 2 || a.top_computed) return;  // readers compute the top (TreeView)
  // Count this workgroup finished once its level-h stores are released at agent scope (every
  // thread's own release fence, then the workgroup barrier, then a release increment), and
  // the last one acquires them (the increment's acquire side and an agent-scope acquire fence
  // in every thread) before it rescans the top level (a waitcnt is no fence).
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (tid == 0)
    s_last = __hip_atomic_fetch_add(a.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
             (uint32_t)(G - 1);
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int top = a.nlevels - 1;
  for (int64_t node = wave; node < a.top_nodes; node += nw) {
    const double c = __hip_atomic_load(a.level[top - 1] + node * 64 + lane, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
    const double v = wave_total64(c);
    if (lane == 63) a.level[top][node] = v;
  }
  if (tid == 0) __hip_atomic_store(a.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The 512-update form as the leading workgroups of a 256-thread launch (gemm_p3.h
// gemm_p3r_kernel): blocks [0, blocks(a)) of the grid in dispatch order, the rescale
// workgroup first (wait_verdict_skip's dispatched-first assumption as in the update's own
// launch), in the host launch's dynamic LDS.  The count is padded to a multiple of 8 (the
// surplus blocks return at once), so the launch's other blocks keep their XCDs.
struct UpdateRider {
  using Args = FusedUpdateArgs;
  static constexpr int kThreads = 256;
  static constexpr int kLdsBytes = UpdLds<kUpdateRiderMax / 256>::kBytes;
  static __host__ __device__ __forceinline__ int blocks(const Args& a) {
    return (a.groups + (a.job.s ? 1 : 0) + 7) & ~7;
  }
  static __device__ __forceinline__ void run(const Args& a, uint8_t* lds, int wg) {
    if (wg < a.groups + (a.job.s ? 1 : 0))
      prio_update_body<kUpdateRiderMax / 256>(a, lds, wg, a.groups);
  }
};

// Host side of the table's one-launch update, in two halves (replay.hip).  prepare: the
// table's lock, the stream's order after committed inserts, and the launch's arguments for
// n in [1, kFusedUpdateMax] updates over `groups` workgroups; on ACME_OK the table stays
// locked until replay_update_release (so no commit slips between the stream's order and the
// launch).  The caller launches on `st` between the two.
int replay_update_prepare(acme_replay* r, const uint64_t* keys, const double* prios, int64_t n,
                          const Gate& gate, hipStream_t st, const RescaleJob* job, int groups,
                          FusedUpdateArgs* out);
void replay_update_release(acme_replay* r);

}  // namespace acme
