// Image-resident implicit-GEMM convolution on f16 operand planes (gfx950).
//
// gemm_p3.h reads a convolution's A operand as im2col rows: every input pixel is fetched
// KH*KW/S^2 times (4x for conv1 / conv2, 9x for conv3) and every fetch goes global -> VGPR
// -> LDS, so the A
// tile's LDS stores (ds_write_b128 ~79 B/clk/CU, MI355X_MICROARCH.md §LDS) or its TA
// issue bound the convolutions (15-34% of the plane-engine ceiling).  Here a block owns
// FPB whole frames: their input image, every plane, is loaded into LDS ONCE (each HBM
// byte once, each LDS byte stored once), and the MFMA A fragments are read from it
// directly, with the tap offset applied per lane (padding taps read a zero unit).  Only
// the weight panel B (K x BN) streams through a two-stage register-staged LDS ring.
//
// A geometry GI (gemm_p3i_geom.h) says where each 16-B unit (8 consecutive k of one GEMM
// row) lives, and which of the plane's 16 zero units a padding tap reads.
//
// A stage is BK k (a multiple of 32): one barrier and one ring hand-off per BK / 16 k16
// steps.  Within a stage the fragments are read in 32-k groups, each group's reads fenced
// before its MFMAs, so the register count does not grow with BK and the k order -- hence
// every sum -- is that of BK = 32.  The last stage is shorter when K % BK != 0.
// Ring, fill and k loop are this kernel's own (group-fenced reads, short last stage); gemm_p3s.h
// and gemm_p3c12.h hold four more: DESIGN 4.1 "five k loops" has how they differ and why.
#pragma once

#include "gemm_p3.h"
#include "gemm_p3i_geom.h"

namespace acme {
namespace gemm {

template <class GI, int FPB, int BN, int WM, int WN, int MT, int BK_, class P>
struct P3ICfg {
  static constexpr int BK = BK_;            // k per stage (one barrier, one ring hand-off)
  static constexpr int GK = 32, KS = 2;     // k per fragment group, its k16 steps
  static constexpr int NG = BK / GK;        // groups per stage
  static_assert(BK % GK == 0 && NG >= 1, "a stage is whole 32-k groups");
  static constexpr int NW = WM * WN, NT = 64 * NW;
  static constexpr int TN = BN / WN, NTL = TN / 32;
  static constexpr int BM = WM * 32 * MT;
  static_assert(BM >= FPB * GI::OPIX, "the block's waves must cover its frames' rows");
  static_assert(TN % 32 == 0, "wave panel of whole 32-column MFMA tiles");
  using Core = P3Core<BM, BN, WM, WN, GK, P>;
  using PB = typename Core::PB;
  static constexpr int NPA = P::A_PLANES;
  static constexpr int ZERO = img_zero_base(FPB * GI::IMG);  // the plane's zero area
  static constexpr int PLANE = ZERO + kImgZeroBytes;
  static constexpr int IMG = NPA * PLANE;
  static constexpr int STAGE_B = NG * PB::BYTES;     // a group's B panel is one PlanP3 tile
  static constexpr int B_UNITS = NG * PB::UNITS;     // 16-B units of a stage's B, per plane
  static constexpr int B_PER = (B_UNITS + NT - 1) / NT;
  static constexpr int MAIN = IMG + 2 * STAGE_B;
  static constexpr int LDS = MAIN > Core::EPI_BYTES ? MAIN : Core::EPI_BYTES;
};

template <class GI, int FPB, int BN, int WM, int WN, int MT, int BK_, class P>
__global__ void __launch_bounds__(64 * WM * WN) gemm_p3i_kernel(const P p_in, int frames) {
  using Cfg = P3ICfg<GI, FPB, BN, WM, WN, MT, BK_, P>;
  using C = typename Cfg::Core;
  using PB = typename Cfg::PB;
  constexpr int NT = Cfg::NT, NTL = Cfg::NTL, TN = Cfg::TN, BK = Cfg::BK, KS = Cfg::KS;
  constexpr int GK = Cfg::GK, NG = Cfg::NG, B_PER = Cfg::B_PER, B_UNITS = Cfg::B_UNITS;
  constexpr int PLANE = Cfg::PLANE, NPA = Cfg::NPA;
  constexpr int NPB = kPlanes;
  static_assert(P::A_MODE == KCONTIG && (NPA == 1 || NPA == kPlanes) && P::B_PLANES == NPB,
                "k-contiguous A (one or two planes), two-plane B");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  // Phase stamps (timing experiment, as gemm_p3ws_kernel's): entry, after the image fill's
  // barrier, after the k loop, exit.
  uint64_t st_rt0 = 0, st_t0 = 0, st_t1 = 0, st_t2 = 0;
  bool stamp = false;
  if constexpr (HasStamps<P>::value) {
    stamp = p_in.stamps != nullptr && tid == 0;
    if (stamp) {
      st_rt0 = __builtin_amdgcn_s_memrealtime();
      st_t0 = __builtin_amdgcn_s_memtime();
    }
  }
  const int f0 = blockIdx.x * FPB;
  const int nf = frames - f0 < FPB ? frames - f0 : FPB;
  const int rows = nf * GI::OPIX;
  const int m0 = f0 * GI::OPIX;
  P p = p_in;
  p.M = m0 + rows < p_in.M ? m0 + rows : p_in.M;  // the epilogue writes this block's rows only
  const int nk = (p.K + BK - 1) / BK;  // the last stage may be short (whole groups)

  // ---- B: the weight panel, register-staged double buffer.
  // Unit u of a stage is unit u % PB::UNITS of group u / PB::UNITS.
  typename P::BRow brow[B_PER];
#pragma unroll
  for (int i = 0; i < B_PER; ++i) {
    const int u = tid + i * NT;
    brow[i] = p.b_row(u < B_UNITS ? PB::row_of(u % PB::UNITS) : 0);
  }
  __amdgpu_buffer_rsrc_t srcB[NPB];
#pragma unroll
  for (int pl = 0; pl < NPB; ++pl) srcB[pl] = plane_rsrc(p.b_src, pl);
  // Two register sets (round 5: a third, loads two iterations ahead, measured slower on the
  // step: 0.4949 -> 0.5011 ms).
  constexpr int RS = 2;
  u32x4 rb[RS][B_PER][NPB];
  auto fetch_b = [&](auto S, int k0) {
    constexpr int set = decltype(S)::value;
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int u = tid + i * NT;
      const int g = u / PB::UNITS, kk = PB::kk_of(u % PB::UNITS);
      const int kg = k0 + g * GK;
      const uint32_t off =
          ((B_UNITS % NT == 0 || u < B_UNITS) && kg + kk < p.K) ? p.b_off(brow[i], kg, kk) : kOOB;
#pragma unroll
      for (int pl = 0; pl < NPB; ++pl)
        rb[set][i][pl] =
            __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(srcB[pl], off, 0, 0));
    }
  };
  auto stash_b = [&](auto S, int buf) {
    constexpr int set = decltype(S)::value;
    uint8_t* sb = smem + Cfg::IMG + buf * Cfg::STAGE_B;
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int u = tid + i * NT;
      if (B_UNITS % NT != 0 && u >= B_UNITS) continue;
      const int off = (u / PB::UNITS) * PB::BYTES + PB::offset(u % PB::UNITS);
#pragma unroll
      for (int pl = 0; pl < NPB; ++pl)
        *reinterpret_cast<u32x4*>(sb + pl * PB::PLANE + off) = rb[set][i][pl];
    }
  };

  fetch_b(Set0{}, 0);
  fetch_b(Set1{}, BK);

  // ---- A: the block's frames, each unit of each plane loaded and stored once.
  constexpr int UB = 16;  // bytes per unit
  using UT = u32x4;
  if constexpr (AU8<P>::value) {
    // The uint8 frames themselves: a 16-B load holds two f16 units (units 2u, 2u + 1 of the
    // same image row), widened exactly; frames from a_src, or from a_src2 past a_split.
    static_assert(FPB == 1 && NPA == 1 && GI::UNITS % 2 == 0, "uint8 frames: one per block");
    constexpr int U8U = GI::UNITS / 2;
    constexpr int PER = (U8U + NT - 1) / NT;
    const bool second = f0 >= p.a_split;
    const __amdgpu_buffer_rsrc_t sa = plane_rsrc(second ? p.a_src2 : p.a_src, 0);
    const int fl = second ? f0 - p.a_split : f0;
    u32x4 v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      const uint32_t off = u < U8U ? (uint32_t)(((int64_t)fl * U8U + u) * 16) : kOOB;
      v[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(sa, off, 0, 0));
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      if (U8U % NT == 0 || u < U8U) {
        *reinterpret_cast<u32x4*>(smem + GI::fill(0, 2 * u)) = f16x8_of_bytes(v[j][0], v[j][1]);
        *reinterpret_cast<u32x4*>(smem + GI::fill(0, 2 * u + 1)) = f16x8_of_bytes(v[j][2], v[j][3]);
      }
    }
    if (tid < 16) *reinterpret_cast<u32x4*>(smem + Cfg::ZERO + 16 * tid) = zero_u4();
  } else {
    constexpr int UNITS = FPB * GI::UNITS;
    constexpr int PER = (UNITS + NT - 1) / NT;
    __amdgpu_buffer_rsrc_t srcA[NPA];
#pragma unroll
    for (int pl = 0; pl < NPA; ++pl) srcA[pl] = plane_rsrc(p.a_src, pl);
    UT v[PER][NPA];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      const int f = u / GI::UNITS;
      const bool ok = u < UNITS && f < nf;
      // Units are HBM-linear over the block's frames: byte (f0 * UNITS + u) * UB.
      const uint32_t off = ok ? (uint32_t)(((int64_t)f0 * GI::UNITS + u) * UB) : kOOB;
#pragma unroll
      for (int pl = 0; pl < NPA; ++pl) {
        v[j][pl] = __builtin_bit_cast(UT, __builtin_amdgcn_raw_buffer_load_b128(srcA[pl], off, 0, 0));
      }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      if (UNITS % NT == 0 || u < UNITS) {
        const int f = u / GI::UNITS;
        const int a = GI::fill(f, u - f * GI::UNITS);
#pragma unroll
        for (int pl = 0; pl < NPA; ++pl) *reinterpret_cast<UT*>(smem + pl * PLANE + a) = v[j][pl];
      }
    }
    if (tid < 16 * NPA)
      *reinterpret_cast<u32x4*>(smem + (tid >> 4) * PLANE + Cfg::ZERO + 16 * (tid & 15)) = zero_u4();
  }
  stash_b(Set0{}, 0);

  // ---- This lane's GEMM rows (one per 32-row block of the wave's tile).
  typename GI::Lane ln[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int lr = wm * 32 * MT + i * 32 + (lane & 31);
    const int f = lr / GI::OPIX;
    ln[i] = GI::lane(f, lr - f * GI::OPIX, lr < rows);
  }
  __syncthreads();
  if constexpr (HasStamps<P>::value)
    if (stamp) st_t1 = __builtin_amdgcn_s_memtime();

  typename C::Acc acc;
  acc.zero();
  // The epilogue's constants, loaded now (their latency hides under the k loop).
  typename EpiPre<P>::type pre{};
  if constexpr (EpiPre<P>::has) pre = p.pre(wn * TN + C::epi_col(lane));

  // One 32-k group: its B panel at sb.
  auto group = [&](int k0, const uint8_t* sb) {
    typename GI::Stage sg[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) sg[i] = GI::stage(ln[i], k0, Cfg::ZERO);
    // Every fragment of the group read first, then the MFMAs (fenced): one LDS latency per
    // group instead of one per k16 step (the scheduler otherwise sinks each read to its first
    // use; round 5: step 0.4969 -> 0.4949 ms with the fences here and in iter below).
    f16x8 fb[KS][NTL][NPB], fa[KS][MT][NPA];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int j = 0; j < NTL; ++j)
#pragma unroll
        for (int pl = 0; pl < NPB; ++pl) fb[s][j][pl] = PB::frag(sb, pl, wn * TN + j * 32, s, lane);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int a = GI::unit(sg[i], ln[i], k0, s, lane >> 5);
#pragma unroll
        for (int pl = 0; pl < NPA; ++pl)
          fa[s][i][pl] = *reinterpret_cast<const f16x8*>(smem + pl * PLANE + a);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NTL; ++j) acc.terms(i, j, fa[s][i], fb[s][j]);
  };
  // One stage: its groups in k order (fewer in a short last stage; block-uniform).
  auto compute = [&](int k0, int buf) {
    const uint8_t* sb = smem + Cfg::IMG + buf * Cfg::STAGE_B;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g > 0) {
        if (k0 + g * GK >= p.K) break;
        __builtin_amdgcn_sched_barrier(0);
      }
      group(k0 + g * GK, sb + g * PB::BYTES);
    }
  };

  // Iteration kt: LDS buffer kt & 1 holds B of stage kt, register set (kt + 1) % RS holds
  // stage kt + 1 (stashed first into buffer (kt + 1) & 1: last read in iteration kt - 1,
  // before the barrier), then stage kt + RS is fetched into set kt % RS (zeros past the end).
  auto iter = [&](auto S, int kt) {
    constexpr int set = decltype(S)::value;
    using Next = std::integral_constant<int, (set + 1) % RS>;
    stash_b(Next{}, (kt + 1) & 1);
    fetch_b(S, (kt + RS) * BK);
    // The weight loads issue before the MFMAs (fenced), so they have the whole iteration
    // to land before the next iteration stores them (round 5: the scheduler had sunk them
    // to just before the barrier, and the next store waited out their latency).
    __builtin_amdgcn_sched_barrier(0);
    compute(kt * BK, kt & 1);
    __syncthreads();
  };
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    iter(Set0{}, kt);
    iter(Set1{}, kt + 1);
  }
  if (kt < nk) iter(Set0{}, kt);

  if constexpr (HasStamps<P>::value)
    if (stamp) st_t2 = __builtin_amdgcn_s_memtime();
  C::epilogue(p, smem, m0, 0, wave, wm, wn, lane, 0, acc, false, &pre);
  if constexpr (HasStamps<P>::value) {
    if (stamp) {
      uint64_t* o = p_in.stamps + 8 * (int64_t)blockIdx.x;
      o[0] = st_rt0;
      o[1] = __builtin_amdgcn_s_memrealtime();
      o[2] = st_t0;
      o[3] = st_t1;
      o[4] = st_t2;
      o[5] = __builtin_amdgcn_s_memtime();
    }
  }
}

// frames: the number of images (p.M = frames * GI::OPIX rows).
template <class GI, int FPB, int BN, int WM, int WN, int MT, int BK_, class P>
inline hipError_t launch_gemm_p3i(const P& p, int frames, hipStream_t st) {
  using Cfg = P3ICfg<GI, FPB, BN, WM, WN, MT, BK_, P>;
  static_assert(Cfg::LDS <= 160 * 1024, "image + two B stages must fit the 160-KiB LDS");
  static hipError_t attr = p3_set_lds(&gemm_p3i_kernel<GI, FPB, BN, WM, WN, MT, BK_, P>, Cfg::LDS);
  if (attr != hipSuccess) return attr;
  if (p.N > BN || p.M != frames * GI::OPIX || p.K % Cfg::GK != 0) return hipErrorInvalidValue;
  const int blocks = (frames + FPB - 1) / FPB;
  hipLaunchKernelGGL((gemm_p3i_kernel<GI, FPB, BN, WM, WN, MT, BK_, P>), dim3(blocks), dim3(Cfg::NT),
                     Cfg::LDS, st, p, frames);
  return hipGetLastError();
}

}  // namespace gemm
}  // namespace acme
