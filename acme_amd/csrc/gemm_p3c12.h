// Fused conv1 -> conv2 forward of the Nature torso, one frame per block (gfx950).
//
// conv1 writes its output x1 as two f16 planes (43 MB per launch on average) and conv2
// reads it back, im2col-duplicated, through L2 (129 MB).  Only the o_tm1 rows' x1 is ever
// needed again (conv2's weight gradient and input-gradient ReLU mask); the o_t rows of the
// online network and all target rows are consumed by conv2 alone.  Here a block computes
// conv1 for one frame from its image in LDS (gemm_p3i.h pixel pairs), its epilogue writes
// x1 straight into a second LDS image in conv2's layout (gemm_p3i_geom.h ImgGeom: swizzled
// channel chunks, the four parity classes one after the other) -- and to HBM only for
// frames below hbm_frames -- then conv2 runs on that image.  Both weight panels stream
// through register-staged two-stage rings; conv2's first two stages are fetched at kernel
// start.  LDS, one block (8 waves) per CU: the frame image with its zero area, 55.5 KB
// (after conv1, conv2's weight ring and both epilogue staging areas), and the two x1 planes
// with theirs, 62 KB, the first of which holds conv1's ring until conv1's epilogue writes
// x1: 117.5 KB.  BK1 / BK2: the two convolutions' stage depths (gemm_p3i.h: one barrier and
// one ring hand-off per stage, 32-k groups within it, the same sums at any depth).
//
// conv3 behind conv2 (round 9).  x2, conv2's output, is read again only by conv3's backward
// and only for the o_tm1 rows, so conv2's epilogue writes it the same way -- P3ConvToLds, an
// LDS image in conv3's layout laid over the x1 planes, which are dead after conv2's k loop,
// and HBM only below a frame limit -- and conv3 runs from that image in the same block:
//   * gemm_p3c12_kernel with G3: conv1 -> conv2 -> conv3 for the target forward, the same
//     117.5 KB (conv3's ring and staging reuse the frame region as conv2's do);
//   * gemm_p3c23_kernel: conv2 -> conv3 for the online forward, conv2_fwd's two frames per
//     block and 16 waves with x1 from HBM, the same 155 KB.
// Every sum keeps the separate kernels' order (32-k groups in k order, P3Core's terms), so x3,
// and x2 where it is stored, are bit-identical to conv2_fwd / conv12_fwd followed by
// conv3_fwd.  Where each region lies in each phase: gemm_p3i_geom.h C123Place / C23Place.
// conv1 and conv2 of gemm_p3c12_kernel keep own rings and k loops (step-interleaved, whole stage
// pairs), P3ImgPhase has gemm_p3i_kernel's (group-fenced): DESIGN 4.1 "five k loops".
#pragma once

#include "conv_p3.h"
#include "gemm_p3i.h"

namespace acme {
namespace gemm {

// A forward convolution's epilogue sink: the block's output frames as LDS images of the next
// layer (both planes, at the output record's write scale; gemm_p3i_geom.h sink_at) and, for
// GEMM rows below hbm_rows, the output planes in HBM.  The values are those of
// P3ConvFwd<Gfrom, NPA>::store8p, and the amax of every row is committed to the output's
// scale record, whether the row reaches HBM or not.
template <class Gfrom, class Gto, int NPA, bool U8 = false, int FPB = 1>
struct P3ConvToLds {
  using Base = conv::P3ConvFwd<Gfrom, NPA, U8>;
  static constexpr int A_MODE = Base::A_MODE, B_MODE = Base::B_MODE;
  static constexpr int A_PLANES = NPA, B_PLANES = kPlanes;
  static constexpr bool kStore8 = true;
  static constexpr bool kAmax = true;
  int M, N, K, k_chunk;
  Base base;
  uint8_t* img;  // LDS images, plane stride `plane` bytes
  int plane;
  int m0;        // the first GEMM row of the block's frame 0
  int hbm_rows;
  __device__ PScale* amax_sc() const { return base.y.sc; }
  using Pre = typename Base::Pre;
  __device__ Pre pre(int n) const { return base.pre(n); }
  __device__ float store8p(int m, int n, const conv::V8& acc, int, const Pre& q) const {
    conv::V8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = acc[j] * q.rs;
      if constexpr (NPA == 1) x = x / 255.0f;
      x += q.b[j];
      v[j] = x > 0.f ? x : 0.f;
    }
    uint32_t h[4], l[4];
    const float mx = conv::split8(v, q.w, h, l);
    int pp = m - m0, f = 0;
    if constexpr (FPB > 1) {
      f = pp / Gfrom::OPIX;
      pp -= f * Gfrom::OPIX;
    }
    const int a = sink_at<Gfrom, Gto>(f, pp, n);
    *reinterpret_cast<u32x4*>(img + a) = u32x4{h[0], h[1], h[2], h[3]};
    *reinterpret_cast<u32x4*>(img + plane + a) = u32x4{l[0], l[1], l[2], l[3]};
    if (m < hbm_rows) {
      const int64_t e = (int64_t)m * Gfrom::CO + n;
      *reinterpret_cast<uint4*>(base.y.p + e) = uint4{h[0], h[1], h[2], h[3]};
      *reinterpret_cast<uint4*>(base.y.p + base.y.stride + e) = uint4{l[0], l[1], l[2], l[3]};
    }
    return mx;
  }
};
// conv1's sink in the fused kernels: x1 as conv2's image.
template <class G1, class G2, bool U8 = false>
using P3C1ToLds = P3ConvToLds<G1, G2, 1, U8, 1>;

// One image-resident convolution inside a fused kernel of NT threads (WM x WN waves of
// 32 x 32, 64 output channels): the weight ring (one 16-B unit per owning thread per plane
// and stage, two register sets) and the k loop of gemm_p3i_kernel -- 32-k groups in k order,
// each group's fragments read before its MFMAs -- over images already in LDS.  P is the
// convolution, PQ the problem its epilogue stores through (P itself, or a P3ConvToLds).
template <class GI, int NT_, int WM, int WN, int BK_, class P, class PQ>
struct P3ImgPhase {
  static constexpr int NT = NT_, GK = 32, KS = 2, BK = BK_, NG = BK / GK, NP = kPlanes;
  static_assert(NT == 64 * WM * WN && BK % GK == 0 && NG >= 1, "whole waves, whole 32-k groups");
  static_assert(P::A_PLANES == NP && P::B_PLANES == NP, "two-plane operands");
  using C = P3Core<WM * 32, 64, WM, WN, GK, PQ>;
  using PB = typename C::PB;
  static_assert(NG * PB::UNITS <= NT, "one weight unit per thread per plane and stage");
  static constexpr int RING = 2 * NG * PB::BYTES;
  struct Ring {
    bool own;
    int g, u;
    typename P::BRow br;
    __amdgpu_buffer_rsrc_t sb[NP];
    u32x4 r[2][NP];
  };
  __device__ static __forceinline__ void init(Ring& w, const P& p, int tid) {
    w.own = tid < NG * PB::UNITS;
    w.g = tid / PB::UNITS;
    w.u = tid % PB::UNITS;
    w.br = p.b_row(w.own ? PB::row_of(w.u) : 0);
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) w.sb[pl] = plane_rsrc(p.b_src, pl);
  }
  template <int SET>
  __device__ static __forceinline__ void fetch(Ring& w, const P& p, int k0) {
    const int kg = k0 + w.g * GK;
    const uint32_t off = w.own && kg < p.K ? p.b_off(w.br, kg, PB::kk_of(w.u)) : kOOB;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
      w.r[SET][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(w.sb[pl], off, 0, 0));
  }
  template <int SET>
  __device__ static __forceinline__ void stash(const Ring& w, uint8_t* ring, int buf) {
    if (!w.own) return;
    uint8_t* s = ring + (buf * NG + w.g) * PB::BYTES + PB::offset(w.u);
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<u32x4*>(s + pl * PB::PLANE) = w.r[SET][pl];
  }
  // The k loop over `rows` GEMM rows of the block's images at img (plane stride `plane`,
  // zero area at `zero`).  On entry register set 0 holds stage 0 and set 1 stage 1; the ring
  // area must be free.  Every iteration ends on a barrier.
  __device__ static __forceinline__ void kloop(const P& p, Ring& w, uint8_t* ring,
                                               const uint8_t* img, int plane, int zero, int rows,
                                               int wm, int wn, int lane, typename C::Acc& acc) {
    const int lr = wm * 32 + (lane & 31);
    const int f = lr / GI::OPIX;
    const typename GI::Lane ln = GI::lane(f, lr - f * GI::OPIX, lr < rows);
    stash<0>(w, ring, 0);
    __syncthreads();
    auto group = [&](int k0, const uint8_t* sb) {
      const typename GI::Stage sg = GI::stage(ln, k0, zero);
      f16x8 fb[KS][NP], fa[KS][NP];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) fb[s][pl] = PB::frag(sb, pl, wn * 32, s, lane);
        const int a = GI::unit(sg, ln, k0, s, lane >> 5);
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
          fa[s][pl] = *reinterpret_cast<const f16x8*>(img + pl * plane + a);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < KS; ++s) acc.terms(0, 0, fa[s], fb[s]);
    };
    auto iter = [&](auto S, int kt) {
      constexpr int set = decltype(S)::value;
      stash<set ^ 1>(w, ring, (kt + 1) & 1);
      fetch<set>(w, p, (kt + 2) * BK);
      __builtin_amdgcn_sched_barrier(0);
      const uint8_t* sb = ring + (kt & 1) * NG * PB::BYTES;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (g > 0) {
          if (kt * BK + g * GK >= p.K) break;  // a short last stage (block-uniform)
          __builtin_amdgcn_sched_barrier(0);
        }
        group(kt * BK + g * GK, sb + g * PB::BYTES);
      }
      __syncthreads();
    };
    const int nk = (p.K + BK - 1) / BK;
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      iter(Set0{}, kt);
      iter(Set1{}, kt + 1);
    }
    if (kt < nk) iter(Set0{}, kt);
  }
};

// G3 / BK3_: the third convolution and its stage depth, or G3 = void for conv1 -> conv2 alone.
template <class G1, class G2, bool U8 = false, int BK1_ = 32, int BK2_ = 32, class G3 = void,
          int BK3_ = 32>
struct P3C12Cfg {
  static constexpr bool C3 = !std::is_void<G3>::value;
  using G3g = std::conditional_t<C3, G3, G2>;  // a geometry to name when there is no conv3
  using Place = C123Place<G1, G2, G3g, BK1_ / 32, BK2_ / 32, BK3_ / 32>;
  using I1 = ImgGeomPairs<G1>;
  using I2 = ImgGeom<G2, false>;
  using P1 = conv::P3ConvFwd<G1, 1, U8>;
  using P2 = conv::P3ConvFwd<G2, kPlanes>;
  static constexpr int NP = kPlanes;
  using P1L = P3C1ToLds<G1, G2, U8>;
  static constexpr int NT = 512, GK = 32, KS = 2;  // GK: k per fragment group (one PlanP3 tile)
  static constexpr int BK1 = BK1_, BK2 = BK2_, NG1 = BK1 / GK, NG2 = BK2 / GK;
  using C1 = P3Core<512, 32, 8, 1, GK, P1L>;  // 8 waves x 64 rows >= 441
  using C2 = P3Core<128, 64, 4, 2, GK, P2>;   // 4 x 2 waves of 32 x 32 (121 rows)
  using PB1 = PlanP3<32, NT, RCONTIG, NP, GK>;
  using PB2 = PlanP3<64, NT, RCONTIG, NP, GK>;
  static_assert(BK1 % GK == 0 && BK2 % GK == 0, "a stage is whole 32-k groups");
  static_assert(NG1 * PB1::UNITS <= NT && NG2 * PB2::UNITS <= NT,
                "one weight unit per thread per plane and stage");
  static constexpr int ZERO1 = img_zero_base(I1::IMG);  // region 0: frame image + zero area
  static constexpr int FRAME = ZERO1 + kImgZeroBytes;
  static constexpr int X1 = FRAME;
  // conv1's ring lies in the first x1 plane's image: its last read is before the k loop's
  // last barrier, and x1 is first written by conv1's epilogue, after it.
  static constexpr int RING1 = X1;
  static constexpr int ZERO2 = img_zero_base(I2::IMG);
  static constexpr int PLANE2 = ZERO2 + kImgZeroBytes;
  static constexpr int LDS = X1 + NP * PLANE2;
  static_assert(2 * NG1 * PB1::BYTES <= I2::IMG, "conv1's ring fits the first x1 plane's image");
  static_assert(2 * NG2 * PB2::BYTES <= I1::IMG && C1::EPI_BYTES <= I1::IMG &&
                    C2::EPI_BYTES <= I1::IMG,
                "conv2's ring and the epilogue staging reuse the frame image region");
  static_assert(G1::OPIX <= 512 && I2::OPIX <= 128 && P2::A_PLANES == NP, "geometry");
  // conv3 (C3): conv2's epilogue writes x2 as conv3's image over the dead x1 planes, and
  // conv3 (4 x 2 waves of 32 x 32, as conv3_fwd alone) runs from it; its ring and staging
  // reuse the frame region as conv2's do.
  using I3 = ImgGeom<G3g, false>;
  using P3 = conv::P3ConvFwd<G3g, kPlanes>;
  using P2L = P3ConvToLds<G2, G3g, kPlanes>;
  using C2L = P3Core<128, 64, 4, 2, GK, P2L>;
  using Ph3 = P3ImgPhase<I3, NT, 4, 2, BK3_, P3, P3>;
  static constexpr int X2 = Place::X2, ZERO3 = Place::ZERO3, PLANE3 = Place::PLANE3;
  // The placement the host checks (gemm_p3i_geom.h C123Place) is the one used here.
  static_assert(Place::FRAME == FRAME && Place::X1 == X1 && Place::PLANE2 == PLANE2 &&
                    Place::LDS == LDS && Place::ring1.lo == RING1 &&
                    Place::ring1.hi == RING1 + 2 * NG1 * PB1::BYTES &&
                    Place::ring2.hi == 2 * NG2 * PB2::BYTES && Place::epi1.hi == C1::EPI_BYTES &&
                    Place::epi23.hi == C2::EPI_BYTES,
                "C123Place describes this kernel");
  static_assert(!C3 || (Place::ring3.hi == Ph3::RING && Place::epi23.hi == C2L::EPI_BYTES &&
                        Place::epi23.hi == Ph3::C::EPI_BYTES && I3::OPIX <= 128),
                "C123Place describes conv3's regions");
  static_assert(Place::ok(), "no two live LDS regions overlap in any phase; under 160 KiB");
};

// With G3 (conv1 -> conv2 -> conv3): x2 is stored to HBM for frames below hbm2_frames only,
// p2.y otherwise names x2's scale record alone, and p3 is conv3 (its a_src: x2's record).
template <class G1, class G2, bool U8, int BK1_, int BK2_, class G3 = void, int BK3_ = 32>
__global__ void __launch_bounds__(512) gemm_p3c12_kernel(
    const conv::P3ConvFwd<G1, 1, U8> p1, const conv::P3ConvFwd<G2, kPlanes> p2, int frames,
    int hbm_frames, const typename P3C12Cfg<G1, G2, U8, BK1_, BK2_, G3, BK3_>::P3 p3,
    int hbm2_frames) {
  using Cfg = P3C12Cfg<G1, G2, U8, BK1_, BK2_, G3, BK3_>;
  using I1 = typename Cfg::I1;
  using I2 = typename Cfg::I2;
  using PB1 = typename Cfg::PB1;
  using PB2 = typename Cfg::PB2;
  using P1 = typename Cfg::P1;
  using P2 = typename Cfg::P2;
  constexpr int NT = Cfg::NT, GK = Cfg::GK, KS = Cfg::KS, NP = Cfg::NP;
  constexpr int BK1 = Cfg::BK1, BK2 = Cfg::BK2, NG1 = Cfg::NG1, NG2 = Cfg::NG2;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = blockIdx.x;
  uint8_t* x1 = smem + Cfg::X1;

  // ---- Weight rings (one unit per owning thread per plane): thread tid owns unit
  // tid % UNITS of its stage's group tid / UNITS.
  const bool own1 = tid < NG1 * PB1::UNITS, own2 = tid < NG2 * PB2::UNITS;
  const int g1 = tid / PB1::UNITS, u1 = tid % PB1::UNITS;
  const int g2 = tid / PB2::UNITS, u2 = tid % PB2::UNITS;
  const typename P1::BRow br1 = p1.b_row(own1 ? PB1::row_of(u1) : 0);
  const typename P2::BRow br2 = p2.b_row(own2 ? PB2::row_of(u2) : 0);
  __amdgpu_buffer_rsrc_t sb1[NP], sb2[NP];
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) {
    sb1[pl] = plane_rsrc(p1.b_src, pl);
    sb2[pl] = plane_rsrc(p2.b_src, pl);
  }
  u32x4 r1[2][NP], r2[2][NP];
  auto fetch1 = [&](auto S, int k0) {
    constexpr int set = decltype(S)::value;
    const uint32_t off =
        own1 && k0 + g1 * GK < p1.K ? p1.b_off(br1, k0 + g1 * GK, PB1::kk_of(u1)) : kOOB;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
      r1[set][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(sb1[pl], off, 0, 0));
  };
  auto fetch2 = [&](auto S, int k0) {
    constexpr int set = decltype(S)::value;
    const uint32_t off =
        own2 && k0 + g2 * GK < p2.K ? p2.b_off(br2, k0 + g2 * GK, PB2::kk_of(u2)) : kOOB;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
      r2[set][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(sb2[pl], off, 0, 0));
  };
  auto stash1 = [&](auto S, int buf) {
    constexpr int set = decltype(S)::value;
    if (!own1) return;
    uint8_t* s = smem + Cfg::RING1 + (buf * NG1 + g1) * PB1::BYTES;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<u32x4*>(s + pl * PB1::PLANE + PB1::offset(u1)) = r1[set][pl];
  };
  auto stash2 = [&](auto S, int buf) {
    constexpr int set = decltype(S)::value;
    if (!own2) return;
    uint8_t* s = smem + (buf * NG2 + g2) * PB2::BYTES;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<u32x4*>(s + pl * PB2::PLANE + PB2::offset(u2)) = r2[set][pl];
  };
  fetch1(Set0{}, 0);
  fetch1(Set1{}, BK1);
  fetch2(Set0{}, 0);
  fetch2(Set1{}, BK2);

  // ---- The frame image (f16 copy, pixel-pair units), each unit once; zero units.
  if constexpr (AU8<P1>::value) {  // the uint8 frame itself, widened exactly (gemm_p3i.h)
    constexpr int U8U = I1::UNITS / 2;
    constexpr int PER = (U8U + NT - 1) / NT;
    const __amdgpu_buffer_rsrc_t sa = plane_rsrc(p1.a_src, 0);
    u32x4 v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      const uint32_t off = u < U8U ? (uint32_t)(((int64_t)f * U8U + u) * 16) : kOOB;
      v[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(sa, off, 0, 0));
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      if (u < U8U) {
        *reinterpret_cast<u32x4*>(smem + I1::fill(0, 2 * u)) = f16x8_of_bytes(v[j][0], v[j][1]);
        *reinterpret_cast<u32x4*>(smem + I1::fill(0, 2 * u + 1)) = f16x8_of_bytes(v[j][2], v[j][3]);
      }
    }
    if (tid < 16) *reinterpret_cast<u32x4*>(smem + Cfg::ZERO1 + 16 * tid) = zero_u4();
    else if (tid < 16 + 16 * NP)
      *reinterpret_cast<u32x4*>(x1 + ((tid >> 4) - 1) * Cfg::PLANE2 + Cfg::ZERO2 + 16 * (tid & 15)) = zero_u4();
  } else {
    constexpr int PER = (I1::UNITS + NT - 1) / NT;
    const __amdgpu_buffer_rsrc_t sa = plane_rsrc(p1.a_src, 0);
    u32x4 v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      const uint32_t off = u < I1::UNITS ? (uint32_t)(((int64_t)f * I1::UNITS + u) * 16) : kOOB;
      v[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(sa, off, 0, 0));
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      if (u < I1::UNITS) *reinterpret_cast<u32x4*>(smem + I1::fill(0, u)) = v[j];
    }
    if (tid < 16) *reinterpret_cast<u32x4*>(smem + Cfg::ZERO1 + 16 * tid) = zero_u4();
    else if (tid < 16 + 16 * NP)
      *reinterpret_cast<u32x4*>(x1 + ((tid >> 4) - 1) * Cfg::PLANE2 + Cfg::ZERO2 + 16 * (tid & 15)) = zero_u4();
  }
  stash1(Set0{}, 0);
  __syncthreads();

  // ---- conv1: 8 waves x 64 rows.
  {
    typename I1::Lane ln[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int lr = wave * 64 + i * 32 + (lane & 31);
      ln[i] = I1::lane(0, lr, lr < G1::OPIX);
    }
    typename Cfg::C1::Acc acc;
    acc.zero();
    auto group = [&](int k0, const uint8_t* sb) {
      typename I1::Stage sg[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) sg[i] = I1::stage(ln[i], k0, Cfg::ZERO1);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        f16x8 fb[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) fb[pl] = PB1::frag(sb, pl, 0, s, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int u = I1::unit(sg[i], ln[i], k0, s, lane >> 5);
          const f16x8 fa[1] = {*reinterpret_cast<const f16x8*>(smem + u)};
          acc.terms(i, 0, fa, fb);
        }
      }
    };
    auto compute = [&](int k0, int buf) {  // a stage's groups in k order (K % BK1 == 0)
#pragma unroll
      for (int g = 0; g < NG1; ++g)
        group(k0 + g * GK, smem + Cfg::RING1 + (buf * NG1 + g) * PB1::BYTES);
    };
    auto iter = [&](auto S, int kt) {
      constexpr int set = decltype(S)::value;
      using Other = std::integral_constant<int, set ^ 1>;
      stash1(Other{}, set ^ 1);
      fetch1(S, (kt + 2) * BK1);
      compute(kt * BK1, set);
      __syncthreads();
    };
    const int nk = p1.K / BK1;
    for (int kt = 0; kt < nk; kt += 2) {
      iter(Set0{}, kt);
      iter(Set1{}, kt + 1);
    }
    typename Cfg::P1L q;
    q.M = (f + 1) * G1::OPIX < p1.M ? (f + 1) * G1::OPIX : p1.M;
    q.N = p1.N; q.K = p1.K; q.k_chunk = p1.k_chunk;
    q.base = p1; q.img = x1; q.plane = Cfg::PLANE2; q.m0 = f * G1::OPIX;
    q.hbm_rows = f < hbm_frames ? q.M : 0;
    Cfg::C1::epilogue(q, smem, q.m0, 0, wave, wave, 0, lane, 0, acc, false);  // ends on a barrier
  }

  // ---- conv2 on the x1 image: 4 x 2 waves of 32 x 32.
  stash2(Set0{}, 0);
  __syncthreads();
  {
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = wm * 32 + (lane & 31);
    const typename I2::Lane ln = I2::lane(0, lr, lr < I2::OPIX);
    typename Cfg::C2::Acc acc;
    acc.zero();
    auto group = [&](int k0, const uint8_t* sb) {
      const typename I2::Stage sg = I2::stage(ln, k0, Cfg::ZERO2);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        f16x8 fb[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) fb[pl] = PB2::frag(sb, pl, wn * 32, s, lane);
        const int u = I2::unit(sg, ln, k0, s, lane >> 5);
        const uint8_t* a = x1 + u;
        f16x8 fa[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) fa[pl] = *reinterpret_cast<const f16x8*>(a + pl * Cfg::PLANE2);
        acc.terms(0, 0, fa, fb);
      }
    };
    auto compute = [&](int k0, int buf) {  // a stage's groups in k order (K % BK2 == 0)
#pragma unroll
      for (int g = 0; g < NG2; ++g) group(k0 + g * GK, smem + (buf * NG2 + g) * PB2::BYTES);
    };
    auto iter = [&](auto S, int kt) {
      constexpr int set = decltype(S)::value;
      using Other = std::integral_constant<int, set ^ 1>;
      stash2(Other{}, set ^ 1);
      fetch2(S, (kt + 2) * BK2);
      compute(kt * BK2, set);
      __syncthreads();
    };
    const int nk = p2.K / BK2;
    for (int kt = 0; kt < nk; kt += 2) {
      iter(Set0{}, kt);
      iter(Set1{}, kt + 1);
    }
    const int m2 = (f + 1) * I2::OPIX < p2.M ? (f + 1) * I2::OPIX : p2.M;
    if constexpr (!Cfg::C3) {
      P2 q = p2;
      q.M = m2;
      Cfg::C2::epilogue(q, smem, f * I2::OPIX, 0, wave, wm, wn, lane, 0, acc, false);
    } else {
      // ---- conv3 on the x2 image.  x1 was last read before the k loop's last barrier: the
      // x2 planes' zero areas, conv3's first two weight stages (registers), then conv2's
      // epilogue into the image.
      using Ph3 = typename Cfg::Ph3;
      using I3 = typename Cfg::I3;
      uint8_t* x2 = smem + Cfg::X2;
      if (tid < 16 * NP)
        *reinterpret_cast<u32x4*>(x2 + (tid >> 4) * Cfg::PLANE3 + Cfg::ZERO3 + 16 * (tid & 15)) = zero_u4();
      typename Ph3::Ring w3;
      Ph3::init(w3, p3, tid);
      Ph3::template fetch<0>(w3, p3, 0);
      Ph3::template fetch<1>(w3, p3, Ph3::BK);
      typename Cfg::P2L q;
      q.M = m2; q.N = p2.N; q.K = p2.K; q.k_chunk = p2.k_chunk;
      q.base = p2; q.img = x2; q.plane = Cfg::PLANE3; q.m0 = f * I2::OPIX;
      q.hbm_rows = f < hbm2_frames ? m2 : 0;
      Cfg::C2L::epilogue(q, smem, q.m0, 0, wave, wm, wn, lane, 0, acc, false);  // ends on a barrier
      typename Ph3::C::Acc acc3;
      acc3.zero();
      const typename Cfg::P3::Pre pre3 = p3.pre(wn * 32 + Ph3::C::epi_col(lane));
      Ph3::kloop(p3, w3, smem, x2, Cfg::PLANE3, Cfg::ZERO3, I3::OPIX, wm, wn, lane, acc3);
      typename Cfg::P3 q3 = p3;
      q3.M = (f + 1) * I3::OPIX < p3.M ? (f + 1) * I3::OPIX : p3.M;
      Ph3::C::epilogue(q3, smem, f * I3::OPIX, 0, wave, wm, wn, lane, 0, acc3, false, &pre3);
    }
  }
}

// frames images; x1 planes are written to HBM for frames [0, hbm_frames) only.
template <int BK1_, int BK2_, class G1, class G2, bool U8>
inline hipError_t launch_gemm_p3c12(const conv::P3ConvFwd<G1, 1, U8>& p1,
                                    const conv::P3ConvFwd<G2, kPlanes>& p2, int frames, int hbm_frames,
                                    hipStream_t st) {
  using Cfg = P3C12Cfg<G1, G2, U8, BK1_, BK2_>;
  static_assert(Cfg::LDS <= 160 * 1024, "LDS");
  static hipError_t attr = p3_set_lds(&gemm_p3c12_kernel<G1, G2, U8, BK1_, BK2_>, Cfg::LDS);
  if (attr != hipSuccess) return attr;
  if (frames < 1 || p1.M != frames * G1::OPIX || p2.M != frames * G2::OPIX || p1.N > 32 ||
      p2.N > 64 || p1.K % (2 * Cfg::BK1) != 0 || p2.K % (2 * Cfg::BK2) != 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((gemm_p3c12_kernel<G1, G2, U8, BK1_, BK2_>), dim3(frames), dim3(Cfg::NT), Cfg::LDS, st, p1, p2,
                     frames, hbm_frames, typename Cfg::P3{}, 0);
  return hipGetLastError();
}

// conv1 -> conv2 -> conv3: x1 to HBM for frames [0, hbm_frames), x2 for [0, hbm2_frames).
template <int BK1_, int BK2_, int BK3_, class G1, class G2, class G3, bool U8>
inline hipError_t launch_gemm_p3c123(const conv::P3ConvFwd<G1, 1, U8>& p1,
                                     const conv::P3ConvFwd<G2, kPlanes>& p2,
                                     const conv::P3ConvFwd<G3, kPlanes>& p3, int frames,
                                     int hbm_frames, int hbm2_frames, hipStream_t st) {
  using Cfg = P3C12Cfg<G1, G2, U8, BK1_, BK2_, G3, BK3_>;
  static_assert(Cfg::LDS <= 160 * 1024, "LDS");
  static hipError_t attr =
      p3_set_lds(&gemm_p3c12_kernel<G1, G2, U8, BK1_, BK2_, G3, BK3_>, Cfg::LDS);
  if (attr != hipSuccess) return attr;
  if (frames < 1 || p1.M != frames * G1::OPIX || p2.M != frames * G2::OPIX ||
      p3.M != frames * G3::OPIX || p1.N > 32 || p2.N != 64 || p3.N > 64 ||
      p1.K % (2 * Cfg::BK1) != 0 || p2.K % (2 * Cfg::BK2) != 0 || p3.K % 32 != 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((gemm_p3c12_kernel<G1, G2, U8, BK1_, BK2_, G3, BK3_>), dim3(frames),
                     dim3(Cfg::NT), Cfg::LDS, st, p1, p2, frames, hbm_frames, p3, hbm2_frames);
  return hipGetLastError();
}

// ---- conv2 -> conv3, two frames per block (the online forward): conv2_fwd's image-resident
// body (x1 from HBM, 8 x 2 waves of 32 x 32 over the two frames' 242 rows), its epilogue into
// two x2 images in LDS -- and to HBM for frames below hbm_frames only; a block may hold one
// frame on each side of that limit -- then conv3 over the same two frames.
template <class G2, class G3, int BK2_, int BK3_>
struct P3C23Cfg {
  using Place = C23Place<G2, G3, BK2_ / 32, BK3_ / 32>;
  using I2 = ImgGeom<G2, false>;
  using I3 = ImgGeom<G3, false>;
  using P2 = conv::P3ConvFwd<G2, kPlanes>;
  using P3 = conv::P3ConvFwd<G3, kPlanes>;
  static constexpr int NT = 1024, FPB = Place::FPB, NP = kPlanes;
  using P2L = P3ConvToLds<G2, G3, kPlanes, false, FPB>;
  using Ph2 = P3ImgPhase<I2, NT, 8, 2, BK2_, P2, P2L>;
  using Ph3 = P3ImgPhase<I3, NT, 8, 2, BK3_, P3, P3>;
  static constexpr int LDS = Place::LDS;
  static_assert(FPB * I2::OPIX <= 256 && FPB * I3::OPIX <= 256, "8 waves of 32 rows cover the frames");
  static_assert(Place::ring2.hi - Place::ring2.lo == Ph2::RING && Place::ring3.hi == Ph3::RING &&
                    Place::EPI == Ph2::C::EPI_BYTES && Place::EPI == Ph3::C::EPI_BYTES,
                "C23Place describes this kernel");
  static_assert(Place::ok(), "no two live LDS regions overlap in any phase; under 160 KiB");
};

template <class G2, class G3, int BK2_, int BK3_>
__global__ void __launch_bounds__(1024) gemm_p3c23_kernel(const conv::P3ConvFwd<G2, kPlanes> p2,
                                                          const conv::P3ConvFwd<G3, kPlanes> p3,
                                                          int frames, int hbm_frames) {
  using Cfg = P3C23Cfg<G2, G3, BK2_, BK3_>;
  using Place = typename Cfg::Place;
  using I2 = typename Cfg::I2;
  using I3 = typename Cfg::I3;
  using Ph2 = typename Cfg::Ph2;
  using Ph3 = typename Cfg::Ph3;
  constexpr int NT = Cfg::NT, NP = Cfg::NP, FPB = Cfg::FPB;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int f0 = blockIdx.x * FPB;
  const int nf = frames - f0 < FPB ? frames - f0 : FPB;

  typename Ph2::Ring w2;
  Ph2::init(w2, p2, tid);
  Ph2::template fetch<0>(w2, p2, 0);
  Ph2::template fetch<1>(w2, p2, Ph2::BK);

  // ---- The block's x1 images, each unit of each plane loaded and stored once (gemm_p3i.h).
  {
    constexpr int UNITS = FPB * I2::UNITS;
    constexpr int PER = (UNITS + NT - 1) / NT;
    __amdgpu_buffer_rsrc_t srcA[NP];
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) srcA[pl] = plane_rsrc(p2.a_src, pl);
    u32x4 v[PER][NP];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      const bool ok = u < UNITS && u / I2::UNITS < nf;
      const uint32_t off = ok ? (uint32_t)(((int64_t)f0 * I2::UNITS + u) * 16) : kOOB;
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        v[j][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(srcA[pl], off, 0, 0));
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int u = tid + j * NT;
      if (UNITS % NT == 0 || u < UNITS) {
        const int f = u / I2::UNITS;
        const int a = I2::fill(f, u - f * I2::UNITS);
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<u32x4*>(smem + pl * Place::PLANE2 + a) = v[j][pl];
      }
    }
    if (tid < 16 * NP)
      *reinterpret_cast<u32x4*>(smem + (tid >> 4) * Place::PLANE2 + Place::ZERO2 + 16 * (tid & 15)) = zero_u4();
  }

  // ---- conv2 (its k loop starts on a barrier).
  typename Cfg::P2L q;
  q.M = (f0 + nf) * I2::OPIX < p2.M ? (f0 + nf) * I2::OPIX : p2.M;
  q.N = p2.N; q.K = p2.K; q.k_chunk = p2.k_chunk;
  q.base = p2; q.img = smem + Place::X2; q.plane = Place::PLANE3; q.m0 = f0 * I2::OPIX;
  q.hbm_rows = (hbm_frames < frames ? hbm_frames : frames) * I2::OPIX;
  typename Ph2::C::Acc acc2;
  acc2.zero();
  const typename Cfg::P2L::Pre pre2 = q.pre(wn * 32 + Ph2::C::epi_col(lane));
  Ph2::kloop(p2, w2, smem + Place::RING2, smem, Place::PLANE2, Place::ZERO2, nf * I2::OPIX, wm, wn,
             lane, acc2);

  // ---- x1 was last read before the k loop's last barrier: the x2 planes' zero areas, conv3's
  // first two weight stages (registers), conv2's epilogue into the x2 images, conv3.
  uint8_t* x2 = smem + Place::X2;
  if (tid < 16 * NP)
    *reinterpret_cast<u32x4*>(x2 + (tid >> 4) * Place::PLANE3 + Place::ZERO3 + 16 * (tid & 15)) = zero_u4();
  typename Ph3::Ring w3;
  Ph3::init(w3, p3, tid);
  Ph3::template fetch<0>(w3, p3, 0);
  Ph3::template fetch<1>(w3, p3, Ph3::BK);
  Ph2::C::epilogue(q, smem, q.m0, 0, wave, wm, wn, lane, 0, acc2, false, &pre2);  // ends on a barrier
  typename Ph3::C::Acc acc3;
  acc3.zero();
  const typename Cfg::P3::Pre pre3 = p3.pre(wn * 32 + Ph3::C::epi_col(lane));
  Ph3::kloop(p3, w3, smem, x2, Place::PLANE3, Place::ZERO3, nf * I3::OPIX, wm, wn, lane, acc3);
  typename Cfg::P3 q3 = p3;
  q3.M = (f0 + nf) * I3::OPIX < p3.M ? (f0 + nf) * I3::OPIX : p3.M;
  Ph3::C::epilogue(q3, smem, f0 * I3::OPIX, 0, wave, wm, wn, lane, 0, acc3, false, &pre3);
}

// `frames` images (an even count); x2 planes are written to HBM for frames [0, hbm_frames).
template <int BK2_, int BK3_, class G2, class G3>
inline hipError_t launch_gemm_p3c23(const conv::P3ConvFwd<G2, kPlanes>& p2,
                                    const conv::P3ConvFwd<G3, kPlanes>& p3, int frames,
                                    int hbm_frames, hipStream_t st) {
  using Cfg = P3C23Cfg<G2, G3, BK2_, BK3_>;
  static hipError_t attr = p3_set_lds(&gemm_p3c23_kernel<G2, G3, BK2_, BK3_>, Cfg::LDS);
  if (attr != hipSuccess) return attr;
  if (frames < 2 || frames % Cfg::FPB != 0 || hbm_frames < 0 || p2.M != frames * G2::OPIX ||
      p3.M != frames * G3::OPIX || p2.N != 64 || p3.N > 64 || p2.K % 32 != 0 || p3.K % 32 != 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((gemm_p3c23_kernel<G2, G3, BK2_, BK3_>), dim3(frames / Cfg::FPB),
                     dim3(Cfg::NT), Cfg::LDS, st, p2, p3, frames, hbm_frames);
  return hipGetLastError();
}

}  // namespace gemm
}  // namespace acme
