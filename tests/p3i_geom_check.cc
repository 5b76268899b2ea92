// Host check of the LDS image geometries (acme_amd/csrc/gemm_p3i_geom.h), compiled and run
// by tests/test_p3i_geom_cpu.py.  For every geometry torso.hip instantiates (the P3I_GEMM
// launches, the fused kernel's halves and launch_gemm_p3s), with that instantiation's frames
// per block and wave counts:
//   1. placement: fill(f, u) is 16-B aligned, injective over the block's frames and units,
//      inside the plane's image and never in the zero area;
//   2. reads: for every GEMM row of the block (rows past a partial block's frames
//      included), every 32-k group, k16 step and lane half, unit() names exactly the
//      fill() address of the HBM unit the im2col definition reads (tap (kh, kw) and channel
//      chunk from k, TF SAME padding from conv::Geom), and a padding tap a zero-area unit;
//   3. conflicts: ds_read_b128 served in the lane groups {0-3, 12-15, 20-27},
//      {4-11, 16-19, 28-31} (and + 32), bank of byte address a = (a / 4) mod 64, every extra
//      distinct address on a busy bank one extra cycle for the group.  Prints, per geometry,
//      "name mean worst": the mean extra cycles per lane-group cycle over every wave, tile,
//      group and step, and the worst lane group's extra cycles.
// Exit status 0: placement and reads hold (the conflict figures are judged by the test).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#ifndef P3I_GEOM_HEADER
#define P3I_GEOM_HEADER "gemm_p3i_geom.h"
#endif
#include P3I_GEOM_HEADER

using namespace acme;

// The Nature torso's layers (acme_amd/csrc/torso.h).
using G1 = conv::Geom<84, 84, 4, 21, 21, 32, 8, 8, 4, 2, 2>;
using G2 = conv::Geom<21, 21, 32, 11, 11, 64, 4, 4, 2, 1, 1>;
using G3 = conv::Geom<11, 11, 64, 11, 11, 64, 3, 3, 1, 1, 1>;

static int g_fail = 0;
#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      if (++g_fail <= 20) {                \
        std::fprintf(stderr, __VA_ARGS__); \
        std::fprintf(stderr, "\n");        \
      }                                    \
    }                                      \
  } while (0)

// The im2col definitions: HBM unit of GEMM row pixel pp, k (a multiple of 8), or -1 (padding).
template <class G, bool DGRAD>
struct DefChunks {
  using GI = gemm::ImgGeom<G, DGRAD>;
  static constexpr int K = G::KH * G::KW * GI::C;
  static int hbm_unit(int pp, int k) {
    const int tap = k / GI::C, chunk = (k % GI::C) / 8;
    const int kh = tap / G::KW, kw = tap % G::KW;
    const int oh = pp / GI::OW, ow = pp % GI::OW;
    const int ih = DGRAD ? oh + G::PT - kh : oh * G::S - G::PT + kh;
    const int iw = DGRAD ? ow + G::PL - kw : ow * G::S - G::PL + kw;
    if (ih < 0 || ih >= GI::H || iw < 0 || iw >= GI::W) return -1;
    return (ih * GI::W + iw) * GI::CPX + chunk;
  }
};
template <class G>
struct DefPairs {
  using GI = gemm::ImgGeomPairs<G>;
  static constexpr int K = G::K;
  static int hbm_unit(int pp, int k) {
    const int kh = k / (G::KW * G::CI), kw = (k % (G::KW * G::CI)) / G::CI;
    const int oh = pp / G::OW, ow = pp % G::OW;
    const int ih = oh * G::S - G::PT + kh, iw = ow * G::S - G::PL + kw;
    if (ih < 0 || ih >= G::IH || iw < 0 || iw >= G::IW) return -1;
    return ih * (G::IW / 2) + iw / 2;
  }
};

static const int kGroup[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// Extra LDS cycles of one lane group: the busiest bank's distinct addresses, less one.
static int group_extra(const int* addr, const int* lanes) {
  int worst = 1;
  for (int bank = 0; bank < 64; ++bank) {
    std::set<int> distinct;
    for (int i = 0; i < 16; ++i) {
      const int a = addr[lanes[i]];
      if (((a / 4) & 63) <= bank && bank < ((a / 4) & 63) + 4) distinct.insert(a);
    }
    if ((int)distinct.size() > worst) worst = (int)distinct.size();
  }
  return worst - 1;
}

// One instantiation: FPB frames per block, WM M-waves of MT 32-row tiles.
template <class GI, class Def>
static void check(const char* name, int FPB, int WM, int MT) {
  const int images = FPB * GI::IMG;
  const int zero = gemm::img_zero_base(images), plane = zero + gemm::kImgZeroBytes;
  // 1. placement
  std::vector<int> owner(plane / 16, -1);
  for (int f = 0; f < FPB; ++f)
    for (int u = 0; u < GI::UNITS; ++u) {
      const int a = GI::fill(f, u);
      CHECK(a % 16 == 0, "%s: fill(%d, %d) = %d is not 16-B aligned", name, f, u, a);
      CHECK(a >= 0 && a + 16 <= images, "%s: fill(%d, %d) = %d leaves the image", name, f, u, a);
      if (a < 0 || a + 16 > images || a % 16) continue;
      CHECK(owner[a / 16] < 0, "%s: fill(%d, %d) = %d is taken", name, f, u, a);
      owner[a / 16] = f * GI::UNITS + u;
    }
  // 2. reads, 3. conflicts
  long cycles = 0, extra = 0;
  int worst = 0;
  for (int nf = 1; nf <= FPB; ++nf) {  // frames this block holds (nf < FPB: a partial block)
    const int rows = nf * GI::OPIX;
    for (int wm = 0; wm < WM; ++wm)
      for (int i = 0; i < MT; ++i)
        for (int k0 = 0; k0 < Def::K; k0 += 32)
          for (int s = 0; s < 2; ++s) {
            int addr[64];
            for (int lane = 0; lane < 64; ++lane) {
              const int lr = wm * 32 * MT + i * 32 + (lane & 31), h = lane >> 5;
              const int f = lr / GI::OPIX;
              const typename GI::Lane ln = GI::lane(f, lr - f * GI::OPIX, lr < rows);
              const typename GI::Stage sg = GI::stage(ln, k0, zero);
              const int a = GI::unit(sg, ln, k0, s, h);
              addr[lane] = a;
              const int hu = lr < rows ? Def::hbm_unit(lr - f * GI::OPIX, k0 + 16 * s + 8 * h) : -1;
              if (hu >= 0)
                CHECK(a == GI::fill(f, hu), "%s: row %d k %d reads %d, not unit %d's %d", name, lr,
                      k0 + 16 * s + 8 * h, a, hu, GI::fill(f, hu));
              else
                CHECK(a >= zero && a + 16 <= plane && a % 16 == 0,
                      "%s: row %d k %d (padding) reads %d outside the zero area", name, lr,
                      k0 + 16 * s + 8 * h, a);
            }
            if (nf < FPB) continue;  // the model counts full blocks
            for (int g = 0; g < 4; ++g) {
              const int e = group_extra(addr, kGroup[g]);
              ++cycles;
              extra += e;
              if (e > worst) worst = e;
            }
          }
  }
  std::printf("%s %.4f %d\n", name, (double)extra / (double)cycles, worst);
}

// The sub-pixel input gradient (gemm_p3s.h): FPB frames per block, per frame and parity
// class two waves of MT = 2 32-row tiles.  The im2col definition: row (i, j) of class
// (ph, pw) is dX pixel (rh + S i, rw + S j); k = (jh, jw, channel) is kernel tap
// kh = ph + S jh, kw = pw + S jw, which reads dZ pixel ((ih + PT - kh) / S, (iw + PL - kw) / S).
template <class G>
static void check_sub(const char* name, int FPB) {
  using GI = gemm::ImgGeomSub<G>;
  const int images = FPB * GI::IMG;
  const int zero = gemm::img_zero_base(images), plane = zero + gemm::kImgZeroBytes;
  std::vector<int> owner(plane / 16, -1);
  for (int f = 0; f < FPB; ++f)
    for (int u = 0; u < GI::UNITS; ++u) {
      const int a = GI::fill(f, u);
      CHECK(a % 16 == 0, "%s: fill(%d, %d) = %d is not 16-B aligned", name, f, u, a);
      CHECK(a >= 0 && a + 16 <= images, "%s: fill(%d, %d) = %d leaves the image", name, f, u, a);
      if (a < 0 || a + 16 > images || a % 16) continue;
      CHECK(owner[a / 16] < 0, "%s: fill(%d, %d) = %d is taken", name, f, u, a);
      owner[a / 16] = f * GI::UNITS + u;
    }
  long cycles = 0, extra = 0;
  int worst = 0;
  for (int nf = 1; nf <= FPB; ++nf)
    for (int f = 0; f < FPB; ++f)
      for (int z = 0; z < GI::CLASSES; ++z) {
        const int ph = z / G::S, pw = z % G::S;
        const int rh = ((ph - G::PT) % G::S + G::S) % G::S, rw = ((pw - G::PL) % G::S + G::S) % G::S;
        const int nh = (G::IH - rh + G::S - 1) / G::S, nw = (G::IW - rw + G::S - 1) / G::S;
        for (int tile = 0; tile < 4; ++tile)  // half * MT + i
          for (int k0 = 0; k0 < GI::KR; k0 += 32)
            for (int s = 0; s < 2; ++s) {
              int addr[64];
              for (int lane = 0; lane < 64; ++lane) {
                const int lr = tile * 32 + (lane & 31), h = lane >> 5;
                const typename GI::Lane ln = GI::lane(f, z, lr, f < nf);
                const int a = GI::unit(GI::stage(ln, k0, zero), ln, k0, s, h);
                addr[lane] = a;
                int hu = -1;
                if (f < nf && lr < nh * nw) {
                  const int k = k0 + 16 * s + 8 * h;
                  const int jh = k / (GI::JW * GI::C), jw = k / GI::C % GI::JW;
                  const int ih = rh + G::S * (lr / nw), iw = rw + G::S * (lr % nw);
                  const int th = ih + G::PT - (ph + G::S * jh), tw = iw + G::PL - (pw + G::S * jw);
                  CHECK(th % G::S == 0 && tw % G::S == 0, "%s: class %d is not a parity class", name, z);
                  const int oh = th / G::S, ow = tw / G::S;
                  if (th >= 0 && tw >= 0 && oh < G::OH && ow < G::OW)
                    hu = (oh * G::OW + ow) * GI::CPX + (k % GI::C) / 8;
                }
                if (hu >= 0)
                  CHECK(a == GI::fill(f, hu), "%s: class %d row %d k %d reads %d, not unit %d's %d",
                        name, z, lr, k0 + 16 * s + 8 * h, a, hu, GI::fill(f, hu));
                else
                  CHECK(a >= zero && a + 16 <= plane && a % 16 == 0,
                        "%s: class %d row %d k %d (padding) reads %d outside the zero area", name, z,
                        lr, k0 + 16 * s + 8 * h, a);
              }
              if (nf < FPB) continue;
              for (int g = 0; g < 4; ++g) {
                const int e = group_extra(addr, kGroup[g]);
                ++cycles;
                extra += e;
                if (e > worst) worst = e;
              }
            }
      }
  std::printf("%s %.4f %d\n", name, (double)extra / (double)cycles, worst);
}

int main() {
  using I1F = gemm::ImgGeomPairs<G1>;
  using I2F = gemm::ImgGeom<G2, false>;
  using I3F = gemm::ImgGeom<G3, false>;
  using I3D = gemm::ImgGeom<G3, true>;
  // name, frames per block, M-waves, 32-row tiles per wave: the P3I_GEMM lines of torso.hip
  // and the two halves of the fused conv1 -> conv2 kernel (gemm_p3c12.h).
  check<I1F, DefPairs<G1>>("conv1_fwd", 1, 7, 2);
  check<I2F, DefChunks<G2, false>>("conv2_fwd", 2, 8, 1);
  check<I3F, DefChunks<G3, false>>("conv3_fwd", 1, 4, 1);
  check<I3D, DefChunks<G3, true>>("conv3_dgrad", 2, 8, 1);
  check<I1F, DefPairs<G1>>("conv12_fwd.conv1", 1, 8, 2);
  check<I2F, DefChunks<G2, false>>("conv12_fwd.conv2", 1, 4, 1);
  check_sub<G2>("conv2_dgrad", 2);  // launch_gemm_p3s<G2, 2>
  if (g_fail) std::fprintf(stderr, "%d checks failed\n", g_fail);
  return g_fail ? 1 : 0;
}
