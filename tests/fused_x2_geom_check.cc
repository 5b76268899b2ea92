// Host check of the fused forwards' LDS placement (acme_amd/csrc/gemm_p3i_geom.h sink_at,
// C123Place, C23Place), compiled and run by tests/test_fused_x2_geom_cpu.py.  For both
// kernels of gemm_p3c12.h that keep x2 in LDS (conv1 -> conv2 -> conv3, one frame per block;
// conv2 -> conv3, two frames per block) and every stage depth torso.hip launches them at:
//   1. sink: for every (frame, oh, ow, chunk) of conv2's output, the LDS offset the epilogue
//      sink writes equals what ImgGeom<G3, false>::fill gives for that HBM unit of x2, the
//      offsets are distinct, inside the frames' images and never in the plane's zero area;
//   2. regions: in every phase of the kernel no two live regions overlap (checked here span
//      by span, and by the struct's own ok());
//   3. budget: the kernel's LDS is at most 160 KiB.
// Prints "name LDS-bytes" per instantiation; exit status 0 when everything holds.
#include <cstdio>
#include <set>
#include <vector>

#include "gemm_p3i_geom.h"

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

// The sink of conv2's epilogue over `fpb` frames of a block whose x2 plane is `plane` bytes
// with its zero area at `zero`.
static void check_sink(const char* name, int fpb, int zero, int plane) {
  using I3 = gemm::ImgGeom<G3, false>;
  std::set<int> seen;
  for (int f = 0; f < fpb; ++f)
    for (int oh = 0; oh < G2::OH; ++oh)
      for (int ow = 0; ow < G2::OW; ++ow)
        for (int c = 0; c < G2::CO / 8; ++c) {
          const int pp = oh * G2::OW + ow;
          const int a = gemm::sink_at<G2, G3>(f, pp, 8 * c);
          // x2 in HBM is [frame][oh][ow][CO]: unit (oh * OW + ow) * (CO / 8) + c.
          const int want = I3::fill(f, pp * (G2::CO / 8) + c);
          CHECK(a == want, "%s: sink (%d, %d, %d, %d) at %d, fill says %d", name, f, oh, ow, c, a, want);
          CHECK(a % 16 == 0 && a >= 0 && a + 16 <= fpb * I3::IMG, "%s: offset %d outside the images", name, a);
          CHECK(a + 16 <= zero && zero + gemm::kImgZeroBytes <= plane, "%s: offset %d in the zero area", name, a);
          CHECK(seen.insert(a).second, "%s: offset %d written twice", name, a);
        }
  CHECK((int)seen.size() == fpb * I3::UNITS, "%s: %zu units written of %d", name, seen.size(), fpb * I3::UNITS);
}

struct Named {
  const char* n;
  gemm::LdsSpan s;
};
// Every pair of a phase's live regions is disjoint, and every region lies inside the budget.
static void check_phase(const char* name, const char* phase, const std::vector<Named>& live, int lds) {
  for (size_t i = 0; i < live.size(); ++i) {
    CHECK(live[i].s.lo >= 0 && live[i].s.lo < live[i].s.hi && live[i].s.hi <= lds,
          "%s %s: %s [%d, %d) outside [0, %d)", name, phase, live[i].n, live[i].s.lo, live[i].s.hi, lds);
    for (size_t j = i + 1; j < live.size(); ++j)
      CHECK(gemm::lds_disjoint(live[i].s, live[j].s), "%s %s: %s [%d, %d) overlaps %s [%d, %d)", name,
            phase, live[i].n, live[i].s.lo, live[i].s.hi, live[j].n, live[j].s.lo, live[j].s.hi);
  }
}

template <int NG1, int NG2, int NG3>
static void check_c123(const char* name) {
  using P = gemm::C123Place<G1, G2, G3, NG1, NG2, NG3>;
  check_sink(name, 1, P::ZERO3, P::PLANE3);
  const int lds = P::LDS;
  check_phase(name, "conv1", {{"frame", P::frame}, {"ring1", P::ring1}}, lds);
  check_phase(name, "conv1 epilogue", {{"staging", P::epi1}, {"x1", P::x1}}, lds);
  check_phase(name, "conv2", {{"ring2", P::ring2}, {"x1", P::x1}}, lds);
  check_phase(name, "conv2 epilogue", {{"staging", P::epi23}, {"x2", P::x2}}, lds);
  check_phase(name, "conv3", {{"ring3", P::ring3}, {"x2", P::x2}}, lds);
  check_phase(name, "conv3 epilogue", {{"staging", P::epi23}}, lds);
  CHECK(P::x2.hi - P::x2.lo == 2 * P::PLANE3, "%s: x2 is two planes", name);
  CHECK(lds <= 160 * 1024, "%s: %d bytes of LDS", name, lds);
  CHECK(P::ok(), "%s: ok() fails", name);
  std::printf("%s %d\n", name, lds);
}

template <int NG2, int NG3>
static void check_c23(const char* name) {
  using P = gemm::C23Place<G2, G3, NG2, NG3>;
  check_sink(name, P::FPB, P::ZERO3, P::PLANE3);
  const int lds = P::LDS;
  check_phase(name, "conv2", {{"x1", P::x1}, {"ring2", P::ring2}}, lds);
  check_phase(name, "conv2 epilogue", {{"staging", P::epi}, {"x2", P::x2}}, lds);
  check_phase(name, "conv3", {{"ring3", P::ring3}, {"x2", P::x2}}, lds);
  check_phase(name, "conv3 epilogue", {{"staging", P::epi}}, lds);
  CHECK(P::x2.hi - P::x2.lo == 2 * P::PLANE3, "%s: x2 is two planes", name);
  CHECK(lds <= 160 * 1024, "%s: %d bytes of LDS", name, lds);
  CHECK(P::ok(), "%s: ok() fails", name);
  std::printf("%s %d\n", name, lds);
}

int main() {
  // torso.hip: kBkFused1 = 32, kBkFused2 = 64, kBkConv2 = 64, kBkConv3 = 32; BK32: 32 throughout.
  check_c123<1, 2, 1>("conv123_fwd");
  check_c123<1, 1, 1>("conv123_fwd.bk32");
  check_c23<2, 1>("conv23_fwd");
  check_c23<1, 1>("conv23_fwd.bk32");
  if (g_fail) std::fprintf(stderr, "%d checks failed\n", g_fail);
  return g_fail ? 1 : 0;
}
