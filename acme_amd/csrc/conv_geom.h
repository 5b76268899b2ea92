// A convolution's static geometry (TF SAME padding: PT / PL rows / columns of zeros above /
// left of the input).  No HIP dependency: host tools and tests include it as it is.
#pragma once

namespace acme {
namespace conv {

template <int IH_, int IW_, int CI_, int OH_, int OW_, int CO_, int KH_, int KW_, int S_,
          int PT_, int PL_>
struct Geom {
  static constexpr int IH = IH_, IW = IW_, CI = CI_, OH = OH_, OW = OW_, CO = CO_;
  static constexpr int KH = KH_, KW = KW_, S = S_, PT = PT_, PL = PL_;
  static constexpr int K = KH * KW * CI;
  static constexpr int IPIX = IH * IW, OPIX = OH * OW;
  static_assert(CI % 4 == 0 && CO % 4 == 0, "channel counts must be multiples of 4");
};

}  // namespace conv
}  // namespace acme
