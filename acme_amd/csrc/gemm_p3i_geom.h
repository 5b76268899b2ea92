// LDS image geometries of the image-resident convolutions (gemm_p3i.h, gemm_p3c12.h,
// gemm_p3s.h).
// No HIP dependency: the kernels include this header and so does the host program of
// tests/test_p3i_geom_cpu.py, which checks every placement and read and models the bank
// conflicts of the A-fragment reads.
//
// A geometry GI says where each 16-B unit (8 consecutive k of one GEMM row) lives:
//   UNITS            16-B HBM units per frame (frames contiguous in HBM);
//   IMG              LDS bytes of one frame's image (one plane);
//   fill(f, u)       LDS byte offset of HBM unit u of the block's frame f;
//   Lane lane(f, pp, ok)         per-lane state of output pixel pp of frame f;
//   Stage stage(lane, k0, zero)  per 32-k group (k0 a multiple of 32); zero: the byte
//                                offset of the plane's zero area (img_zero_base());
//   int unit(stage, lane, k0, s, h)  byte offset of the lane's unit in k16 step s (lane
//                                    half h); for a padding tap, the zero unit in the bank
//                                    group its read would have had in an unbounded image.
// Every plane ends in a zero area of 16 units, one per bank group, 256-B aligned, so a
// padding lane's address is its unbounded one folded into the area (zero + (a & 255)): it
// is chosen once per group in stage(), and unit() costs what a real pixel's does.
//
// Bank conflicts.  A ds_read_b128 is served in groups of 16 lanes -- {0-3, 12-15, 20-27}
// and {4-11, 16-19, 28-31} of each half wave -- and a group is conflict-free when its 16
// units fall in 16 distinct bank groups (unit index mod 16).  Lane r of a fragment is GEMM
// row r, so those lane sets are conflict-free whenever the lanes read CONSECUTIVE image
// positions: position = GEMM row + a constant of the tap, for every lane of the block.
// The layouts below are built for exactly that:
//   * stride 1: pixels row-major with pitch OW (= W);
//   * stride S: the S*S (row, column) residue classes of the input stored class-major,
//     each with pitch OW, so a tap (one class, a fixed shift) reads pixel oh * OW + ow + c;
//   * frames FPITCH apart with FPITCH = OPIX (mod 16), so the rule carries over a frame
//     boundary inside a wave;
//   * a padding tap reads the zero unit of the bank group of its (unbounded) position.
#pragma once

#include "conv_geom.h"

#if defined(__HIPCC__)
#define ACME_GEOM_FN __host__ __device__ static __forceinline__
#else
#define ACME_GEOM_FN static inline
#endif

namespace acme {
namespace gemm {

constexpr int kImgZeroBytes = 256;  // 16 zero units, one per bank group

// Where the zero area of a plane with `bytes` of images starts.
constexpr int img_zero_base(int bytes) { return (bytes + 255) & ~255; }

// The smallest pitch >= n with pitch = opix (mod 16).
constexpr int img_pitch(int n, int opix) { return n + (((opix - n) % 16) + 16) % 16; }

// Channel-chunk images (conv2 / conv3 forward, stride-1 input gradient) over conv_geom.h's
// Geom G.  Forward (DGRAD = false): the image is the layer input X [IH][IW][CI], GEMM rows
// are (frame, oh, ow), tap (kh, kw) reads (oh*S - PT + kh, ow*S - PL + kw).  Input gradient
// (DGRAD = true, stride 1): the image is dZ [OH][OW][CO], rows are (frame, ih, iw), tap
// (kh, kw) reads (ih + PT - kh, iw + PL - kw).  K is ordered (kh, kw, channel), as
// conv_p3.h; C is 32 or 64, so a 32-k group stays within one tap.
// LDS layout, per plane: pixel (ih, iw) of frame f is position
//   q = f * FPITCH + class(ih % S, iw % S) * CH * CW + (ih / S) * CW + iw / S
// (CH x CW the class image, CW = OW); the 16-B channel chunk c of position q sits at chunk
// c ^ ((q >> SWZ) & (CPX - 1)), CPX chunks per pixel, so 16 consecutive positions' reads of
// one chunk fall in 16 distinct bank groups.
template <class G, bool DGRAD>
struct ImgGeom {
  static constexpr int H = DGRAD ? G::OH : G::IH, W = DGRAD ? G::OW : G::IW;
  static constexpr int C = DGRAD ? G::CO : G::CI;
  static constexpr int OH = DGRAD ? G::IH : G::OH, OW = DGRAD ? G::IW : G::OW;
  static constexpr int S = DGRAD ? 1 : G::S;
  static constexpr int KW = G::KW;
  static constexpr int OPIX = OH * OW, IPIX = H * W;
  static constexpr int CPX = C / 8;  // 16-B chunks per pixel
  static constexpr int SWZ = CPX == 8 ? 1 : 2;
  static constexpr int CH = (H + S - 1) / S, CW = (W + S - 1) / S;  // one class's image
  static constexpr int FPITCH = img_pitch(S * S * CH * CW, OPIX);   // positions per frame
  static constexpr int UNITS = IPIX * CPX, IMG = FPITCH * 2 * C;
  static_assert(!DGRAD || G::S == 1, "strided input gradients are not image-resident");
  static_assert(C == 32 || C == 64, "a 32-k group must stay within one tap");
  static_assert(S == 1 || S == 2, "stride 1 or 2");
  static_assert(CW == OW, "class pitch = output pitch: a tap's positions are row + constant");
  ACME_GEOM_FN int dh(int kh) { return DGRAD ? G::PT - kh : kh - G::PT; }
  ACME_GEOM_FN int dw(int kw) { return DGRAD ? G::PL - kw : kw - G::PL; }
  // Position of pixel (ih, iw), in the image or not (arithmetic shifts: -1 >> 1 = -1).
  ACME_GEOM_FN int pix(int fr, int ih, int iw) {
    if constexpr (S == 1) return fr * FPITCH + ih * CW + iw;
    else return fr * FPITCH + ((ih & 1) * 2 + (iw & 1)) * (CH * CW) + (ih >> 1) * CW + (iw >> 1);
  }
  ACME_GEOM_FN int swz(int q) { return (q >> SWZ) & (CPX - 1); }
  // Byte offset of channel chunk c of pixel (ih, iw) of frame fr.
  ACME_GEOM_FN int at(int fr, int ih, int iw, int c) {
    const int q = pix(fr, ih, iw);
    return q * (2 * C) + 16 * (c ^ swz(q));
  }
  ACME_GEOM_FN int fill(int f, int u) {
    const int px = u / CPX, c = u - px * CPX;
    const int ih = px / W, iw = px - ih * W;
    return at(f, ih, iw, c);
  }
  struct Lane {
    int f, ih, iw;
    bool ok;
  };
  ACME_GEOM_FN Lane lane(int f, int pp, bool ok) {
    const int oh = pp / OW, ow = pp - oh * OW;
    return Lane{f, oh * S, ow * S, ok};
  }
  struct Stage {
    int base, x;  // position byte base (in the zero area for a padding tap), chunk swizzle
  };
  ACME_GEOM_FN Stage stage(const Lane& l, int k0, int zero) {
    const int tap = k0 / C;  // wave-uniform
    const int kh = tap / KW, kw = tap - kh * KW;
    const int ih = l.ih + dh(kh), iw = l.iw + dw(kw);
    const bool in = l.ok && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
    const int q = pix(l.f, ih, iw);
    const int b = q * (2 * C);  // a multiple of the pixel size: the chunk stays inside 256 B
    return Stage{in ? b : zero + (b & 255), swz(q)};
  }
  ACME_GEOM_FN int unit(const Stage& st, const Lane&, int k0, int s, int h) {
    const int c = ((k0 % C) >> 3) + 2 * s + h;
    return st.base + 16 * (c ^ st.x);
  }
};

// Pixel-pair images for a 4-channel input (conv1 over the frames, one plane): a unit is two
// horizontally adjacent pixels x 4 channels, which is exactly the 8 k of one MFMA lane
// (k = (kh, kw, c): kw even, kw + 1) -- 16 B of the f16 frame copy.  A 32-k group is one
// kernel row kh (KW * CI = 32).  LDS layout: unit (ih, pw) (pw = iw / 2) of frame f is
// position
//   q = f * FPITCH + class(ih % S, pw % (S / 2)) * CH * CW + (ih / S) * CW + pw / (S / 2)
// with CW = OW, so kernel row kh, pair kp of output pixel (oh, ow) reads position
// oh * OW + ow + a constant of (kh, kp).
template <class G>
struct ImgGeomPairs {
  static constexpr int UNIT = 16;  // LDS bytes per unit
  static constexpr int H = G::IH, W = G::IW;
  static constexpr int OW = G::OW, OPIX = G::OPIX;
  static constexpr int PAIRS = W / 2;
  static constexpr int SR = G::S, SC = G::S / 2;  // row / pair-column classes
  static constexpr int CH = (H + SR - 1) / SR, CW = (PAIRS + SC - 1) / SC;
  static constexpr int FPITCH = img_pitch(SR * SC * CH * CW, OPIX);
  static constexpr int UNITS = H * PAIRS, IMG = FPITCH * UNIT;
  static_assert(G::CI == 4 && G::KW * G::CI == 32, "4 channels, one kernel row per group");
  static_assert(W % 2 == 0 && G::S % 2 == 0 && G::PL % 2 == 0, "pairs never straddle the border");
  static_assert((SR & (SR - 1)) == 0 && (SC & (SC - 1)) == 0, "power-of-two classes");
  static_assert(CW == OW, "class pitch = output pitch: a tap's positions are row + constant");
  // Position of unit (ih, pw), in the image or not: the row part, then the whole.
  ACME_GEOM_FN int row_pos(int fr, int ih) {
    const int cr = ih & (SR - 1);
    return fr * FPITCH + cr * SC * (CH * CW) + (ih - cr) / SR * CW;
  }
  ACME_GEOM_FN int pos(int rp, int pw) {
    const int cc = pw & (SC - 1);
    return rp + cc * (CH * CW) + (pw - cc) / SC;
  }
  ACME_GEOM_FN int fill(int f, int u) {
    const int ih = u / PAIRS, pw = u - ih * PAIRS;
    return pos(row_pos(f, ih), pw) * UNIT;
  }
  struct Lane {
    int f, ih, iw;
    bool ok;
  };
  ACME_GEOM_FN Lane lane(int f, int pp, bool ok) {
    const int oh = pp / OW, ow = pp - oh * OW;
    return Lane{f, oh * G::S - G::PT, ow * G::S - G::PL, ok};
  }
  struct Stage {
    int rp;    // row_pos of the group's kernel row
    bool in;   // ... which lies inside the image
    int zero;  // the plane's zero area
  };
  ACME_GEOM_FN Stage stage(const Lane& l, int k0, int zero) {
    const int ih = l.ih + k0 / 32;
    return Stage{row_pos(l.f, ih), l.ok && (unsigned)ih < (unsigned)H, zero};
  }
  ACME_GEOM_FN int unit(const Stage& st, const Lane& l, int, int s, int h) {
    const int iw = l.iw + 4 * s + 2 * h;  // kw = (16 s + 8 h) / 4; even
    const int q = pos(st.rp, (iw - (iw & 1)) / 2);
    const int a = q * UNIT;
    return st.in && (unsigned)iw < (unsigned)W ? a : st.zero + (a & 255);
  }
};

// Sub-pixel images for a strided input gradient (gemm_p3s.h: conv2's dZ -> dX).  The image
// is dZ [OH][OW][CO], row-major with pitch OW, channel chunks swizzled by the pixel index
// within the frame as ImgGeom's; frames lie IMG bytes apart (a wave reads one frame only).
// dX's pixels split into the S*S parity classes of conv_p3.h P3ConvDgradSubZ: class
// z = (ph, pw) holds the pixels (rh + S i, rw + S j), i < nh, j < nw, as GEMM rows
// i * nw + j, and its K = (jh, jw, channel) is the sub-kernel kh = ph + S jh, kw = pw + S jw,
// whose tap reads dZ (oh0 - jh, ow0 - jw), (oh0, ow0) the row's anchor.  A class of nw < OW
// columns wraps inside a 16-lane group, so its reads keep some conflicts (the row order
// is the problem's, shared with its epilogue).
// A padding tap reads the zero area's unit of its chunk alone (one address for every
// padding lane of a read): with the row wrap left, a banked choice as ImgGeom's did not
// pay here (model 0.59 -> 0.50, kernel and step unchanged).
template <class G>
struct ImgGeomSub {
  static constexpr int S = G::S, CLASSES = S * S;
  static constexpr int H = G::OH, W = G::OW, C = G::CO;
  static constexpr int JW = G::KW / S, KR = (G::KH / S) * JW * C;
  static constexpr int CPX = C / 8;
  static constexpr int SWZ = CPX == 8 ? 1 : 2;
  static constexpr int UNITS = H * W * CPX, IMG = H * W * 2 * C;
  static_assert(C == 32 || C == 64, "a 32-k group must stay within one tap");
  struct Cls {
    int ph, pw, rh, rw, nh, nw;
  };
  ACME_GEOM_FN Cls cls(int z) {
    const int ph = z / S, pw = z % S;
    const int rh = ((ph - G::PT) % S + S) % S, rw = ((pw - G::PL) % S + S) % S;
    return Cls{ph, pw, rh, rw, (G::IH - rh + S - 1) / S, (G::IW - rw + S - 1) / S};
  }
  ACME_GEOM_FN int swz(int q) { return (q >> SWZ) & (CPX - 1); }
  ACME_GEOM_FN int fill(int f, int u) {
    const int q = u / CPX, c = u - q * CPX;
    return f * IMG + q * (2 * C) + 16 * (c ^ swz(q));
  }
  struct Lane {
    int f, oh0, ow0;  // the row's dZ anchor
    bool ok;
  };
  // Row lr of class z of the block's frame f (ok: the frame exists).
  ACME_GEOM_FN Lane lane(int f, int z, int lr, bool ok) {
    const Cls k = cls(z);
    const bool in = ok && lr < k.nh * k.nw;
    const int i = in ? lr / k.nw : 0, j = in ? lr - i * k.nw : 0;
    return Lane{f, (k.rh + S * i + G::PT - k.ph) / S, (k.rw + S * j + G::PL - k.pw) / S, in};
  }
  struct Stage {
    int base, x;  // pixel byte base (in the zero area for a padding tap), chunk swizzle
  };
  ACME_GEOM_FN Stage stage(const Lane& l, int k0, int zero) {
    constexpr int T = JW * C;
    const int jh = k0 / T, jw = (k0 - jh * T) / C;  // wave-uniform
    const int oh = l.oh0 - jh, ow = l.ow0 - jw;
    const bool in = l.ok && (unsigned)oh < (unsigned)H && (unsigned)ow < (unsigned)W;
    const int q = oh * W + ow;
    const int b = l.f * IMG + q * (2 * C);
    return in ? Stage{b, swz(q)} : Stage{zero, 0};
  }
  ACME_GEOM_FN int unit(const Stage& st, const Lane&, int k0, int s, int h) {
    const int c = ((k0 % C) >> 3) + 2 * s + h;
    return st.base + 16 * (c ^ st.x);
  }
};

// ---- Fused forwards (gemm_p3c12.h): a convolution's epilogue writes its output straight
// into the next layer's LDS image, and the placement of every region in every phase.

// Byte offset, within a plane of the block's ImgGeom<Gto, false> images, of output channels
// n .. n + 7 (n a multiple of 8) of output pixel pp of the block's frame f of a forward
// convolution over Gfrom: the unit ImgGeom<Gto, false>::fill places there from HBM.
template <class Gfrom, class Gto>
ACME_GEOM_FN int sink_at(int f, int pp, int n) {
  static_assert(Gfrom::OH == Gto::IH && Gfrom::OW == Gto::IW && Gfrom::CO == Gto::CI,
                "the output is the next layer's input");
  const int oh = pp / Gfrom::OW, ow = pp - oh * Gfrom::OW;
  return ImgGeom<Gto, false>::at(f, oh, ow, n / 8);
}

// A weight ring of two stages of ng 32-k groups of a [32][bn] two-plane f16 panel, and the
// epilogue's row-major f32 staging of `waves` 32 x tn tiles (gemm_p3.h P3Core::EPI_BYTES).
constexpr int p3_ring_bytes(int bn, int ng) { return 2 * ng * (2 * bn * 32 * 2); }
constexpr int p3_epi_bytes(int waves, int tn) { return waves * 32 * (tn + 4) * 4; }

struct LdsSpan {
  int lo, hi;  // bytes [lo, hi)
};
constexpr bool lds_disjoint(LdsSpan a, LdsSpan b) { return a.hi <= b.lo || b.hi <= a.lo; }
constexpr int lds_max(int a, int b) { return a > b ? a : b; }

// conv1 -> conv2 (-> conv3), one frame per block, 8 waves (gemm_p3c12_kernel).  Region 0
// holds the frame image, then conv2's and conv3's weight rings and every epilogue's
// staging; region 1 the two x1 planes (conv1's ring in the first until conv1's epilogue
// writes x1), then, once conv2's k loop has read x1 for the last time, the two x2 planes.
template <class G1, class G2, class G3, int NG1, int NG2, int NG3>
struct C123Place {
  using I1 = ImgGeomPairs<G1>;
  using I2 = ImgGeom<G2, false>;
  using I3 = ImgGeom<G3, false>;
  static constexpr int NP = 2, WAVES = 8;
  static constexpr int ZERO1 = img_zero_base(I1::IMG), FRAME = ZERO1 + kImgZeroBytes;
  static constexpr int ZERO2 = img_zero_base(I2::IMG), PLANE2 = ZERO2 + kImgZeroBytes;
  static constexpr int ZERO3 = img_zero_base(I3::IMG), PLANE3 = ZERO3 + kImgZeroBytes;
  static constexpr int X1 = FRAME, X2 = FRAME;
  static constexpr int LDS = X1 + NP * PLANE2;
  static constexpr LdsSpan frame{0, FRAME}, x1{X1, X1 + NP * PLANE2}, x2{X2, X2 + NP * PLANE3};
  static constexpr LdsSpan ring1{X1, X1 + p3_ring_bytes(32, NG1)};
  static constexpr LdsSpan ring2{0, p3_ring_bytes(64, NG2)}, ring3{0, p3_ring_bytes(64, NG3)};
  static constexpr LdsSpan epi1{0, p3_epi_bytes(WAVES, 32)}, epi23{0, p3_epi_bytes(WAVES, 32)};
  // Phases: conv1's k loop {frame, ring1}; its epilogue {epi1, x1}; conv2's k loop
  // {ring2, x1}; its epilogue {epi23, x2}; conv3's k loop {ring3, x2}; its epilogue {epi23}.
  static constexpr bool ok() {
    return lds_disjoint(frame, ring1) && ring1.hi <= X1 + I2::IMG && lds_disjoint(epi1, x1) &&
           lds_disjoint(ring2, x1) && lds_disjoint(epi23, x2) && lds_disjoint(ring3, x2) &&
           x2.hi <= x1.hi && epi1.hi <= FRAME && epi23.hi <= FRAME && ring2.hi <= FRAME &&
           ring3.hi <= FRAME && LDS <= 160 * 1024;
  }
};

// conv2 -> conv3, two frames per block, 16 waves (gemm_p3c23_kernel).  conv2's k loop reads
// the x1 images (two planes of two frames) beside its weight ring; then x1 is dead: conv2's
// epilogue stages through the bottom and writes the x2 images above the staging, conv3's
// ring and its epilogue's staging reuse the bottom.
template <class G2, class G3, int NG2, int NG3>
struct C23Place {
  using I2 = ImgGeom<G2, false>;
  using I3 = ImgGeom<G3, false>;
  static constexpr int NP = 2, FPB = 2, WAVES = 16;
  static constexpr int ZERO2 = img_zero_base(FPB * I2::IMG), PLANE2 = ZERO2 + kImgZeroBytes;
  static constexpr int ZERO3 = img_zero_base(FPB * I3::IMG), PLANE3 = ZERO3 + kImgZeroBytes;
  static constexpr int RING2 = NP * PLANE2;
  static constexpr int EPI = p3_epi_bytes(WAVES, 32);
  static constexpr int X2 = img_zero_base(lds_max(EPI, p3_ring_bytes(64, NG3)));
  static constexpr LdsSpan x1{0, NP * PLANE2}, ring2{RING2, RING2 + p3_ring_bytes(64, NG2)};
  static constexpr LdsSpan epi{0, EPI}, x2{X2, X2 + NP * PLANE3}, ring3{0, p3_ring_bytes(64, NG3)};
  static constexpr int LDS = lds_max(ring2.hi, x2.hi);
  // Phases: conv2's k loop {x1, ring2}; its epilogue {epi, x2}; conv3's k loop {ring3, x2};
  // its epilogue {epi}.
  static constexpr bool ok() {
    return lds_disjoint(x1, ring2) && lds_disjoint(epi, x2) && lds_disjoint(ring3, x2) &&
           LDS <= 160 * 1024;
  }
};

}  // namespace gemm
}  // namespace acme
