// Box arithmetic shared by csrc/anchors.hip and csrc/detect.hip: overlap measures, the decode
// of one anchor's regression and the flat-candidate lookup.  One definition each, so the
// reference-faithful path and the per-class path cannot drift apart.  Bit-exact with the
// reference's fp32 op sequence: every including file compiles these without FMA contraction.
#pragma once
#pragma clang fp contract(off)
#include <math.h>
#include "common.hpp"

namespace edet {

__device__ __forceinline__ float iou_tf(const float* b1, const float* b2) {
  const float zero = 0.f;
  const float b1_w = fmaxf(zero, b1[3] - b1[1]), b1_h = fmaxf(zero, b1[2] - b1[0]);
  const float b2_w = fmaxf(zero, b2[3] - b2[1]), b2_h = fmaxf(zero, b2[2] - b2[0]);
  const float a1 = b1_w * b1_h, a2 = b2_w * b2_h;
  const float iy1 = fmaxf(b1[0], b2[0]), ix1 = fmaxf(b1[1], b2[1]);
  const float iy2 = fminf(b1[2], b2[2]), ix2 = fminf(b1[3], b2[3]);
  const float iw = fmaxf(zero, ix2 - ix1), ih = fmaxf(zero, iy2 - iy1);
  const float inter = iw * ih;
  const float uni = (a1 + a2) - inter;
  return (uni == 0.f) ? 0.f : inter / uni;  // divide_no_nan
}

// iou_tf in fp64, the same op order and the same uni == 0 -> 0 rule (Soft-NMS, detect.hip)
__device__ __forceinline__ double iou_tf64(const double* b1, const double* b2) {
  const double zero = 0.0;
  const double b1_w = fmax(zero, b1[3] - b1[1]), b1_h = fmax(zero, b1[2] - b1[0]);
  const double b2_w = fmax(zero, b2[3] - b2[1]), b2_h = fmax(zero, b2[2] - b2[0]);
  const double a1 = b1_w * b1_h, a2 = b2_w * b2_h;
  const double iy1 = fmax(b1[0], b2[0]), ix1 = fmax(b1[1], b2[1]);
  const double iy2 = fmin(b1[2], b2[2]), ix2 = fmin(b1[3], b2[3]);
  const double iw = fmax(zero, ix2 - ix1), ih = fmax(zero, iy2 - iy1);
  const double inter = iw * ih;
  const double uni = (a1 + a2) - inter;
  return (uni == 0.0) ? 0.0 : inter / uni;  // divide_no_nan
}

// DIoU of b1 (the kept box) and b2 in get_iou's op order: iou - |c2 - c1|^2 / diag^2 with
// the norms taken as sqrt(sum of squares) and squared again, divide_no_nan for both ratios
__device__ __forceinline__ float diou_tf(const float* b1, const float* b2) {
  const float iou = iou_tf(b1, b2);
  const float eymin = fminf(b1[0], b2[0]), exmin = fminf(b1[1], b2[1]);
  const float eymax = fmaxf(b1[2], b2[2]), exmax = fmaxf(b1[3], b2[3]);
  const float c1y = (b1[0] + b1[2]) / 2.0f, c1x = (b1[1] + b1[3]) / 2.0f;
  const float c2y = (b2[0] + b2[2]) / 2.0f, c2x = (b2[1] + b2[3]) / 2.0f;
  const float dy = c2y - c1y, dx = c2x - c1x;
  const float e = sqrtf(dy * dy + dx * dx);
  const float ey = eymax - eymin, ex = exmax - exmin;
  const float d = sqrtf(ey * ey + ex * ex);
  const float e2 = e * e, d2 = d * d;
  return iou - ((d2 == 0.f) ? 0.f : e2 / d2);
}

// Anchors._boxes_decoder (anchors.py:245-274) for one (pyramid row, anchor): `an` the anchor's
// (y1, x1, y2, x2), `rc` its four regressions [ty, tx, th, tw], `o` the decoded box
template <typename T>
__device__ __forceinline__ void decode_one(const float* an, const T* rc, float* o) {
  const float ty = to_f<T>(rc[0]), tx = to_f<T>(rc[1]), th = to_f<T>(rc[2]), tw = to_f<T>(rc[3]);
  const float ycenter_a = (an[2] + an[0]) / 2.0f, xcenter_a = (an[3] + an[1]) / 2.0f;
  const float ha = an[2] - an[0], wa = an[3] - an[1];
  const float w = expf(tw) * wa;
  const float h = expf(th) * ha;
  const float yc = ty * ha + ycenter_a;
  const float xc = tx * wa + xcenter_a;
  o[0] = yc - h / 2.0f;
  o[1] = xc - w / 2.0f;
  o[2] = yc + h / 2.0f;
  o[3] = xc + w / 2.0f;
}

// Anchors._boxes_encoder (anchors.py:219-243) for one (anchor, ground truth) pair, k_targets' op
// sequence: returns [ty, tx, th, tw] (csrc/match.hip: the pair pass and the force pass)
__device__ __forceinline__ float4 encode_one(const float4 an, const float* gb) {
  const float ycenter_a = (an.z + an.x) / 2.0f, xcenter_a = (an.w + an.y) / 2.0f;
  float ha = an.z - an.x, wa = an.w - an.y;
  const float ycenter = (gb[2] + gb[0]) / 2.0f, xcenter = (gb[3] + gb[1]) / 2.0f;
  float h = gb[2] - gb[0], w = gb[3] - gb[1];
  const float eps = 1e-8f;
  ha = fmaxf(eps, ha); wa = fmaxf(eps, wa); h = fmaxf(eps, h); w = fmaxf(eps, w);
  return make_float4((ycenter - ycenter_a) / ha, (xcenter - xcenter_a) / wa, logf(h / ha), logf(w / wa));
}

// flat candidate index within one image (levels concatenated, each [H][W][A]) -> pyramid row
// and anchor
__device__ __forceinline__ void cand_locate(const edet_pyramid& p, int A, int n, int i, int64_t& row, int& a) {
  int seg = 0, r = i;
  for (; seg < p.nseg - 1; ++seg) {
    const int cnt = p.H[seg] * p.W[seg] * A;
    if (r < cnt) break;
    r -= cnt;
  }
  a = r % A;
  row = (int64_t)p.row_off[seg] + (int64_t)n * p.H[seg] * p.W[seg] + r / A;
}

}  // namespace edet
