// Detection loss: sigmoid focal loss (losses/focal_loss.py:26-52) + Huber box loss
// (losses/box_loss.py:21-30) summed as in EfficientDetNetTrain._get_loss
// (efficientnet/efficientdet_net_train.py:41-52), forward and backward in one pass.
//
// Per level l (segment of the pyramid), with N+ = sum(masks) + 1 over the batch:
//   focal_l = sum FL / (N+ * B*H_l*W_l*A*NC)      (FL / normalizer, then Keras
//                                                  SUM_OVER_BATCH_SIZE = mean over elements)
//   box_l   = sum huber(pred - t) * [t != 0] / (4 N+)
//   loss   += box_weight * box_l + focal_l
// The one-hot class target of the reference (anchors.py:133) is represented by its index.
#include <float.h>
#include "common.hpp"

namespace edet {

constexpr int LCLS_ROWS = 32;  // rows per classification block (8 / 16 / 32 / 64: 363 / 197 / 191 / 200 us)
constexpr int LBOX_ROWS = 256;

struct LossArgs {
  const void* cls;
  const void* box;
  const int32_t* cls_t;
  const float* box_t;
  const float* npos;
  void* dcls;
  void* dbox;
  float* loss;
  float* parts;
  edet_pyramid p;
  int ldc, ldb, A, NC;
  float alpha, gamma, delta, box_weight, count_scale;
  int nb_cls;
};

__device__ __forceinline__ float block_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// focal loss value and d/dx for one logit (focal_loss.py:42-52, TF sigmoid CE formulation)
__device__ __forceinline__ void focal_elem(float x, float y, float alpha, float gamma, bool g15, float& fl, float& dfl) {
  // v_rcp_f32 / v_sqrt_f32 (1 ulp) instead of the correctly rounded division and square root
  // the build flags select for '/' and sqrtf: this kernel is VALU-bound over 127 M logits
  const float z = __expf(-fabsf(x));
  const float r = __builtin_amdgcn_rcpf(1.f + z);
  const float p = x >= 0.f ? r : z * r;                  // sigmoid(x)
  const float pt = y * p + (1.f - y) * (1.f - p);
  const float at = y * alpha + (1.f - y) * (1.f - alpha);
  const float om = fmaxf(1.f - pt, 0.f);
  float mod, dmodf;                                      // (1-pt)^g and g*(1-pt)^(g-1)
  if (g15) {
    const float sq = __builtin_amdgcn_sqrtf(om);
    mod = om * sq;
    dmodf = 1.5f * sq;
  } else {
    const float lg = __logf(om);
    mod = om > 0.f ? __expf(gamma * lg) : 0.f;
    dmodf = om > 0.f ? gamma * __expf((gamma - 1.f) * lg) : 0.f;
  }
  const float ce = fmaxf(x, 0.f) - x * y + __logf(1.f + z);
  const float dpt = (2.f * y - 1.f) * p * (1.f - p);
  fl = at * mod * ce;
  dfl = at * (-dmodf * dpt * ce + mod * (p - y));
}

// gamma = 1.5 with a 0/1 target, branch-free and cancellation-free (same value as focal_elem):
// with z = exp(-|x|), r = 1/(1+z): sigmoid = x >= 0 ? r : z r, and
//   q  = 1 - pt = (x >= 0) != y ? r : z r           (the modulating base, exact)
//   ce = log(1+z) + max(y ? -x : x, 0)
//   p (1-p) = z r^2,   p - y = (y ? -1 : 1) q,   dpt = -(y ? -1 : 1) p (1-p)
//   fl  = at q^1.5 ce
//   dfl = at (y ? -1 : 1) sqrt(q) (1.5 p (1-p) ce + q^2)
// kpos / kneg fold at * sign * (1 / normaliser) for y = 1 / y = 0.
// Three transcendentals per logit instead of four (round 6): with h = exp(-|x|/2) and
// s = rsqrt(1 + h^2), z = h^2, r = s^2, sqrt(r) = s, sqrt(z r) = h s and log(1+z) = -2 log(s),
// so the sigmoid's reciprocal and the modulating square root come from one v_rsq_f32
__device__ __forceinline__ void focal_elem15(float x, bool y, float apos, float aneg, float kpos, float kneg,
                                             float& fl, float& dfl) {
  const float h = __builtin_amdgcn_exp2f(fabsf(x) * -0.72134752044448170f);  // exp(-|x|/2)
  const float z = h * h;
  const float s = __builtin_amdgcn_rsqf(1.f + z);
  const float r = s * s;
  const float zr = z * r;
  const bool flip = (x >= 0.f) != y;
  const float q = flip ? r : zr;
  const float sq = flip ? s : h * s;
  const float ce = fmaf(-1.3862943611198906f, __builtin_amdgcn_logf(s), fmaxf(y ? -x : x, 0.f));
  fl = (y ? apos : aneg) * q * sq * ce;
  dfl = (y ? kpos : kneg) * sq * fmaf(1.5f * zr * r, ce, q * q);
}

// Two logits at a time in packed fp32 (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32: the
// multiplies of focal_elem15 on both lanes of a pair in one instruction; the transcendentals and
// selects stay scalar).  Same formula as focal_elem15.
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void focal_pair15(f2v x, bool y0, bool y1, float apos, float aneg, float kpos, float kneg,
                                             f2v& fl, f2v& dfl) {
  const f2v t = f2v{fabsf(x.x), fabsf(x.y)} * -0.72134752044448170f;
  const f2v h = f2v{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
  const f2v z = h * h;
  const f2v z1 = z + 1.f;
  const f2v sv = f2v{__builtin_amdgcn_rsqf(z1.x), __builtin_amdgcn_rsqf(z1.y)};
  const f2v r = sv * sv;
  const f2v zr = z * r;
  const f2v hs = h * sv;
  const bool fl0 = (x.x >= 0.f) != y0, fl1 = (x.y >= 0.f) != y1;
  const f2v q = f2v{fl0 ? r.x : zr.x, fl1 ? r.y : zr.y};
  const f2v sq = f2v{fl0 ? sv.x : hs.x, fl1 ? sv.y : hs.y};
  const f2v lg = f2v{__builtin_amdgcn_logf(sv.x), __builtin_amdgcn_logf(sv.y)};
  const f2v mx = f2v{fmaxf(y0 ? -x.x : x.x, 0.f), fmaxf(y1 ? -x.y : x.y, 0.f)};
  const f2v ce = lg * -1.3862943611198906f + mx;
  const f2v a = f2v{y0 ? apos : aneg, y1 ? apos : aneg};
  const f2v k = f2v{y0 ? kpos : kneg, y1 ? kpos : kneg};
  fl = a * q * sq * ce;
  dfl = k * sq * ((zr * r * 1.5f) * ce + q * q);
}

template <typename T>
__global__ __launch_bounds__(256) void k_loss(LossArgs g) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const float npos = *g.npos + 1.f;
  const bool g15 = g.gamma == 1.5f;
  int b = blockIdx.x;
  if (b < g.nb_cls) {
    int seg, chunk;
    chunk_lookup(g.p, LCLS_ROWS, b, seg, chunk);
    const int rows = seg_rows(g.p, seg);
    const int m0 = g.p.row_off[seg] + chunk * LCLS_ROWS;
    const int nr = min(LCLS_ROWS, g.p.row_off[seg] + rows - m0);
    const int AN = g.A * g.NC;
    const float inv = 1.f / (npos * (float)rows * (float)AN * g.count_scale);
    T* X = (T*)g.cls;  // logits; gradient written in place when dcls == cls
    T* D = (T*)g.dcls;
    float s = 0.f;
    if (g15 && g.NC >= 8 && (g.ldc & 7) == 0 && D == X && sizeof(T) == 2) {
      // the training path (gamma = 1.5, bf16 logits, gradient in place): the thread's vectors
      // walked incrementally (no division per vector), a vector's positives as two column
      // indices (NC >= 8: it spans at most two anchors), the logits in packed pairs
      const int nvec = g.ldc / 8, step_r = 256 / nvec, step_v = 256 - step_r * nvec;
      const float invNC = 1.f / (float)g.NC;
      const float apos = g.alpha, aneg = 1.f - g.alpha, kpos = -g.alpha * inv, kneg = (1.f - g.alpha) * inv;
      int r = tid / nvec, vi = tid - r * nvec;
      while (r < nr) {
        const int cv = vi * 8, m = m0 + r;
        T* px = X + (size_t)m * g.ldc + cv;
        float x[8], d[8];
        ld8(px, x);
        const int32_t* tr = g.cls_t + (size_t)m * g.A;
        const int a0 = (int)(((float)cv + 0.5f) * invNC);  // exact for cv < 2^20
        // a0 >= A in a vector that lies wholly in the pad columns (ldc >= roundup8(A*NC) + 8)
        const int ta = (a0 < g.A) ? tr[a0] : -1, tb = (a0 + 1 < g.A) ? tr[a0 + 1] : -1;
        const int p0 = (ta >= 0 && ta < g.NC) ? a0 * g.NC + ta : -1;
        const int p1 = (tb >= 0 && tb < g.NC) ? (a0 + 1) * g.NC + tb : -1;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const int c0 = cv + j, c1 = c0 + 1;
          f2v fl, dfl;
          focal_pair15(f2v{x[j], x[j + 1]}, c0 == p0 || c0 == p1, c1 == p0 || c1 == p1, apos, aneg, kpos, kneg,
                       fl, dfl);
          const bool v0 = c0 < AN, v1 = c1 < AN;
          d[j] = v0 ? dfl.x : 0.f;
          d[j + 1] = v1 ? dfl.y : 0.f;
          s += (v0 ? fl.x : 0.f) + (v1 ? fl.y : 0.f);
        }
        st8(px, d);
        // next vector of this thread (256 further): no division per vector
        vi += step_v;
        r += step_r;
        if (vi >= nvec) { vi -= nvec; ++r; }
      }
      // (two vectors in flight per trip measured the same, r06ab: 166.8 -> 162.1 us against
      // 160.8 -> 156.9 for this form, r06aa)
    } else if ((g.ldc & 7) == 0 && (!D || D == X)) {
      const int nvec = g.ldc / 8;
      for (int e = tid; e < nr * nvec; e += 256) {
        const int r = e / nvec, cv = (e - r * nvec) * 8;
        const int m = m0 + r;
        T* px = X + (size_t)m * g.ldc + cv;
        float x[8], d[8];
        ld8(px, x);
        const int32_t* tr = g.cls_t + (size_t)m * g.A;
        // (anchor, class) of the vector's first column; the next 7 step without a division
        // and, with NC >= 8, stay within two anchors whose targets are read once
        const int a0 = cv / g.NC;
        int a = a0, c = cv - a0 * g.NC;
        // (a0 >= A in a vector that lies wholly in the pad columns)
        const int ta = (a0 < g.A) ? tr[a0] : -1, tb = (a0 + 1 < g.A) ? tr[a0 + 1] : -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int col = cv + j;
          d[j] = 0.f;
          if (j > 0 && ++c == g.NC) { c = 0; ++a; }
          if (col < AN) {
            const bool yb = (g.NC >= 8 ? (a == a0 ? ta : tb) : tr[a]) == c;
            float fl, dfl;
            if (g15) {
              focal_elem15(x[j], yb, g.alpha, 1.f - g.alpha, -g.alpha * inv, (1.f - g.alpha) * inv, fl, dfl);
              d[j] = dfl;
            } else {
              focal_elem(x[j], yb ? 1.f : 0.f, g.alpha, g.gamma, g15, fl, dfl);
              d[j] = dfl * inv;
            }
            s += fl;
          }
        }
        if (D) st8(px, d);
      }
    } else {  // generic strides / separate gradient buffer
      for (int e = tid; e < nr * AN; e += 256) {
        const int r = e / AN, col = e - r * AN;
        const int m = m0 + r;
        const int a = col / g.NC, c = col - a * g.NC;
        const float x = to_f<T>(X[(size_t)m * g.ldc + col]);
        const float y = (g.cls_t[(size_t)m * g.A + a] == c) ? 1.f : 0.f;
        float fl, dfl;
        focal_elem(x, y, g.alpha, g.gamma, g15, fl, dfl);
        s += fl;
        if (D) D[(size_t)m * g.ldc + col] = from_f<T>(dfl * inv);
      }
      if (D && g.ldc > AN) {
        const int pad = g.ldc - AN;
        for (int e = tid; e < nr * pad; e += 256) {
          const int r = e / pad;
          D[(size_t)(m0 + r) * g.ldc + AN + (e - r * pad)] = from_f<T>(0.f);
        }
      }
    }
    s = block_sum(s, red);
    if (tid == 0) {
      atomicAdd(g.loss, s * inv);
      if (g.parts) atomicAdd(g.parts + seg, s * inv);
    }
    return;
  }
  b -= g.nb_cls;
  int seg, chunk;
  chunk_lookup(g.p, LBOX_ROWS, b, seg, chunk);
  const int rows = seg_rows(g.p, seg);
  const int m0 = g.p.row_off[seg] + chunk * LBOX_ROWS;
  const int nr = min(LBOX_ROWS, g.p.row_off[seg] + rows - m0);
  const int A4 = g.A * 4;
  const float inv = 1.f / (4.f * npos);
  T* P = (T*)g.box;
  T* D = (T*)g.dbox;
  const float dl = g.delta;
  float s = 0.f;
  for (int e = tid; e < nr * A4; e += 256) {
    const int r = e / A4, col = e - r * A4;
    const int m = m0 + r;
    const float t = g.box_t[(size_t)m * A4 + col];
    const float pr = to_f<T>(P[(size_t)m * g.ldb + col]);
    const float mask = (t != 0.f) ? 1.f : 0.f;
    const float err = pr - t, ae = fabsf(err);
    const float h = (ae <= dl) ? 0.5f * err * err : 0.5f * dl * dl + dl * (ae - dl);
    s += h * mask;
    if (D) {
      const float dh = (ae <= dl) ? err : (err > 0.f ? dl : -dl);
      D[(size_t)m * g.ldb + col] = from_f<T>(dh * mask * inv * g.box_weight);
    }
  }
  if (D && g.ldb > A4) {
    const int pad = g.ldb - A4;
    for (int e = tid; e < nr * pad; e += 256) {
      const int r = e / pad;
      D[(size_t)(m0 + r) * g.ldb + A4 + (e - r * pad)] = from_f<T>(0.f);
    }
  }
  s = block_sum(s, red);
  if (tid == 0) {
    atomicAdd(g.loss, s * inv * g.box_weight);
    if (g.parts) atomicAdd(g.parts + EDET_MAX_SEG + seg, s * inv);
  }
}

// ------------------------------------------------------------------ box branch with an IoU term
// edet_detection_loss_iou: Huber as in k_loss's box blocks plus an IoU-family loss on the
// decoded boxes of the positive anchors (include/edet.h has the definition).  The predictions
// are overwritten by their gradient, so both terms come from the same loaded values and their
// summed gradient is stored once.
//
// Work split.  A block owns one LBOX_ROWS chunk of a level, a thread owns whole anchors: the four
// regressions as one 8-byte (bf16) or 16-byte (f32) vector, the four targets as one float4, the
// mask byte.  Positives are well under 1 % of the anchors in training, so the IoU arithmetic
// (about 150 VALU instructions, an exp pair, divisions) would run at one or two live lanes per
// wave if each owner did its own.  Instead:
//   phase 1  every thread walks its anchors: Huber value and gradient in registers; a
//            non-positive anchor's gradient is stored at once.  Each wave ballots its positives
//            and appends them (slot, predictions, targets) to its own IOU_WCAP-entry region of an
//            LDS list -- a wave-private counter, no atomics, no barrier, a fixed order.
//   barrier  one __syncthreads per block.
//   phase 2  the four regions are walked as one dense list, one lane per positive: the lane
//            recomputes the entry's Huber gradient (the same function, the same bits), adds the
//            IoU gradient in fp32 and does the anchor's single vector store.
// A positive that finds its wave's region full (dense synthetic masks; training never gets
// near) is handled by its owner in phase 1 with the same arithmetic.
constexpr int IOU_WCAP = 64;
constexpr float BOX_CLIP = 4.135166556742356f;  // log(1000 / 16)

struct BoxIouArgs {
  const void* box;
  const float* box_t;
  const float* npos;
  const float* anchors;
  const uint8_t* mask;
  void* dbox;
  float* loss;
  float* parts;
  float* iou_parts;
  edet_pyramid p;
  int ldb, A;
  float delta, box_weight, iou_weight;
  int vec;
};

// four contiguous elements -> fp32; vec: the pointer is aligned for one vector access
__device__ __forceinline__ void ld4(const float* p, bool vec, float* o) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = p[j];
  }
}
__device__ __forceinline__ void ld4(const uint16_t* p, bool vec, float* o) {
  if (vec) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = bf2f(p[j]);
  }
}
__device__ __forceinline__ void st4(float* p, bool vec, const float* v) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = v[j];
  }
}
__device__ __forceinline__ void st4(uint16_t* p, bool vec, const float* v) {
  if (vec) {
    *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16),
                                              (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = f2bf(v[j]);
  }
}

// Huber of one anchor's four components in k_loss's arithmetic (the same expressions, so an
// anchor without an IoU term gets the bits edet_detection_loss writes): returns sum h * [t != 0],
// d[j] = d(box_weight * box_l) / d pred[j]
__device__ __forceinline__ float huber4(const float* p, const float* t, float dl, float inv, float bw, float* d) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float mask = (t[j] != 0.f) ? 1.f : 0.f;
    const float err = p[j] - t[j], ae = fabsf(err);
    const float h = (ae <= dl) ? 0.5f * err * err : 0.5f * dl * dl + dl * (ae - dl);
    s += h * mask;
    const float dh = (ae <= dl) ? err : (err > 0.f ? dl : -dl);
    d[j] = dh * mask * inv * bw;
  }
  return s;
}

// 1 / d, and 0 for d == 0: a ratio with a zero denominator is 0 and has no gradient
__device__ __forceinline__ float rcp0(float d) { return d == 0.f ? 0.f : 1.f / d; }

// centre / size form of an anchor's regressions (ty, tx, th, tw), th and tw clamped to +-BOX_CLIP
struct CSBox { float yc, xc, h, w; };
__device__ __forceinline__ CSBox decode_clamped(const float* r, float ha, float wa, float yca, float xca) {
  CSBox b;
  b.h = expf(fminf(fmaxf(r[2], -BOX_CLIP), BOX_CLIP)) * ha;
  b.w = expf(fminf(fmaxf(r[3], -BOX_CLIP), BOX_CLIP)) * wa;
  b.yc = r[0] * ha + yca;
  b.xc = r[1] * wa + xca;
  return b;
}

// One positive anchor: L = 1 - iou + penalty(KIND) of the decoded prediction p against the decoded
// target t, and gi[j] = dL / d p[j].  Backward by hand: the gradient is collected on the
// intersection area (gI), the predicted area (gA), the enclosing sides (gey, gex) and the
// predicted centre and size, then taken through the corners and the decode.  min / max pass
// their gradient to the predicted box where it is strictly the selected argument.
template <int KIND>
__device__ __forceinline__ float iou_term(const float* p, const float* t, const float* an, float* gi) {
  const float ha = an[2] - an[0], wa = an[3] - an[1];
  const float yca = 0.5f * (an[0] + an[2]), xca = 0.5f * (an[1] + an[3]);
  const CSBox P = decode_clamped(p, ha, wa, yca, xca), T = decode_clamped(t, ha, wa, yca, xca);
  const float py1 = P.yc - 0.5f * P.h, py2 = P.yc + 0.5f * P.h, px1 = P.xc - 0.5f * P.w, px2 = P.xc + 0.5f * P.w;
  const float ty1 = T.yc - 0.5f * T.h, ty2 = T.yc + 0.5f * T.h, tx1 = T.xc - 0.5f * T.w, tx2 = T.xc + 0.5f * T.w;
  const float dyi = fminf(py2, ty2) - fmaxf(py1, ty1), dxi = fminf(px2, tx2) - fmaxf(px1, tx1);
  const float ih = fmaxf(dyi, 0.f), iw = fmaxf(dxi, 0.f);
  const float inter = ih * iw;
  const float U = P.h * P.w + T.h * T.w - inter;
  const float rU = rcp0(U);
  const float iou = inter * rU;
  float L = 1.f - iou;
  float gI = -(U + inter) * rU * rU, gA = inter * rU * rU;  // d(-iou) / d inter, / d area(P)
  float gyc = 0.f, gxc = 0.f, gh = 0.f, gw = 0.f, gey = 0.f, gex = 0.f;
  if (KIND != EDET_IOU_LOSS_IOU) {
    const float ey = fmaxf(py2, ty2) - fminf(py1, ty1), ex = fmaxf(px2, tx2) - fminf(px1, tx1);
    if (KIND == EDET_IOU_LOSS_GIOU) {
      const float C = ey * ex, rC = rcp0(C);
      L += (C - U) * rC;  // 1 - U / C
      gI += rC;
      gA -= rC;
      gey = U * rC * rC * ex;
      gex = U * rC * rC * ey;
    } else {
      const float r2 = rcp0(ey * ey + ex * ex);
      const float dy = P.yc - T.yc, dx = P.xc - T.xc, rho2 = dy * dy + dx * dx;
      L += rho2 * r2;
      gyc = 2.f * dy * r2;
      gxc = 2.f * dx * r2;
      gey = -2.f * rho2 * r2 * r2 * ey;
      gex = -2.f * rho2 * r2 * r2 * ex;
      if (KIND == EDET_IOU_LOSS_CIOU) {
        const float k = 0.40528473456935109f;  // 4 / pi^2
        const float da = atanf(T.w * rcp0(T.h)) - atanf(P.w * rcp0(P.h));
        const float v = k * da * da;
        const float al = v * rcp0((1.f - iou) + v);  // a constant in the backward
        L += al * v;
        // d atan(w / h) = (h dw - w dh) / (h^2 + w^2)
        const float sv = P.h == 0.f ? 0.f : -2.f * k * da * al * rcp0(P.h * P.h + P.w * P.w);
        gw += sv * P.h;
        gh -= sv * P.w;
      }
    }
  }
  const float gih = dyi > 0.f ? gI * iw : 0.f, giw = dxi > 0.f ? gI * ih : 0.f;
  const float gy1 = (py1 > ty1 ? -gih : 0.f) - (py1 < ty1 ? gey : 0.f);
  const float gy2 = (py2 < ty2 ? gih : 0.f) + (py2 > ty2 ? gey : 0.f);
  const float gx1 = (px1 > tx1 ? -giw : 0.f) - (px1 < tx1 ? gex : 0.f);
  const float gx2 = (px2 < tx2 ? giw : 0.f) + (px2 > tx2 ? gex : 0.f);
  gyc += gy1 + gy2;
  gxc += gx1 + gx2;
  gh += 0.5f * (gy2 - gy1) + gA * P.w;
  gw += 0.5f * (gx2 - gx1) + gA * P.h;
  gi[0] = gyc * ha;
  gi[1] = gxc * wa;
  gi[2] = fabsf(p[2]) <= BOX_CLIP ? gh * P.h : 0.f;  // d exp(th) ha / d th; nothing through the clamp
  gi[3] = fabsf(p[3]) <= BOX_CLIP ? gw * P.w : 0.f;
  return L;
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void k_box_iou(BoxIouArgs g) {
  __shared__ float red[4];
  __shared__ float4 l_p[4 * IOU_WCAP], l_t[4 * IOU_WCAP];
  __shared__ int l_i[4 * IOU_WCAP];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float npos = *g.npos + 1.f;
  int seg, chunk;
  chunk_lookup(g.p, LBOX_ROWS, blockIdx.x, seg, chunk);
  const int rows = seg_rows(g.p, seg);
  const int m0 = g.p.row_off[seg] + chunk * LBOX_ROWS;
  const int nr = min(LBOX_ROWS, g.p.row_off[seg] + rows - m0);
  const int A = g.A, A4 = A * 4, n = nr * A;
  const int hw = g.p.H[seg] * g.p.W[seg];
  int abase = 0;  // the level's first anchor (k_decode's indexing: anchors are per image)
  for (int s = 0; s < seg; ++s) abase += g.p.H[s] * g.p.W[s] * A;
  const float inv = 1.f / (4.f * npos), kw = g.iou_weight / npos;
  const bool vec = g.vec != 0;
  const T* P = (const T*)g.box;
  T* D = (T*)g.dbox;
  // anchor of slot i of this chunk (row m0 + i / A, anchor i % A)
  auto anchor_of = [&](int r, int a) { return g.anchors + ((size_t)abase + (size_t)((m0 + r - g.p.row_off[seg]) % hw) * A + a) * 4; };
  float hs = 0.f, ls = 0.f;
  int cnt = 0;  // this wave's positives so far (wave-uniform)
  for (int base = 0; base < n; base += 256) {
    const int i = base + tid;
    const bool valid = i < n;
    bool pos = false;
    int r = 0, a = 0;
    float p[4], t[4], d[4];
    if (valid) {
      r = i / A;
      a = i - r * A;
      const size_t m = (size_t)(m0 + r);
      ld4(P + m * g.ldb + 4 * a, vec, p);
      ld4(g.box_t + (m * A + a) * 4, vec, t);
      pos = g.mask[m * A + a] != 0;
      hs += huber4(p, t, g.delta, inv, g.box_weight, d);
    }
    bool listed = false;
    const unsigned long long bal = __ballot(pos);
    if (bal) {
      const int k = cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
      if (pos) {
        if (k < IOU_WCAP) {
          const int e = wave * IOU_WCAP + k;
          l_i[e] = i;
          l_p[e] = make_float4(p[0], p[1], p[2], p[3]);
          l_t[e] = make_float4(t[0], t[1], t[2], t[3]);
          listed = true;
        } else {
          float gi[4];
          ls += iou_term<KIND>(p, t, anchor_of(r, a), gi);
#pragma unroll
          for (int j = 0; j < 4; ++j) d[j] += kw * gi[j];
        }
      }
      cnt += __popcll(bal);
    }
    if (valid && D && !listed) st4(D + (size_t)(m0 + r) * g.ldb + 4 * a, vec, d);
  }
  if (lane == 0) wcnt[wave] = cnt;
  __syncthreads();
  const bool any = (wcnt[0] | wcnt[1] | wcnt[2] | wcnt[3]) != 0;  // a block without positives adds no IoU term
  const int c0 = min(wcnt[0], IOU_WCAP), c1 = c0 + min(wcnt[1], IOU_WCAP), c2 = c1 + min(wcnt[2], IOU_WCAP),
            total = c2 + min(wcnt[3], IOU_WCAP);
  for (int q = tid; q < total; q += 256) {  // total <= 4 * IOU_WCAP = 256: one trip
    const int w = (q >= c0) + (q >= c1) + (q >= c2);
    const int e = w * IOU_WCAP + q - (w == 0 ? 0 : w == 1 ? c0 : w == 2 ? c1 : c2);
    const int i = l_i[e];
    const float4 pv = l_p[e], tv = l_t[e];
    const int r = i / A, a = i - r * A;
    const float p[4] = {pv.x, pv.y, pv.z, pv.w}, t[4] = {tv.x, tv.y, tv.z, tv.w};
    float d[4], gi[4];
    huber4(p, t, g.delta, inv, g.box_weight, d);
    ls += iou_term<KIND>(p, t, anchor_of(r, a), gi);
    if (D) {
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] += kw * gi[j];
      st4(D + (size_t)(m0 + r) * g.ldb + 4 * a, vec, d);
    }
  }
  if (D && g.ldb > A4) {
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {  // ldb % 4 == 0: the pad is whole vectors
      const int pv = (g.ldb - A4) / 4;
      for (int e = tid; e < nr * pv; e += 256) {
        const int r = e / pv;
        st4(D + (size_t)(m0 + r) * g.ldb + A4 + 4 * (e - r * pv), true, z);
      }
    } else {
      const int pad = g.ldb - A4;
      for (int e = tid; e < nr * pad; e += 256) {
        const int r = e / pad;
        D[(size_t)(m0 + r) * g.ldb + A4 + (e - r * pad)] = from_f<T>(0.f);
      }
    }
  }
  hs = block_sum(hs, red);
  ls = block_sum(ls, red);
  if (tid == 0) {
    atomicAdd(g.loss, hs * inv * g.box_weight);
    if (g.parts) atomicAdd(g.parts + EDET_MAX_SEG + seg, hs * inv);
    if (any) {
      const float il = ls / npos;
      atomicAdd(g.loss, g.iou_weight * il);
      if (g.iou_parts) atomicAdd(g.iou_parts + seg, il);
    }
  }
}

// 16 mask bytes per thread and step, few blocks: the count ends in one same-address atomic
// per block (exact: integer-valued floats far below 2^24)
__global__ void k_count_pos(const uint8_t* mask, int64_t n, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  const int64_t nv = n / 16, stride = (int64_t)gridDim.x * 256;
  // four 16-byte vectors per trip, all requested before any is counted (the 64-block grid
  // walked ~6 dependent loads per thread: 14.9 us for D0's 1.6 MB of masks)
  for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < nv; i0 += 4 * stride) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = i0 + u * stride;
      v[u] = i < nv ? reinterpret_cast<const uint4*>(mask)[i] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t w4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int b = 0; b < 4; ++b) s += ((w4[k] >> (8 * b)) & 0xffu) ? 1.f : 0.f;
    }
  }
  for (int64_t i = nv * 16 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    s += mask[i] ? 1.f : 0.f;
  s = block_sum(s, red);
  if (threadIdx.x == 0) atomicAdd(out, s);
}

__global__ void k_onehot_index(const float* onehot, int64_t n, int NC, int32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = onehot + i * NC;
  int best = 0;
  float bv = p[0];
  for (int c = 1; c < NC; ++c)
    if (p[c] > bv) { bv = p[c]; best = c; }
  out[i] = best;
}

}  // namespace edet

using namespace edet;

extern "C" {

int edet_detection_loss(int dtype, const void* cls, int ldc, const void* box, int ldb,
                        const edet_pyramid* p, int A, int NC, const int32_t* cls_t,
                        const float* box_t, const float* npos_sum, float alpha, float gamma,
                        float delta, float box_weight, float focal_count_scale, void* dcls,
                        void* dbox, float* loss, float* level_parts, edet_stream_t stream) {
  EDET_REQUIRE(cls && box && p && cls_t && box_t && npos_sum && loss, "detection_loss: null argument");
  EDET_REQUIRE(ldc >= A * NC && ldb >= A * 4 && p->nseg >= 1 && p->nseg <= EDET_MAX_SEG,
               "detection_loss: bad strides");
  LossArgs g{};
  g.cls = cls; g.box = box; g.cls_t = cls_t; g.box_t = box_t; g.npos = npos_sum; g.dcls = dcls;
  g.dbox = dbox; g.loss = loss; g.parts = level_parts; g.p = *p; g.ldc = ldc; g.ldb = ldb;
  g.A = A; g.NC = NC; g.alpha = alpha; g.gamma = gamma; g.delta = delta; g.box_weight = box_weight;
  g.count_scale = focal_count_scale > 0.f ? focal_count_scale : 1.f;
  g.nb_cls = total_chunks(*p, LCLS_ROWS);
  const int nb = g.nb_cls + total_chunks(*p, LBOX_ROWS);
  EDET_DTYPE_DISPATCH(dtype, T, {
    if (nb) EDET_LAUNCH(k_loss<T>, dim3(nb), dim3(256), 0, (hipStream_t)stream, g);
    return check_launch("edet detection_loss");
  });
}

int edet_detection_loss_iou(int dtype, const void* cls, int ldc, const void* box, int ldb,
                            const edet_pyramid* p, int A, int NC, const int32_t* cls_t,
                            const float* box_t, const float* npos_sum, float alpha, float gamma,
                            float delta, float box_weight, float focal_count_scale, void* dcls,
                            void* dbox, float* loss, float* level_parts, const float* anchors,
                            const uint8_t* mask, int iou_kind, float iou_weight, float* iou_parts,
                            edet_stream_t stream) {
  EDET_REQUIRE(cls && box && p && cls_t && box_t && npos_sum && loss, "detection_loss_iou: null argument");
  EDET_REQUIRE(anchors && mask, "detection_loss_iou: null anchors or mask");
  EDET_REQUIRE(ldc >= A * NC && ldb >= A * 4 && A > 0 && p->nseg >= 1 && p->nseg <= EDET_MAX_SEG,
               "detection_loss_iou: bad strides");
  EDET_REQUIRE(iou_kind >= EDET_IOU_LOSS_IOU && iou_kind <= EDET_IOU_LOSS_CIOU,
               "detection_loss_iou: unknown iou_kind %d", iou_kind);
  EDET_REQUIRE(iou_weight >= 0.f && iou_weight <= FLT_MAX,
               "detection_loss_iou: iou_weight must be finite and >= 0");
  // the class blocks of k_loss alone (its grid puts them first), then the whole box branch
  LossArgs g{};
  g.cls = cls; g.box = box; g.cls_t = cls_t; g.box_t = box_t; g.npos = npos_sum; g.dcls = dcls;
  g.dbox = dbox; g.loss = loss; g.parts = level_parts; g.p = *p; g.ldc = ldc; g.ldb = ldb;
  g.A = A; g.NC = NC; g.alpha = alpha; g.gamma = gamma; g.delta = delta; g.box_weight = box_weight;
  g.count_scale = focal_count_scale > 0.f ? focal_count_scale : 1.f;
  g.nb_cls = total_chunks(*p, LCLS_ROWS);
  BoxIouArgs b{};
  b.box = box; b.box_t = box_t; b.npos = npos_sum; b.anchors = anchors; b.mask = mask; b.dbox = dbox;
  b.loss = loss; b.parts = level_parts; b.iou_parts = iou_parts; b.p = *p; b.ldb = ldb; b.A = A;
  b.delta = delta; b.box_weight = box_weight; b.iou_weight = iou_weight;
  const int nb_box = total_chunks(*p, LBOX_ROWS);
  const hipStream_t st = (hipStream_t)stream;
  EDET_DTYPE_DISPATCH(dtype, T, {
    // one vector per anchor: four storage elements and the float4 of targets, all aligned
    const uintptr_t va = 4 * sizeof(T) - 1;
    b.vec = ldb % 4 == 0 && !((uintptr_t)box & va) && !((uintptr_t)dbox & va) && !((uintptr_t)box_t & 15);
    if (g.nb_cls) EDET_LAUNCH(k_loss<T>, dim3(g.nb_cls), dim3(256), 0, st, g);
    if (nb_box) {
      switch (iou_kind) {
        case EDET_IOU_LOSS_IOU: EDET_LAUNCH((k_box_iou<T, EDET_IOU_LOSS_IOU>), dim3(nb_box), dim3(256), 0, st, b); break;
        case EDET_IOU_LOSS_GIOU: EDET_LAUNCH((k_box_iou<T, EDET_IOU_LOSS_GIOU>), dim3(nb_box), dim3(256), 0, st, b); break;
        case EDET_IOU_LOSS_DIOU: EDET_LAUNCH((k_box_iou<T, EDET_IOU_LOSS_DIOU>), dim3(nb_box), dim3(256), 0, st, b); break;
        default: EDET_LAUNCH((k_box_iou<T, EDET_IOU_LOSS_CIOU>), dim3(nb_box), dim3(256), 0, st, b); break;
      }
    }
    return check_launch("edet detection_loss_iou");
  });
}

int edet_count_positives(const uint8_t* mask, int64_t n, float* out, edet_stream_t stream) {
  EDET_REQUIRE(mask && out, "count_positives: null argument");
  if (n <= 0) return EDET_OK;
  EDET_REQUIRE(((uintptr_t)mask & 15) == 0, "count_positives: mask must be 16-byte aligned");
  // one trip of four vectors per thread where that takes at most 128 blocks (each block ends
  // in one fp32 atomic on the same address: integer counts, exact in any order)
  int nb = (int)((n / 16 + 1023) / 1024);
  if (nb > 128) nb = 128;
  if (nb < 1) nb = 1;
  EDET_LAUNCH(k_count_pos, dim3(nb), dim3(256), 0, (hipStream_t)stream, mask, n, out);
  return check_launch("edet count_positives");
}

int edet_onehot_to_index(const float* onehot, int64_t n, int NC, int32_t* out,
                         edet_stream_t stream) {
  EDET_REQUIRE(onehot && out && NC > 0, "onehot_to_index: bad argument");
  if (n <= 0) return EDET_OK;
  EDET_LAUNCH(k_onehot_index, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     onehot, n, NC, out);
  return check_launch("edet onehot_to_index");
}

}  // extern "C"
