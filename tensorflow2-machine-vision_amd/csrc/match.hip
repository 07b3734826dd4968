// Target assignment with forced matching (edet_generate_targets_matched, include/edet.h): the
// per-anchor arg-max of k_targets plus the per-ground-truth arg-max over all of an image's
// anchors, which gives every ground truth its best anchor whatever the threshold.  Bit-exact
// with k_targets' fp32 op sequence: no FMA contraction, correctly rounded division, first index
// on ties.
//
//   k_match_clear  zeroes the per-ground-truth keys (a kernel: graph-capturable everywhere)
//   k_match        the pair pass: every (anchor, ground truth) IoU of an image, the per-anchor
//                  running best in registers, the per-ground-truth best as a 64-bit key max
//   k_force        one block per image: keys -> forced anchors, lowest k wins an anchor, rewrite
//                  of the forced anchors' targets
#pragma clang fp contract(off)
#include "blockops.hpp"
#include "boxes.hpp"

#include <algorithm>

namespace edet {

constexpr int MT_THREADS = 256;  // threads of a k_match / k_force block
constexpr int MT_TILE = 128;     // ground truths staged in LDS at a time

// index of flat anchor i of image n in the [rows][A] target arrays: (pyramid row) * A + a.
// Compile-time segment indices only, so the pyramid stays in scalar registers.
__device__ __forceinline__ int64_t target_index(const edet_pyramid& p, int A, int n, int i) {
  int cnt = p.H[0] * p.W[0] * A, start = 0, sel_start = 0;
  int64_t sel_base = (int64_t)p.row_off[0] * A + (int64_t)n * cnt;
#pragma unroll
  for (int s = 1; s < EDET_MAX_SEG; ++s) {
    start += cnt;
    cnt = s < p.nseg ? p.H[s] * p.W[s] * A : 0;
    const bool in = s < p.nseg && i >= start;
    sel_start = in ? start : sel_start;
    sel_base = in ? (int64_t)p.row_off[s] * A + (int64_t)n * cnt : sel_base;
  }
  return sel_base + (i - sel_start);
}

// forced anchor of a ground truth from its key: float_bits(v) << 32 | (0xFFFFFFFF - i), 0 = none
__device__ __forceinline__ int key_anchor(u64 key) { return key ? (int)(0xFFFFFFFFu - (uint32_t)key) : -1; }

// (wave_max_u32 / wave_max_u64, the DPP reductions of the keys: blockops.hpp)
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

__global__ void k_match_clear(u64* p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT_THREADS) p[i] = 0;
}

// The pair pass.  Block = (image n, chunk of 256 * AP consecutive flat anchors); a thread owns
// the anchors base + j * 256 + tid (j < AP), so a wave's anchor loads and target stores are
// contiguous.  The image's ground truths are staged in LDS in tiles of MT_TILE (box, area, and
// the value of a pair without intersection); every lane reads the same LDS address in the k loop
// (a broadcast).  A pair whose intersection is 0 has IoU exactly 0 -- iou_tf gives 0 / uni, or 0
// by the uni == 0 rule -- unless an area is NaN (inf * 0), where iou_tf gives NaN: `zn + az.y`
// is that value, so the union and the division are skipped for almost every pair and the result
// is iou_tf's bit for bit.
//
// FORCE: per ground truth a lane folds its AP anchors' pairs with v > 0 into one key
// float_bits(v) << 32 | (0xFFFFFFFF - i): v > 0, so the bit order is the value order, and the
// complement lets the lowest i win equal values.  A wave whose ballot finds no such pair skips
// the ground truth; otherwise it reduces the keys (wave_max_u64) and lane 0 issues one 64-bit LDS
// max into the block's slot.  After the tile, thread k pushes a non-zero slot to gt_best[n][k]
// with one 64-bit global max.  Integer maxima: the result does not depend on their order.
template <int AP, bool FORCE>
__global__ __launch_bounds__(MT_THREADS) void k_match(const float* anchors, edet_pyramid p, int A, int N, int chunks,
                                                      const float* gt, const int32_t* gt_cls, const int32_t* n_gt,
                                                      int max_gt, float thr, float* box_t, int32_t* cls_t,
                                                      uint8_t* mask, u64* gt_best, int32_t* gt_anchor) {
  __shared__ float4 s_box[MT_TILE];
  __shared__ float2 s_az[MT_TILE];  // (area, value of a pair without intersection: 0, or NaN for a NaN area)
  __shared__ u64 s_key[FORCE ? MT_TILE : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = blockIdx.x / chunks, base = (blockIdx.x - n * chunks) * (MT_THREADS * AP);
  const int ng = min(max(n_gt[n], 0), max_gt);
  const float* g = gt + (size_t)n * max_gt * 4;

  float4 an[AP];
  float a1[AP], zn[AP], bv[AP];
  int best[AP];
  bool valid[AP];
#pragma unroll
  for (int j = 0; j < AP; ++j) {
    const int i = base + j * MT_THREADS + tid;
    valid[j] = i < N;
    an[j] = valid[j] ? reinterpret_cast<const float4*>(anchors)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    a1[j] = fmaxf(0.f, an[j].w - an[j].y) * fmaxf(0.f, an[j].z - an[j].x);
    zn[j] = a1[j] != a1[j] ? a1[j] : 0.f;
    bv[j] = 0.f;
    best[j] = 0;
  }

  for (int t0 = 0; t0 < ng; t0 += MT_TILE) {
    const int tn = min(MT_TILE, ng - t0);
    if (t0) __syncthreads();  // the previous tile's readers are done
    if (tid < tn) {
      const float* b = g + 4 * (t0 + tid);
      const float4 gb = make_float4(b[0], b[1], b[2], b[3]);
      const float a2 = fmaxf(0.f, gb.w - gb.y) * fmaxf(0.f, gb.z - gb.x);
      s_box[tid] = gb;
      s_az[tid] = make_float2(a2, a2 != a2 ? a2 : 0.f);
      if constexpr (FORCE) s_key[tid] = 0;
    }
    __syncthreads();
    for (int kk = 0; kk < tn; ++kk) {
      const float4 gb = s_box[kk];
      const float2 az = s_az[kk];
      const int k = t0 + kk;
      u64 key = 0;
#pragma unroll
      for (int j = 0; j < AP; ++j) {
        // iou_tf(anchor, ground truth), the areas taken from registers / LDS
        const float iy1 = fmaxf(an[j].x, gb.x), ix1 = fmaxf(an[j].y, gb.y);
        const float iy2 = fminf(an[j].z, gb.z), ix2 = fminf(an[j].w, gb.w);
        const float iw = fmaxf(0.f, ix2 - ix1), ih = fmaxf(0.f, iy2 - iy1);
        const float inter = iw * ih;
        float v;
        if (inter == 0.f) {
          v = zn[j] + az.y;
        } else {
          const float uni = (a1[j] + az.x) - inter;
          v = (uni == 0.f) ? 0.f : inter / uni;
        }
        if (k == 0 || v > bv[j]) { bv[j] = v; best[j] = k; }
        if constexpr (FORCE) {
          const uint32_t i = (uint32_t)(base + j * MT_THREADS + tid);
          if (valid[j] && v > 0.f) key = umax64(key, ((u64)__float_as_uint(v) << 32) | (0xFFFFFFFFu - i));
        }
      }
      if constexpr (FORCE) {
        if (__ballot(key != 0)) {  // wave-uniform: every lane takes part in the reduction
          key = wave_max_u64(key);
          if (lane == 0) atomicMax(&s_key[kk], key);
        }
      }
    }
    if constexpr (FORCE) {
      __syncthreads();
      if (tid < tn && s_key[tid]) atomicMax(gt_best + (size_t)n * max_gt + t0 + tid, s_key[tid]);
    }
  }

#pragma unroll
  for (int j = 0; j < AP; ++j) {
    if (!valid[j]) continue;
    const int64_t o = target_index(p, A, n, base + j * MT_THREADS + tid);
    const bool pos = ng > 0 && bv[j] >= thr;
    float4 enc = make_float4(0.f, 0.f, 0.f, 0.f);
    int cls = 0;
    if (pos) {
      enc = encode_one(an[j], g + 4 * best[j]);
      cls = gt_cls[(size_t)n * max_gt + best[j]];
    }
    reinterpret_cast<float4*>(box_t)[o] = enc;
    cls_t[o] = cls;
    mask[o] = pos ? 1 : 0;
  }
  if (!FORCE && gt_anchor && base == 0)
    for (int k = tid; k < max_gt; k += MT_THREADS) gt_anchor[(size_t)n * max_gt + k] = -1;
}

// The force pass, one block per image, after the pair pass on the same stream.  Thread k turns
// gt_best[n][k] into f_k (-1 for a zero key and for k >= n_gt) and writes gt_anchor; it then
// scans the f_j of every j < k, staged in LDS 256 at a time, for the same anchor.  A thread that
// finds none and has f_k >= 0 is the lowest k of its anchor and rewrites that anchor's targets:
// one writer per target row.  O(n_gt^2) LDS reads; more than 256 ground truths loop in rounds.
__global__ __launch_bounds__(MT_THREADS) void k_force(const float* anchors, edet_pyramid p, int A, const float* gt,
                                                      const int32_t* gt_cls, const int32_t* n_gt, int max_gt,
                                                      const u64* gt_best, float* box_t, int32_t* cls_t, uint8_t* mask,
                                                      int32_t* gt_anchor) {
  __shared__ int s_f[MT_THREADS];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int ng = min(max(n_gt[n], 0), max_gt);
  const u64* kb = gt_best + (size_t)n * max_gt;
  for (int k0 = 0; k0 < max_gt; k0 += MT_THREADS) {
    const int k = k0 + tid;
    const int fk = k < ng ? key_anchor(kb[k]) : -1;
    if (gt_anchor && k < max_gt) gt_anchor[(size_t)n * max_gt + k] = fk;
    bool first = fk >= 0;
    for (int j0 = 0; j0 <= k0 && k0 < ng; j0 += MT_THREADS) {  // block-uniform bounds
      __syncthreads();
      s_f[tid] = j0 + tid < ng ? key_anchor(kb[j0 + tid]) : -1;
      __syncthreads();
      const int lim = min(MT_THREADS, k - j0);
      if (fk >= 0)
        for (int j = 0; j < lim; ++j) first = first && s_f[j] != fk;
    }
    if (first) {
      const int64_t o = target_index(p, A, n, fk);
      reinterpret_cast<float4*>(box_t)[o] =
          encode_one(reinterpret_cast<const float4*>(anchors)[fk], gt + ((size_t)n * max_gt + k) * 4);
      cls_t[o] = gt_cls[(size_t)n * max_gt + k];
      mask[o] = 1;
    }
  }
}

// Anchors per thread of the pair pass: the largest AP that still leaves `floor` blocks, with
//   force_match != 0:  AP in {4, 2, 1}, floor  512 blocks (two per CU)
//   force_match == 0:  AP in {2, 1},    floor 2048 blocks
// Measured at D0 512x512 (49 104 anchors an image: 48 / 96 / 192 chunks at AP 4 / 2 / 1), us per
// call, median of 9 alternating windows (scripts/targets_bench.py --ap 1,2,4; spread < 1 %
// except at B = 1, G = 8, where the call is launch-bound):
//   B   G  | force 1: AP 1    AP 2    AP 4 | force 0: AP 1    AP 2    AP 4
//   32   8 |        29.17   25.38  *24.40 |        16.28  *14.78   14.95
//   32 100 |       205.05  176.56 *165.65 |       116.79 *100.11  104.09
//    8   8 |        15.27  *14.00   16.57 |        *7.25    7.30    8.60
//    8 100 |        80.01  *76.01   97.76 |       *34.53   36.60   54.82
//    1   8 |       *12.10   12.11   14.00 |        *7.16    7.15    7.18
//    1 100 |       *50.01   64.64   88.04 |       *14.26   29.27   48.42
// (* = what the rule picks.)  The forced form wants fewer, longer blocks -- every block ends in
// up to one global max per ground truth -- so its floor is lower and AP 4 pays at B = 32; the
// plain form never gained from AP 4.  Only these three block counts were measured: the floors
// sit between them, not at a measured optimum.
static int match_ap(long batch, long N, bool force) {
  if (const int f = dev_knob(62)) return f;  // development slot 62: 1, 2 or 4
  const long floor = force ? 512 : 2048;
  for (int ap = force ? 4 : 2; ap > 1; ap >>= 1)
    if (batch * ((N + MT_THREADS * ap - 1) / (MT_THREADS * ap)) >= floor) return ap;
  return 1;
}

}  // namespace edet

using namespace edet;

extern "C" int edet_generate_targets_matched(const float* anchors, const edet_pyramid* p, int A, const float* gt,
                                             const int32_t* gt_cls, const int32_t* n_gt, int max_gt, float iou_thr,
                                             float* box_t, int32_t* cls_t, uint8_t* mask, int force_match,
                                             uint64_t* gt_best, int32_t* gt_anchor, edet_stream_t stream) {
  EDET_REQUIRE(anchors && p && gt && gt_cls && n_gt && box_t && cls_t && mask && max_gt >= 1 && A > 0,
               "generate_targets_matched: bad argument");
  EDET_REQUIRE(p->nseg >= 1 && p->nseg <= EDET_MAX_SEG && p->batch >= 0, "generate_targets_matched: bad pyramid");
  EDET_REQUIRE(!force_match || gt_best, "generate_targets_matched: force_match needs the gt_best scratch");
  EDET_REQUIRE((((uintptr_t)anchors | (uintptr_t)box_t) & 15) == 0,
               "generate_targets_matched: anchors and box_t must be 16-byte aligned");
  long N = 0;
  for (int s = 0; s < p->nseg; ++s) {
    EDET_REQUIRE(p->H[s] >= 0 && p->W[s] >= 0, "generate_targets_matched: bad pyramid");
    N += (long)p->H[s] * p->W[s] * A;
  }
  const long B = p->batch;
  EDET_REQUIRE(N <= (1L << 30) && B * max_gt <= (1L << 40), "generate_targets_matched: sizes out of range");
  if (B == 0) return EDET_OK;
  const int ap = match_ap(B, N, force_match != 0);
  EDET_REQUIRE(ap == 1 || ap == 2 || ap == 4, "generate_targets_matched: anchors per thread %d", ap);
  const long chunks = std::max(1L, (N + MT_THREADS * ap - 1) / (MT_THREADS * ap));
  EDET_REQUIRE(B * chunks < (1L << 31), "generate_targets_matched: grid out of range");
  hipStream_t st = (hipStream_t)stream;
  u64* kb = (u64*)gt_best;
  if (force_match) {
    const long nk = B * max_gt;
    EDET_LAUNCH(k_match_clear, dim3((unsigned)std::min(1024L, (nk + MT_THREADS - 1) / MT_THREADS)), dim3(MT_THREADS),
                0, st, kb, (int64_t)nk);
  }
#define MATCH_LAUNCH(AP, FORCE)                                                                                    \
  EDET_LAUNCH((k_match<AP, FORCE>), dim3((unsigned)(B * chunks)), dim3(MT_THREADS), 0, st, anchors, *p, A, (int)N, \
              (int)chunks, gt, gt_cls, n_gt, max_gt, iou_thr, box_t, cls_t, mask, kb, gt_anchor)
  if (force_match) {
    if (ap == 4) MATCH_LAUNCH(4, true); else if (ap == 2) MATCH_LAUNCH(2, true); else MATCH_LAUNCH(1, true);
    EDET_LAUNCH(k_force, dim3((unsigned)B), dim3(MT_THREADS), 0, st, anchors, *p, A, gt, gt_cls, n_gt, max_gt,
                (const u64*)kb, box_t, cls_t, mask, gt_anchor);
  } else {
    if (ap == 4) MATCH_LAUNCH(4, false); else if (ap == 2) MATCH_LAUNCH(2, false); else MATCH_LAUNCH(1, false);
  }
#undef MATCH_LAUNCH
  return check_launch("edet generate_targets_matched");
}
