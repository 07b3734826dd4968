// COCO bbox AP@[.50:.95] on the device (edet_eval_match / edet_eval_sort / edet_eval_ap; the
// contract is in include/edet.h, "COCO evaluation").  Area range "all", one detection cap, no
// crowd annotations.  All arithmetic is fp64 without contraction: IEEE add / mul / div give the
// bits of a numpy restatement in the same order.
//
//   k_eval_match       one block per image, 10 waves.  Phase A, whole block: the detections' keys
//                      (class | score descending | row) sorted in LDS, the ground truths sorted
//                      by (class, index), both sets of boxes staged in that order, and an LDS
//                      table of the fp64 IoU of every same-class pair.  Phase B: wave k matches
//                      at threshold k, walking the sorted detections; lanes are strided over the
//                      class's ground truths and keep their matched flags in one register.  Then
//                      the image's slots (key with the slot in its low bits, 16-bit TP mask) and
//                      the per-class ground-truth counts (integer atomics: order-free sums).
//   k_eval_sort_chunk  LDS bitonic sort of 8192-key chunks
//   k_eval_merge       one rank-merge round: a key's place is its index in its own run plus the
//                      number of sibling-run keys before it (binary search)
//   k_eval_ap          one block per (class, threshold): the class segment by binary search, the
//                      TP total, then the segment walked from its end in 256-record chunks with a
//                      suffix count (precision / recall) and a suffix maximum (the envelope);
//                      the 101 recall steps land in LDS and are summed in a fixed order
//
// No floating-point atomics; the only atomics are integer adds and ORs whose order cannot
// reach the result.
#pragma clang fp contract(off)
#include "blockops.hpp"

#include <algorithm>

namespace edet {

constexpr int EV_T = EDET_EVAL_THRESHOLDS;     // IoU thresholds = waves of the match block's phase B
constexpr int EV_R = EDET_EVAL_RECALL_STEPS;   // recall steps
constexpr int EV_MAXM = EDET_EVAL_MAX_DETS, EV_MAXG = EDET_EVAL_MAX_GT, EV_MAXC = EDET_EVAL_MAX_CLASSES;
constexpr int EV_TABLE = EDET_EVAL_TABLE_PAIRS;  // fp64 IoUs of the pair table: 128 KiB
constexpr int EV_MATCH_THREADS = 64 * EV_T;
constexpr int EV_SLOT_BITS = 25, EV_CLASS_SHIFT = 57;
constexpr u64 EV_SLOT_MASK = (1ull << EV_SLOT_BITS) - 1ull;
constexpr u64 EV_SENTINEL = ~0ull;  // an unused slot: sorts last
constexpr int EV_CHUNK = 8192;      // keys of one LDS-sorted chunk (64 KiB)
constexpr int EV_AP_THREADS = 256;

// IoU of two (y1, x1, y2, x2) fp32 boxes: the coordinates' differences formed in fp64, areas
// unclamped, 0 unless the union is positive
__device__ __forceinline__ double eval_iou(const float4 d, const float4 g) {
  const double ih = fmax(0.0, (double)fminf(d.z, g.z) - (double)fmaxf(d.x, g.x));
  const double iw = fmax(0.0, (double)fminf(d.w, g.w) - (double)fmaxf(d.y, g.y));
  const double inter = ih * iw;
  const double ad = ((double)d.z - (double)d.x) * ((double)d.w - (double)d.y);
  const double ag = ((double)g.z - (double)g.x) * ((double)g.w - (double)g.y);
  const double uni = (ad + ag) - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}

__device__ __forceinline__ float4 load_box(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }

// Dynamic LDS: table[tcap] (fp64) | dbox[PM] | gbox[PG] (float4) | keys[PM] (8 B) | gkey[PG] (4 B);
// PM / PG the powers of two at or above M / G, tcap even.
__global__ __launch_bounds__(EV_MATCH_THREADS) void k_eval_match(
    const float* boxes, const int32_t* classes, const float* scores, const int32_t* counts, const float* gt_boxes,
    const int32_t* gt_classes, const int32_t* n_gt, int M, int G, int NC, int PM, int PG, int tcap,
    const double* iou_thr, int image0, u64* keys_out, uint16_t* tp_out, int32_t* n_gt_class) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int dstart[EV_MAXC], dend[EV_MAXC], gstart[EV_MAXC], gend[EV_MAXC], cbase[EV_MAXC];
  __shared__ uint32_t mask[EV_MAXM];
  __shared__ int s_total;
  double* table = reinterpret_cast<double*>(smem);
  float4* dbox = reinterpret_cast<float4*>(smem + (size_t)tcap * 8);
  float4* gbox = dbox + PM;
  u64* keys = reinterpret_cast<u64*>(gbox + PG);
  uint32_t* gkey = reinterpret_cast<uint32_t*>(keys + PM);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = min(max(counts[b], 0), M), ng = min(max(n_gt[b], 0), G);

  // ---- phase A: sort, stage, table
  for (int q = tid; q < PM; q += EV_MATCH_THREADS) {
    u64 k = EV_SENTINEL;
    if (q < cnt) {
      int c = classes[(size_t)b * M + q];
      if (c < 0 || c >= NC) c = 0;  // not a class: recorded with the background, never evaluated
      float s = scores[(size_t)b * M + q];
      if (s == 0.f) s = 0.f;  // -0 and +0 are one score
      k = ((u64)c << EV_CLASS_SHIFT) | ((u64)desc_bits(s) << EV_SLOT_BITS) | (u64)q;
    }
    keys[q] = k;
  }
  for (int q = tid; q < PG; q += EV_MATCH_THREADS) {
    uint32_t k = ~0u;
    if (q < ng) {
      const int c = gt_classes[(size_t)b * G + q];
      if (c >= 1 && c < NC) k = ((uint32_t)c << 10) | (uint32_t)q;
    }
    gkey[q] = k;
  }
  if (tid < EV_MAXC) { dstart[tid] = 0; dend[tid] = 0; gstart[tid] = 0; gend[tid] = 0; }
  if (tid < EV_MAXM) mask[tid] = 0;
  __syncthreads();
  bitonic_sort(keys, PM);  // class ascending, score descending, row ascending
  bitonic_sort(gkey, PG);  // class ascending, index ascending; background and padding last

  for (int q = tid; q < cnt; q += EV_MATCH_THREADS) {
    const u64 k = keys[q];
    const int c = (int)(k >> EV_CLASS_SHIFT);
    dbox[q] = load_box(boxes + ((size_t)b * M + (size_t)(k & EV_SLOT_MASK)) * 4);
    if (q == 0 || (int)(keys[q - 1] >> EV_CLASS_SHIFT) != c) dstart[c] = q;
    if (q == cnt - 1 || (int)(keys[q + 1] >> EV_CLASS_SHIFT) != c) dend[c] = q + 1;
  }
  for (int q = tid; q < ng; q += EV_MATCH_THREADS) {
    const uint32_t k = gkey[q];
    if (k == ~0u) continue;
    const int c = (int)(k >> 10);  // (the sentinel's class field matches no class)
    gbox[q] = load_box(gt_boxes + ((size_t)b * G + (k & 1023u)) * 4);
    if (q == 0 || (int)(gkey[q - 1] >> 10) != c) gstart[c] = q;
    if (q == ng - 1 || (int)(gkey[q + 1] >> 10) != c) gend[c] = q + 1;
  }
  __syncthreads();
  if (wave == 0) {  // the classes' offsets in the pair table (two classes a lane) and the counts
    const int c0 = 2 * lane, c1 = c0 + 1;
    const int g0 = c0 ? gend[c0] - gstart[c0] : 0, g1 = gend[c1] - gstart[c1];
    const int p0 = (dend[c0] - dstart[c0]) * g0, p1 = (dend[c1] - dstart[c1]) * g1;
    int inc = p0 + p1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      inc += (lane >= o) ? t : 0;
    }
    cbase[c0] = inc - p0 - p1;
    cbase[c1] = inc - p1;
    if (lane == 63) s_total = inc;
    if (g0) atomicAdd(n_gt_class + c0, g0);
    if (g1) atomicAdd(n_gt_class + c1, g1);
  }
  __syncthreads();
  const bool use_table = s_total <= tcap;  // block-uniform
  if (use_table) {
    for (int q = wave; q < cnt; q += EV_T) {
      const int c = (int)(keys[q] >> EV_CLASS_SHIFT);
      const int g0 = gstart[c], n = gend[c] - g0;
      if (c == 0 || n == 0) continue;
      const int base = cbase[c] + (q - dstart[c]) * n;
      const float4 d = dbox[q];
      for (int j = lane; j < n; j += 64) table[base + j] = eval_iou(d, gbox[g0 + j]);
    }
  }
  __syncthreads();

  // ---- phase B: wave k matches at threshold k.  Lane l owns the class's ground truths l, l + 64,
  // ...; bit s of `matched` is the flag of l + 64 s.  The winner of a detection is the largest
  // (IoU bits, index): the IoU's bits need 62 of a word's 64, so the arg-max is a 64-bit maximum
  // of the bits and then a 32-bit maximum of index + 1 among the lanes that hold it.
  {
    const double thr = fmin(iou_thr[wave], 1.0 - 1e-10);
    uint32_t matched = 0;
    int cur = -1;
    for (int q = 0; q < cnt; ++q) {
      const int c = (int)(keys[q] >> EV_CLASS_SHIFT);
      const int g0 = gstart[c], n = gend[c] - g0;
      if (c == 0 || n == 0) continue;  // wave-uniform
      if (c != cur) { cur = c; matched = 0; }
      const int base = cbase[c] + (q - dstart[c]) * n;
      const float4 d = dbox[q];
      u64 best = 0;
      uint32_t bj = 0;
      for (int s = 0, j = lane; j < n; ++s, j += 64) {
        if ((matched >> s) & 1u) continue;
        const double v = use_table ? table[base + j] : eval_iou(d, gbox[g0 + j]);
        const u64 bits = (u64)__double_as_longlong(v);
        if (v >= thr && bits >= best) { best = bits; bj = (uint32_t)j + 1u; }  // (later j wins a tie)
      }
      if (__ballot(bj != 0)) {  // wave-uniform: every lane takes part in the reductions
        const u64 top = wave_max_u64(best);
        const uint32_t w = wave_max_u32(best == top ? bj : 0u) - 1u;
        if (lane == (int)(w & 63u)) matched |= 1u << (w >> 6);
        if (lane == 0) atomicOr(&mask[q], 1u << wave);
      }
    }
  }
  __syncthreads();

  const size_t slot0 = (size_t)(image0 + b) * M;
  for (int q = tid; q < M; q += EV_MATCH_THREADS) {
    keys_out[slot0 + q] = q < cnt ? ((keys[q] & ~EV_SLOT_MASK) | (u64)(slot0 + q)) : EV_SENTINEL;
    tp_out[slot0 + q] = q < cnt ? (uint16_t)mask[q] : (uint16_t)0;
  }
}

// chunk `blockIdx.x` of keys[0, n), padded with the sentinel, sorted into out
__global__ __launch_bounds__(1024) void k_eval_sort_chunk(const u64* keys, int64_t n, u64* out) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64* s = reinterpret_cast<u64*>(smem);
  const int64_t base = (int64_t)blockIdx.x * EV_CHUNK;
  for (int t = threadIdx.x; t < EV_CHUNK; t += 1024) s[t] = base + t < n ? keys[base + t] : EV_SENTINEL;
  __syncthreads();
  bitonic_sort(s, EV_CHUNK);
  for (int t = threadIdx.x; t < EV_CHUNK; t += 1024) out[base + t] = s[t];
}

// One merge round over sorted runs of w keys (npad and w multiples of EV_CHUNK).  Real keys are
// unique, sentinels are not: a left-run key counts the sibling's keys below it, a right-run key
// those at or below it, so every key of a pair gets a place of its own.
__global__ __launch_bounds__(256) void k_eval_merge(const u64* in, u64* out, int64_t npad, int64_t w) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= npad) return;
  const int64_t pair0 = t / (2 * w) * (2 * w), idx = t - pair0;
  const bool right = idx >= w;
  const int64_t sib0 = pair0 + (right ? 0 : w);
  const u64 key = in[t];
  int64_t lo = 0, hi = min(max(npad - sib0, (int64_t)0), w);
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const u64 v = in[sib0 + mid];
    if (right ? v <= key : v < key) lo = mid + 1; else hi = mid;
  }
  out[pair0 + (right ? idx - w : idx) + lo] = key;
}

// first index of sorted[0, n) whose key is >= target
__device__ __forceinline__ int64_t key_lower_bound(const u64* sorted, int64_t n, u64 target) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// number of the recall steps at or below x
__device__ __forceinline__ int steps_upto(const double* thr, double x) {
  int lo = 0, hi = EV_R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Block (class c, threshold k).  Record i of the class's nd records (score descending) has
// tp_i = T - (TPs after i), precision tp_i / ((i + 1) + eps), recall tp_i / n, and the envelope
// is the suffix maximum of the precision; the segment is walked from its end, 256 records at a
// time, carrying the TPs and the maximum of the chunks already seen.  Record i owns the recall
// steps in (recall_{i-1}, recall_i] (record 0: from step 0) and stores its envelope there.
__global__ __launch_bounds__(EV_AP_THREADS) void k_eval_ap(const u64* sorted, int64_t n, const uint16_t* tp,
                                                           const int32_t* n_gt_class, const double* rec_thr,
                                                           double* ap, double* ar) {
  constexpr int NW = EV_AP_THREADS / 64;
  __shared__ double q[EV_R], thr[EV_R];
  __shared__ int64_t seg[2];
  __shared__ int wsum[2][NW];
  __shared__ double wmax[2][NW];
  const int c = blockIdx.x / EV_T, k = blockIdx.x - c * EV_T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ngt = n_gt_class[c];
  if (c == 0 || ngt <= 0) {  // block-uniform: background, or a class without ground truths
    if (tid == 0) { ap[blockIdx.x] = -1.0; ar[blockIdx.x] = -1.0; }
    return;
  }
  if (tid < EV_R) { q[tid] = 0.0; thr[tid] = rec_thr[tid]; }
  if (tid < 2) {
    const int cc = c + tid;
    seg[tid] = key_lower_bound(sorted, n, cc >= EV_MAXC ? EV_SENTINEL : (u64)cc << EV_CLASS_SHIFT);
  }
  __syncthreads();
  const u64* rec = sorted + seg[0];
  const int nd = (int)(seg[1] - seg[0]);

  int T = 0;
  for (int i = tid; i < nd; i += EV_AP_THREADS) T += (tp[rec[i] & EV_SLOT_MASK] >> k) & 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) T += __shfl_xor(T, o, 64);
  if (lane == 0) wsum[0][wave] = T;
  __syncthreads();
  T = (wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3]);
  __syncthreads();

  const double eps = 0x1p-52, dn = (double)ngt;
  const uint64_t above = (~0ull << lane) << 1;  // the lanes after this one
  int after = 0;       // TPs of the chunks already walked
  double carry = 0.0;  // their largest precision (precisions are >= 0)
  for (int ch = (nd + EV_AP_THREADS - 1) / EV_AP_THREADS - 1, r = 1; ch >= 0; --ch, r ^= 1) {
    const int i = ch * EV_AP_THREADS + tid;
    const bool valid = i < nd;
    const int bit = valid ? (tp[rec[i] & EV_SLOT_MASK] >> k) & 1 : 0;
    const uint64_t bal = __ballot(bit);
    if (lane == 0) wsum[r][wave] = __popcll(bal);
    __syncthreads();
    int suf = __popcll(bal & above), tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int t = wsum[r][w];
      suf += (w > wave) ? t : 0;
      tot += t;
    }
    const int tpi = T - after - suf;
    const double pr = valid ? (double)tpi / ((double)(i + 1) + eps) : 0.0;
    double env = pr;  // suffix maximum: wave, block, earlier chunks
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double t = __shfl_down(env, o, 64);
      env = (lane + o < 64) ? fmax(env, t) : env;
    }
    if (lane == 0) wmax[r][wave] = env;
    __syncthreads();
    double all = carry;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const double t = wmax[r][w];
      env = (w > wave) ? fmax(env, t) : env;
      all = fmax(all, t);
    }
    env = fmax(env, carry);
    if (valid && (bit || i == 0)) {
      const int r1 = steps_upto(thr, (double)tpi / dn);
      for (int s = i == 0 ? 0 : steps_upto(thr, (double)(tpi - bit) / dn); s < r1; ++s) q[s] = env;
    }
    carry = all;
    after += tot;
  }
  __syncthreads();
  if (wave == 0) {  // the 101 steps in a fixed order
    double v = q[lane] + (lane + 64 < EV_R ? q[lane + 64] : 0.0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) {
      ap[blockIdx.x] = v / (double)EV_R;
      ar[blockIdx.x] = (double)T / dn;
    }
  }
}

static int64_t eval_pad(int64_t n) { return (n + EV_CHUNK - 1) / EV_CHUNK * EV_CHUNK; }

static int set_lds(const void* fn, size_t lds, const char* what) {
  if (lds <= 48 * 1024) return EDET_OK;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) return EDET_OK;
  set_error("%s: %zu bytes of LDS: %s", what, lds, hipGetErrorString(e));
  return EDET_EHIP;
}

}  // namespace edet

using namespace edet;

extern "C" {

int edet_eval_match(const float* boxes, const int32_t* classes, const float* scores, const int32_t* counts,
                    const float* gt_boxes, const int32_t* gt_classes, const int32_t* n_gt, int batch, int M, int G,
                    int NC, const double* iou_thr, int image0, int capacity_images, int table_pairs, uint64_t* keys,
                    uint16_t* tp, int32_t* n_gt_class, edet_stream_t stream) {
  EDET_REQUIRE(boxes && classes && scores && counts && gt_boxes && gt_classes && n_gt && iou_thr && keys && tp &&
                   n_gt_class,
               "eval_match: null argument");
  EDET_REQUIRE(M >= 1 && M <= EV_MAXM, "eval_match: M %d outside 1..%d detections an image", M, EV_MAXM);
  EDET_REQUIRE(G >= 1 && G <= EV_MAXG, "eval_match: G %d outside 1..%d ground truths an image", G, EV_MAXG);
  EDET_REQUIRE(NC >= 2 && NC <= EV_MAXC, "eval_match: NC %d outside 2..%d (class 0 is background, 7 key bits)", NC,
               EV_MAXC);
  EDET_REQUIRE(capacity_images >= 0 && (int64_t)capacity_images * M <= (1ll << EV_SLOT_BITS),
               "eval_match: capacity %d images x %d slots exceeds 2^%d, the key's slot field", capacity_images, M,
               EV_SLOT_BITS);
  EDET_REQUIRE(batch >= 0 && image0 >= 0 && (int64_t)image0 + batch <= capacity_images,
               "eval_match: capacity overflow, images %d..%lld of %d", image0, (long long)image0 + batch,
               capacity_images);
  EDET_REQUIRE(table_pairs >= -1 && table_pairs <= EV_TABLE, "eval_match: table_pairs %d outside -1..%d", table_pairs,
               EV_TABLE);
  if (batch == 0) return EDET_OK;
  int PM = 2, PG = 2;
  while (PM < M) PM <<= 1;
  while (PG < G) PG <<= 1;
  // the table never needs more than M * G pairs; an even count keeps the boxes 16-byte aligned
  int tcap = table_pairs < 0 ? EV_TABLE : table_pairs;
  tcap = (int)std::min<int64_t>(tcap, (int64_t)M * G);
  tcap = (tcap + 1) & ~1;
  const size_t lds = (size_t)tcap * 8 + (size_t)(PM + PG) * 16 + (size_t)PM * 8 + (size_t)PG * 4;
  EDET_REQUIRE(lds <= 156 * 1024, "eval_match: %zu bytes of LDS, a block has 160 KiB", lds);  // (static: 3.5 KiB)
  if (const int rc = set_lds(reinterpret_cast<const void*>(&k_eval_match), lds, "eval_match")) return rc;
  EDET_LAUNCH(k_eval_match, dim3((unsigned)batch), dim3(EV_MATCH_THREADS), lds, (hipStream_t)stream, boxes, classes,
              scores, counts, gt_boxes, gt_classes, n_gt, M, G, NC, PM, PG, tcap, iou_thr, image0, (u64*)keys, tp,
              n_gt_class);
  return check_launch("edet eval_match");
}

int edet_eval_sort(const uint64_t* keys, int64_t n, uint64_t* scratch, edet_stream_t stream) {
  EDET_REQUIRE(keys && scratch, "eval_sort: null argument");
  EDET_REQUIRE(n >= 0 && n <= (1ll << EV_SLOT_BITS), "eval_sort: %lld keys outside 0..2^%d", (long long)n,
               EV_SLOT_BITS);
  if (n == 0) return EDET_OK;
  const int64_t npad = eval_pad(n);
  int rounds = 0;
  for (int64_t w = EV_CHUNK; w < npad; w <<= 1) ++rounds;
  // the buffers alternate per round; the chunks start in the one that leaves the result in front
  u64 *a = (u64*)scratch + (rounds & 1 ? npad : 0), *b = (u64*)scratch + (rounds & 1 ? 0 : npad);
  const hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)EV_CHUNK * 8;
  if (const int rc = set_lds(reinterpret_cast<const void*>(&k_eval_sort_chunk), lds, "eval_sort")) return rc;
  EDET_LAUNCH(k_eval_sort_chunk, dim3((unsigned)(npad / EV_CHUNK)), dim3(1024), lds, st, (const u64*)keys, n, a);
  for (int64_t w = EV_CHUNK; w < npad; w <<= 1) {
    EDET_LAUNCH(k_eval_merge, dim3((unsigned)(npad / 256)), dim3(256), 0, st, (const u64*)a, b, npad, w);
    std::swap(a, b);
  }
  return check_launch("edet eval_sort");
}

int edet_eval_ap(const uint64_t* sorted, int64_t n, const uint16_t* tp, const int32_t* n_gt_class, int NC,
                 const double* rec_thr, double* ap, double* ar, edet_stream_t stream) {
  EDET_REQUIRE(sorted && tp && n_gt_class && rec_thr && ap && ar, "eval_ap: null argument");
  EDET_REQUIRE(NC >= 2 && NC <= EV_MAXC, "eval_ap: NC %d outside 2..%d", NC, EV_MAXC);
  EDET_REQUIRE(n >= 0 && n <= (1ll << EV_SLOT_BITS), "eval_ap: %lld records outside 0..2^%d", (long long)n,
               EV_SLOT_BITS);
  EDET_LAUNCH(k_eval_ap, dim3((unsigned)(NC * EV_T)), dim3(EV_AP_THREADS), 0, (hipStream_t)stream,
              (const u64*)sorted, n, tp, n_gt_class, rec_thr, ap, ar);
  return check_launch("edet eval_ap");
}

}  // extern "C"
