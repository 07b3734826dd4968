// Per-class detection post-processing (edet_detect_per_class): the multi-label protocol of the
// published EfficientDet evaluation.  Every (anchor, class >= 1) pair whose logit reaches the
// threshold is a candidate; NMS suppresses within a class only.
//
//   k_cand_count / k_cand_write   chip-wide threshold scan of the logits with an ordered
//                                 compaction: blocks own contiguous row chunks numbered in flat
//                                 (image, level, row) order, pass 1 counts, pass 2 sums the counts
//                                 of the blocks before it and writes its survivors in place
//   k_sel_hist / k_sel_count /    EDET_SELECT_TOPK only, for images with more candidates than the
//   k_sel_write                   cap: a most-significant-digit radix select of the cap-th best
//                                 logit key over the same grid (one integer histogram per digit),
//                                 then an ordered write of the candidates above the threshold key
//                                 and of the first of those equal to it
//   k_nms_pc                      one block per image: LDS bitonic sort by (class, logit desc,
//                                 anchor), decode of the candidates' boxes only, wave-parallel
//                                 greedy NMS per class out of LDS, final sort by score
//   k_softnms_pc                  edet_detect_per_class_soft, in place of k_nms_pc: the same sort
//                                 and decode, then per-class Gaussian Soft-NMS in fp64, one pass
//                                 over a class's live candidates per pick (decay, drop, arg-max,
//                                 in-place compaction), small classes a wave each and large ones
//                                 by the whole block (its section below)
//
// No floating-point atomics and no order-dependent integer atomics (the histograms are integer
// sums): the candidate list, and so every output, is a function of the inputs alone.
#pragma clang fp contract(off)
#include <float.h>
#include "blockops.hpp"
#include "boxes.hpp"

namespace edet {

constexpr int DET_CH = EDET_DETECT_CHUNK_ROWS;  // pyramid rows per scan block
constexpr int DET_THREADS = 256;                // scan block (4 waves)
constexpr uint64_t KEY_SENTINEL = ~0ull;        // sorts after every real key

// (desc_bits / desc_float, the order-preserving float key, and bitonic_sort: blockops.hpp)
// scan key: class (8) | logit, descending (32) | anchor index in the image (24)
__device__ __forceinline__ uint64_t make_key(int c, float v, int i) {
  if (v == 0.f) v = 0.f;  // -0 and +0 are one score
  return ((uint64_t)c << 56) | ((uint64_t)desc_bits(v) << 24) | (uint64_t)i;
}

// The scan block `bid` of a grid numbered (image, level, chunk): its image, its level, the
// first pyramid row of its chunk, the chunk's rows and the image-flat index of the chunk's
// first anchor.  nbi: blocks per image.
struct ScanBlock {
  int n, first;   // image; index of the image's first block
  int64_t row0;   // first pyramid row
  int nr;         // rows (<= DET_CH)
  int abase;      // flat anchor index of (row0, a = 0) within the image
};
__device__ __forceinline__ ScanBlock scan_block(const edet_pyramid& p, int A, int nbi, int bid) {
  ScanBlock b;
  b.n = bid / nbi;
  b.first = b.n * nbi;
  int c = bid - b.first, ab = 0, s = 0;
  for (; s < p.nseg - 1; ++s) {
    const int hw = p.H[s] * p.W[s], nc = cdiv(hw, DET_CH);
    if (c < nc) break;
    c -= nc;
    ab += hw * A;
  }
  const int hw = p.H[s] * p.W[s];
  b.row0 = (int64_t)p.row_off[s] + (int64_t)b.n * hw + (int64_t)c * DET_CH;
  b.nr = min(DET_CH, hw - c * DET_CH);
  b.abase = ab + c * DET_CH * A;
  return b;
}

// A block's chunk is the contiguous element span [e0, e1) of the logits buffer (its rows, up
// to the last row's last used column).  It is read as "virtual vectors" of 16 bytes on the
// buffer's 16-byte grid: vector v covers elements [ea + v * VE, ea + (v + 1) * VE) with ea the
// grid point at or below e0.  Interior vectors are one aligned 16-byte load; the first and
// the last may straddle the span's ends and are read element by element (the scalar prologue
// and epilogue).  Vector order is element order, so it is flat candidate order.
template <typename T>
struct Span {
  static constexpr int VE = 16 / (int)sizeof(T);
  const T* cls;
  int64_t e0, e1, ea, eb;  // eb: element offset of the chunk's first row (== e0)
  int nv, ldc, anc, NC, A, abase;
  float thr;

  __device__ __forceinline__ Span(const T* cls_, const ScanBlock& b, int ldc_, int A_, int NC_, float thr_)
      : cls(cls_), ldc(ldc_), anc(A_ * NC_), NC(NC_), A(A_), abase(b.abase), thr(thr_) {
    e0 = eb = b.row0 * ldc;
    e1 = (b.row0 + b.nr - 1) * ldc + anc;
    const int mis = (int)(((uintptr_t)(cls + e0) & 15) / sizeof(T));
    ea = e0 - mis;
    nv = (int)((e1 - ea + VE - 1) / VE);
  }
  __device__ __forceinline__ bool full(int v) const {
    const int64_t es = ea + (int64_t)v * VE;
    return v < nv && es >= e0 && es + VE <= e1;
  }
  // the 16 bytes of an interior vector (issued ahead of their use); zeros otherwise
  __device__ __forceinline__ uint4 fetch(int v) const {
    return full(v) ? gld16(cls + ea + (int64_t)v * VE) : make_uint4(0u, 0u, 0u, 0u);
  }
  // class and image-flat anchor of span element `rel` (relative to eb); false for a pad
  // column or the background class.  Only lanes that passed the compare get here.
  __device__ __forceinline__ bool locate(int rel, int& c, int& i) const {
    const int r = rel / ldc, col = rel - r * ldc;
    const int a = col / NC;
    c = col - a * NC;
    i = abase + r * A + a;
    return col < anc && c != 0;
  }
  // values of vector v and the mask of its candidates
  __device__ __forceinline__ uint32_t eval(int v, uint4 raw, float* o) const {
    const int64_t es = ea + (int64_t)v * VE;
    uint32_t m = 0;
    if (full(v)) {
      if constexpr (sizeof(T) == 2) {
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[2 * j] = __uint_as_float(w[j] << 16);
          o[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
      } else {
        o[0] = __uint_as_float(raw.x); o[1] = __uint_as_float(raw.y);
        o[2] = __uint_as_float(raw.z); o[3] = __uint_as_float(raw.w);
      }
#pragma unroll
      for (int j = 0; j < VE; ++j) m |= (uint32_t)(o[j] >= thr) << j;
    } else if (v < nv) {
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        const int64_t e = es + j;
        const bool in = e >= e0 && e < e1;
        o[j] = in ? to_f<T>(cls[in ? e : e0]) : 0.f;
        m |= (uint32_t)(in && o[j] >= thr) << j;
      }
    } else {
#pragma unroll
      for (int j = 0; j < VE; ++j) o[j] = 0.f;
    }
    if (m) {
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        int c, i;
        if (((m >> j) & 1u) && !locate((int)(es + j - eb), c, i)) m &= ~(1u << j);
      }
    }
    return m;
  }
};

constexpr int SEL_BINS = 2048;   // bins of one digit's histogram (11 bits; the last fp32 digit uses 1024)
constexpr int SEL_DIGITS = 3;    // histograms per image in scratch
constexpr int SEL_STATE = 8;     // ints of select state per image: (prefix, rank) after each digit

// Pass 1: counts[bid] = candidates in the block's chunk.  ZERO (the top-K path): an image's
// first block also clears the image's digit histograms.
template <typename T, bool ZERO = false>
__global__ __launch_bounds__(DET_THREADS) void k_cand_count(const T* cls, int ldc, edet_pyramid p, int A, int NC,
                                                            int nbi, float thr, int32_t* counts, int32_t* hist) {
  __shared__ int wsum[DET_THREADS / 64];
  const ScanBlock b = scan_block(p, A, nbi, blockIdx.x);
  if constexpr (ZERO) {
    if ((int)blockIdx.x == b.first)
      for (int q = threadIdx.x; q < SEL_DIGITS * SEL_BINS; q += DET_THREADS)
        hist[(size_t)b.n * SEL_DIGITS * SEL_BINS + q] = 0;
  }
  const Span<T> sp(cls, b, ldc, A, NC, thr);
  int cnt = 0;
  uint4 raw = sp.fetch(threadIdx.x);
  for (int v = threadIdx.x; v < sp.nv; v += DET_THREADS) {
    const uint4 nxt = sp.fetch(v + DET_THREADS);
    float o[Span<T>::VE];
    cnt += __popc(sp.eval(v, raw, o));
    raw = nxt;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// Pass 2: the block's offset within its image is the sum of the counts of the image's blocks
// before it (the block adds them itself); it then streams its chunk again and writes survivor
// k of the image to cand[n][k] while k < cap.  The image's last block writes total / overflow.
template <typename T>
__global__ __launch_bounds__(DET_THREADS) void k_cand_write(const T* cls, int ldc, edet_pyramid p, int A, int NC,
                                                            int nbi, float thr, const int32_t* counts, int cap,
                                                            uint64_t* cand, int32_t* total, int32_t* overflow) {
  constexpr int VE = Span<T>::VE, NW = DET_THREADS / 64;
  __shared__ int wsum[2][NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ScanBlock b = scan_block(p, A, nbi, blockIdx.x);
  int base = 0;
  for (int j = b.first + tid; j < (int)blockIdx.x; j += DET_THREADS) base += counts[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o, 64);
  if (lane == 0) wsum[0][wave] = base;
  __syncthreads();
  base = (wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3]);
  __syncthreads();
  const int mine = counts[blockIdx.x];
  if ((int)blockIdx.x == b.first + nbi - 1 && tid == 0) {
    total[b.n] = base + mine;
    overflow[b.n] = (base + mine > cap) ? 1 : 0;
  }
  if (mine == 0 || base >= cap) return;  // block-uniform

  const Span<T> sp(cls, b, ldc, A, NC, thr);
  uint64_t* out = cand + (size_t)b.n * cap;
  const uint64_t lt = (1ull << lane) - 1ull;
  int run = base;  // candidates of the image before this round, the same in every thread
  uint4 raw = sp.fetch(tid);
  for (int v0 = 0, r = 0; v0 < sp.nv && run < cap; v0 += DET_THREADS, r ^= 1) {
    const int v = v0 + tid;
    const uint4 nxt = sp.fetch(v + DET_THREADS);
    float o[VE];
    const uint32_t m = sp.eval(v, raw, o);
    raw = nxt;
    // lane offset: the candidates of the lower lanes' vectors (ballot + popcount per element
    // slot), only in waves that hold a candidate at all
    int loff = 0, wtot = 0;
    if (__ballot(m != 0)) {
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        const uint64_t bj = __ballot((m >> j) & 1u);
        loff += __popcll(bj & lt);
        wtot += __popcll(bj);
      }
    }
    if (lane == 0) wsum[r][wave] = wtot;
    __syncthreads();  // (one per round: the two wsum rows alternate)
    int pos = run + loff;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int t = wsum[r][w];
      pos += (w < wave) ? t : 0;
      run += t;
    }
    if (m) {
      const int rel0 = (int)(sp.ea + (int64_t)v * VE - sp.eb);
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        if ((m >> j) & 1u) {
          int c, i;
          sp.locate(rel0 + j, c, i);
          if (pos < cap) out[pos] = make_key(c, o[j], i);
          ++pos;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- exact top-K selection
// An image with total > cap candidates keeps the first cap in (logit descending, flat id
// ascending) order.  With k = sel_key(logit) that is: every candidate whose key is below the
// cap-th smallest key T, and the first need_eq = cap - #{k < T} candidates with k == T in flat
// order.  T is found digit by digit from the top (11 + 11 + 10 bits).  The pass of digit d
// histograms that digit over the candidates whose higher digits equal the prefix of T known
// so far; the next launch finds the bin in which the cumulative count reaches the remaining
// rank.  A bf16 logit's low 10 key bits follow from its sign (the key's top bit), so two digits
// order bf16 keys completely: the select then works on key >> 10.
template <typename T>
struct Sel {
  static constexpr int ND = sizeof(T) == 2 ? 2 : 3;  // digit passes
  static constexpr int KS = sizeof(T) == 2 ? 10 : 0;  // the select compares key >> KS
};
__device__ __forceinline__ int sel_shift(int d) { return d == 0 ? 21 : (d == 1 ? 10 : 0); }
__device__ __forceinline__ int sel_width(int d) { return d == 2 ? 10 : 11; }
__device__ __forceinline__ uint32_t sel_key(float v) {
  if (v == 0.f) v = 0.f;  // -0 and +0 are one score (make_key)
  return desc_bits(v);
}

// Resolve digit d of the image's threshold key: the bin of the digit's finished histogram gh
// in which the running count first reaches `rank` (1-based, among the candidates under
// `prefix`).  On return prefix has the digit appended and rank counts within that bin.  Every
// block computes this for itself; the image's first block records it in st for the next launch.
// lh (SEL_BINS ints) is staging space and is free again afterwards.
__device__ __forceinline__ void sel_resolve(const int32_t* gh, int d, int* lh, int* wsum, int* res, bool record,
                                            int32_t* st, uint32_t& prefix, int& rank) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = tid; q < SEL_BINS; q += DET_THREADS) lh[q] = gh[q];
  if (tid == 0) { res[0] = 0; res[1] = 1; }
  __syncthreads();
  constexpr int PER = SEL_BINS / DET_THREADS;  // consecutive bins per thread
  int s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) s += lh[tid * PER + j];
  int inc = s;  // inclusive scan over the block, in bin order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    inc += (lane >= o) ? t : 0;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int exc = inc - s;
#pragma unroll
  for (int w = 0; w < DET_THREADS / 64; ++w) exc += (w < wave) ? wsum[w] : 0;
  if (exc < rank && rank <= exc + s) {  // one thread: the histogram holds at least `rank`
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int c = lh[tid * PER + j];
      if (exc < rank && rank <= exc + c) { res[0] = tid * PER + j; res[1] = rank - exc; }
      exc += c;
    }
  }
  __syncthreads();
  prefix = (prefix << sel_width(d)) | (uint32_t)res[0];
  rank = res[1];
  if (record && tid == 0) { st[2 * d] = (int32_t)prefix; st[2 * d + 1] = rank; }
  __syncthreads();  // lh, wsum and res are reused
}

// Digit pass d of an overflowing image: hist[n][d][bin] += the block's candidates under the
// prefix (integer adds, order-free).  Blocks of an image within the cap leave at once.
template <typename T>
__global__ __launch_bounds__(DET_THREADS) void k_sel_hist(const T* cls, int ldc, edet_pyramid p, int A, int NC,
                                                          int nbi, float thr, int cap, int d, const int32_t* total,
                                                          int32_t* state, int32_t* hist) {
  __shared__ int lh[SEL_BINS];
  __shared__ int wsum[DET_THREADS / 64];
  __shared__ int res[2];
  const ScanBlock b = scan_block(p, A, nbi, blockIdx.x);
  if (total[b.n] <= cap) return;  // block-uniform
  int32_t* st = state + (size_t)b.n * SEL_STATE;
  int32_t* gh = hist + (size_t)b.n * SEL_DIGITS * SEL_BINS;
  uint32_t prefix = 0;
  int rank = cap;
  if (d > 0) {
    if (d > 1) { prefix = (uint32_t)st[2 * (d - 2)]; rank = st[2 * (d - 2) + 1]; }
    sel_resolve(gh + (d - 1) * SEL_BINS, d - 1, lh, wsum, res, (int)blockIdx.x == b.first, st, prefix, rank);
  }
  for (int q = threadIdx.x; q < SEL_BINS; q += DET_THREADS) lh[q] = 0;
  __syncthreads();
  const int sh = sel_shift(d), shp = d > 0 ? sel_shift(d - 1) : 0;
  const uint32_t mask = (1u << sel_width(d)) - 1u;
  const Span<T> sp(cls, b, ldc, A, NC, thr);
  uint4 raw = sp.fetch(threadIdx.x);
  for (int v = threadIdx.x; v < sp.nv; v += DET_THREADS) {
    const uint4 nxt = sp.fetch(v + DET_THREADS);
    float o[Span<T>::VE];
    const uint32_t m = sp.eval(v, raw, o);
    raw = nxt;
    if (m) {
#pragma unroll
      for (int j = 0; j < Span<T>::VE; ++j) {
        const uint32_t k = sel_key(o[j]);
        if (((m >> j) & 1u) && (d == 0 || (k >> shp) == prefix)) atomicAdd(&lh[(k >> sh) & mask], 1);
      }
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < SEL_BINS; q += DET_THREADS) {
    const int c = lh[q];
    if (c) atomicAdd(&gh[d * SEL_BINS + q], c);
  }
}

// After the last digit: the threshold key T (as key >> KS) and need_eq are known.  Per block,
// cgt[bid] / ceq[bid] = its candidates better than / equal to T.
template <typename T>
__global__ __launch_bounds__(DET_THREADS) void k_sel_count(const T* cls, int ldc, edet_pyramid p, int A, int NC,
                                                           int nbi, float thr, int cap, const int32_t* total,
                                                           int32_t* state, const int32_t* hist, int32_t* cgt,
                                                           int32_t* ceq) {
  constexpr int ND = Sel<T>::ND, KS = Sel<T>::KS;
  __shared__ int lh[SEL_BINS];
  __shared__ int wsum[2 * (DET_THREADS / 64)];
  __shared__ int res[2];
  const ScanBlock b = scan_block(p, A, nbi, blockIdx.x);
  if (total[b.n] <= cap) return;  // block-uniform
  int32_t* st = state + (size_t)b.n * SEL_STATE;
  uint32_t tk = (uint32_t)st[2 * (ND - 2)];
  int need = st[2 * (ND - 2) + 1];
  sel_resolve(hist + ((size_t)b.n * SEL_DIGITS + (ND - 1)) * SEL_BINS, ND - 1, lh, wsum, res,
              (int)blockIdx.x == b.first, st, tk, need);
  const Span<T> sp(cls, b, ldc, A, NC, thr);
  int ngt = 0, neq = 0;
  uint4 raw = sp.fetch(threadIdx.x);
  for (int v = threadIdx.x; v < sp.nv; v += DET_THREADS) {
    const uint4 nxt = sp.fetch(v + DET_THREADS);
    float o[Span<T>::VE];
    const uint32_t m = sp.eval(v, raw, o);
    raw = nxt;
    if (m) {
#pragma unroll
      for (int j = 0; j < Span<T>::VE; ++j) {
        const uint32_t k = sel_key(o[j]) >> KS;
        const bool c = (m >> j) & 1u;
        ngt += (c && k < tk) ? 1 : 0;
        neq += (c && k == tk) ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ngt += __shfl_xor(ngt, o, 64);
    neq += __shfl_xor(neq, o, 64);
  }
  if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = ngt; wsum[4 + (threadIdx.x >> 6)] = neq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    cgt[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    ceq[blockIdx.x] = (wsum[4] + wsum[5]) + (wsum[6] + wsum[7]);
  }
}

// The ordered write of an overflowing image, over the first-in-flat-order keys k_cand_write
// left there: candidate g of those better than T goes to cand[n][g], candidate e < need_eq of
// those equal to T to cand[n][cap - need_eq + e]; g and e count in flat order (the block sums
// its predecessors' counts itself, lanes by ballot + popcount, waves through two alternating
// LDS rows as in k_cand_write).
template <typename T>
__global__ __launch_bounds__(DET_THREADS) void k_sel_write(const T* cls, int ldc, edet_pyramid p, int A, int NC,
                                                           int nbi, float thr, int cap, const int32_t* total,
                                                           const int32_t* state, const int32_t* cgt,
                                                           const int32_t* ceq, uint64_t* cand) {
  constexpr int VE = Span<T>::VE, NW = DET_THREADS / 64, ND = Sel<T>::ND, KS = Sel<T>::KS;
  __shared__ int wsum[2][2 * NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ScanBlock b = scan_block(p, A, nbi, blockIdx.x);
  if (total[b.n] <= cap) return;  // block-uniform
  const uint32_t tk = (uint32_t)state[(size_t)b.n * SEL_STATE + 2 * (ND - 1)];
  const int need = state[(size_t)b.n * SEL_STATE + 2 * (ND - 1) + 1];
  const int first_eq = cap - need;  // == the image's candidates better than T
  int bg = 0, be = 0;
  for (int j = b.first + tid; j < (int)blockIdx.x; j += DET_THREADS) { bg += cgt[j]; be += ceq[j]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bg += __shfl_xor(bg, o, 64);
    be += __shfl_xor(be, o, 64);
  }
  if (lane == 0) { wsum[0][wave] = bg; wsum[0][NW + wave] = be; }
  __syncthreads();
  bg = (wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3]);
  be = (wsum[0][4] + wsum[0][5]) + (wsum[0][6] + wsum[0][7]);
  __syncthreads();
  if (cgt[blockIdx.x] == 0 && (ceq[blockIdx.x] == 0 || be >= need)) return;  // block-uniform

  const Span<T> sp(cls, b, ldc, A, NC, thr);
  uint64_t* out = cand + (size_t)b.n * cap;
  const uint64_t lt = (1ull << lane) - 1ull;
  int rg = bg, re = be;  // candidates of the two kinds before this round, the same in every thread
  uint4 raw = sp.fetch(tid);
  for (int v0 = 0, r = 0; v0 < sp.nv; v0 += DET_THREADS, r ^= 1) {
    const int v = v0 + tid;
    const uint4 nxt = sp.fetch(v + DET_THREADS);
    float o[VE];
    const uint32_t m = sp.eval(v, raw, o);
    raw = nxt;
    uint32_t mg = 0, me = 0;
    if (m) {
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        const uint32_t k = sel_key(o[j]) >> KS;
        mg |= (uint32_t)(((m >> j) & 1u) && k < tk) << j;
        me |= (uint32_t)(((m >> j) & 1u) && k == tk) << j;
      }
    }
    int og = 0, oe = 0, wg = 0, we = 0;
    if (__ballot((mg | me) != 0)) {
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        const uint64_t gj = __ballot((mg >> j) & 1u), ej = __ballot((me >> j) & 1u);
        og += __popcll(gj & lt);
        wg += __popcll(gj);
        oe += __popcll(ej & lt);
        we += __popcll(ej);
      }
    }
    if (lane == 0) { wsum[r][wave] = wg; wsum[r][NW + wave] = we; }
    __syncthreads();  // (one per round: the two wsum rows alternate)
    int pg = rg + og, pe = re + oe;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int tg = wsum[r][w], te = wsum[r][NW + w];
      pg += (w < wave) ? tg : 0;
      pe += (w < wave) ? te : 0;
      rg += tg;
      re += te;
    }
    if (mg | me) {
      const int rel0 = (int)(sp.ea + (int64_t)v * VE - sp.eb);
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        const bool g = (mg >> j) & 1u, e = (me >> j) & 1u;
        if (g || e) {
          int c, i;
          sp.locate(rel0 + j, c, i);
          const int pos = g ? pg : ((pe < need) ? first_eq + pe : -1);
          if ((unsigned)pos < (unsigned)cap) out[pos] = make_key(c, o[j], i);  // (never past the image's slots)
          pg += g ? 1 : 0;
          pe += e ? 1 : 0;
        }
      }
    }
  }
}

__device__ __forceinline__ float lane_bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// The start of both per-image kernels, by the whole block: the image's m candidate keys into
// LDS (padded to the power of two P, which is returned), sorted by (class, logit descending,
// anchor), the boxes of the sorted candidates and the class segments [cstart, cend).
template <typename T>
__device__ __forceinline__ int sort_candidates(const float* anchors, const edet_pyramid& p, int A, const T* box,
                                               int ldb, const uint64_t* cand, int n, int m, uint64_t* keys,
                                               float4* boxes, int* cstart, int* cend) {
  const int tid = threadIdx.x;
  int P = 1;
  while (P < m) P <<= 1;
  for (int q = tid; q < P; q += blockDim.x) keys[q] = (q < m) ? cand[q] : KEY_SENTINEL;
  if (tid < 256) { cstart[tid] = 0; cend[tid] = 0; }
  __syncthreads();
  bitonic_sort(keys, P);  // class ascending, logit descending, anchor ascending

  // boxes of the sorted candidates, and the class segments [cstart, cend)
  for (int q = tid; q < m; q += blockDim.x) {
    const uint64_t k = keys[q];
    const int i = (int)(k & 0xffffffu), c = (int)(k >> 56);
    int64_t row;
    int a;
    cand_locate(p, A, n, i, row, a);
    float bx[4];
    decode_one<T>(anchors + (size_t)i * 4, box + row * ldb + a * 4, bx);
    boxes[q] = make_float4(bx[0], bx[1], bx[2], bx[3]);
    if (q == 0 || (int)(keys[q - 1] >> 56) != c) cstart[c] = q;
    if (q == m - 1 || (int)(keys[q + 1] >> 56) != c) cend[c] = q + 1;
  }
  __syncthreads();
  return P;
}

// The end of both: keys holds the output keys (score or logit descending (32) | anchor (24) |
// class (8)) sorted ascending, dropped candidates as the sentinel behind them.  Thread k writes
// output k, its box decoded again from its regression (the LDS copy was reused).  SOFT: the
// key's float is the score already; else it is the logit.
template <typename T, bool SOFT>
__device__ __forceinline__ void write_detections(const float* anchors, const edet_pyramid& p, int A, const T* box,
                                                 int ldb, const uint64_t* keys, int n, int m, int max_out,
                                                 float* out_boxes, int32_t* out_cls, float* out_scores,
                                                 int32_t* out_count) {
  const int lim = min(max_out, m);
  for (int k = threadIdx.x; k < lim; k += blockDim.x) {
    const uint64_t key = keys[k];
    if (key == KEY_SENTINEL) continue;
    if (k + 1 == lim || keys[k + 1] == KEY_SENTINEL) out_count[n] = k + 1;  // (m > 0: at least one is kept)
    const int i = (int)((key >> 8) & 0xffffffu);
    int64_t row;
    int a;
    cand_locate(p, A, n, i, row, a);
    decode_one<T>(anchors + (size_t)i * 4, box + row * ldb + a * 4, out_boxes + ((size_t)n * max_out + k) * 4);
    out_cls[(size_t)n * max_out + k] = (int)(key & 0xffu);
    const float v = desc_float((uint32_t)(key >> 32));
    out_scores[(size_t)n * max_out + k] = SOFT ? v : 1.0f / (1.0f + expf(-v));
  }
}

// One 1024-thread block per image.  Dynamic LDS: keys[pcap] (8 B) then boxes[cap] (16 B), pcap
// the power of two at or above cap.
template <typename T>
__global__ __launch_bounds__(1024) void k_nms_pc(const float* anchors, edet_pyramid p, int A, const T* box, int ldb,
                                                 int NC, const uint64_t* cand, const int32_t* total, int cap,
                                                 int pcap, int max_out, float iou_thr, int diou, float* out_boxes,
                                                 int32_t* out_cls, float* out_scores, int32_t* out_count) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int cstart[256], cend[256];
  __shared__ int next_cls;
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem);
  float4* boxes = reinterpret_cast<float4*>(smem + (size_t)pcap * 8);
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int m = min(total[n], cap);
  if (m == 0) {  // block-uniform
    if (tid == 0) out_count[n] = 0;
    return;
  }
  if (tid == 0) next_cls = 1;
  const int P = sort_candidates<T>(anchors, p, A, box, ldb, cand + (size_t)n * cap, n, m, keys, boxes, cstart, cend);

  // Greedy NMS, a wave per class.  The class's kept boxes are compacted to the front of its
  // own segment of `boxes` (kept box k at s0 + k, never past the candidate being resolved, and
  // every lane of the tile holds its own box in registers by then).  A candidate's key is
  // rewritten as its output key (logit desc, anchor, class), or the sentinel when dropped.
  for (;;) {
    int c = 0;
    if (lane == 0) c = atomicAdd(&next_cls, 1);  // which wave takes a class does not reach the result
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= NC) break;
    const int s0 = cstart[c], s1 = cend[c];
    int nk = 0;
    for (int t0 = s0; t0 < s1; t0 += 64) {
      const int q = t0 + lane;
      const bool valid = q < s1;
      const uint64_t key = valid ? keys[q] : KEY_SENTINEL;
      const float4 bq = boxes[valid ? q : s0];
      const float b[4] = {bq.x, bq.y, bq.z, bq.w};
      bool alive = valid && nk < max_out, kept = false;
      for (int k = 0; k < nk && alive; ++k) {  // against the boxes kept from earlier tiles
        const float4 kq = boxes[s0 + k];
        const float kb[4] = {kq.x, kq.y, kq.z, kq.w};
        if ((diou ? diou_tf(kb, b) : iou_tf(kb, b)) >= iou_thr) alive = false;
      }
      uint64_t live = __ballot(alive);
      while (live && nk < max_out) {  // the lowest live lane is kept, the lanes above test against it
        const int l = __builtin_ctzll(live);
        const float kb[4] = {lane_bcast(b[0], l), lane_bcast(b[1], l), lane_bcast(b[2], l), lane_bcast(b[3], l)};
        if (lane == l) {
          kept = true;
          alive = false;
          boxes[s0 + nk] = make_float4(kb[0], kb[1], kb[2], kb[3]);
        }
        ++nk;
        if (alive && (diou ? diou_tf(kb, b) : iou_tf(kb, b)) >= iou_thr) alive = false;
        live = __ballot(alive);
      }
      if (valid)
        keys[q] = kept ? (((key >> 24) & 0xffffffffull) << 32) | ((key & 0xffffffull) << 8) | (key >> 56)
                       : KEY_SENTINEL;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next tile reads this tile's kept boxes
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  bitonic_sort(keys, P);  // logit descending, anchor ascending, class ascending; dropped last

  write_detections<T, false>(anchors, p, A, box, ldb, keys, n, m, max_out, out_boxes, out_cls, out_scores, out_count);
}

// ---------------------------------------------------------------- Gaussian Soft-NMS
// Per class: pick the live candidate with the largest score s (fp64; on equal s the lower
// anchor), emit it, multiply every other live s_j by exp(-iou^2 / sigma), drop j once s_j <
// min_score; until the class is empty or has max_out picks.  The winner of a round depends on
// every earlier decay, so the class's live list is swept once per pick.  A sweep ("pass") does
// three things to each live candidate: the decay by the current pick, the min_score test, and
// its share of the arg-max under (s descending, anchor ascending), which is the next pick.
// The live list sits at the front of the class's own segment of keys / boxes / score and is
// compacted in place by every pass (ballot + popcount prefix, candidates keep their order), so
// passes shrink as candidates retire or drop.  Emission k of a class goes to the segment's slot
// s1 - 1 - k: live + emitted + dropped is the segment's size, so that slot is behind the live
// list once the pass that retired the pick has run.
//
// Work split: a class whose segment has at most SOFT_WAVE_MAX candidates is swept by one wave
// (classes claimed from a counter, as in k_nms_pc); a larger one by the whole block afterwards,
// 1024 candidates per round.  A block pass pays one barrier per round, one for the cross-wave
// arg-max and the 16-entry LDS reduction, about the time of three to four 64-candidate tiles of
// a wave pass; a wave working alone breaks even there, hence 256 = four tiles.  (A segment is
// never re-routed: a block class whose live list shrinks under 256 stays with the block.)
//
// Arithmetic: overlap (iou_tf64, the op order of iou_tf), decay and scores are fp64 without
// contraction; IEEE add / mul / div are the same bits on any conforming machine, so against an
// fp64 host restatement in the same order only exp differs: <= 1 ulp here (the HIP math API's
// documented bound for the double exp) plus <= 1 ulp there, and the product's own rounding moves
// by <= 1 ulp with it.  That is <= 3 ulp = 6.7e-16 relative per decay, <= 7e-14 after 100
// decays (the initial sigmoid adds 2 ulp once).  The score is rounded to fp32 once, on emission.
constexpr int SOFT_WAVE_MAX = 256;

// arg-max operand: the score's bits (s >= 0, so their unsigned order is the order of s) and
// (2^24 - 1 - anchor) << 12 | position (24 + 12 bits), so the larger tag is the lower anchor.
// A real tag is never 0 (anchor < 2^24 - 1), so {0, 0} loses to every candidate.
struct SoftBest {
  uint64_t sb, tag;
};
__device__ __forceinline__ SoftBest soft_better(SoftBest a, SoftBest b) {
  return (b.sb > a.sb || (b.sb == a.sb && b.tag > a.tag)) ? b : a;
}
__device__ __forceinline__ SoftBest soft_xor(SoftBest v, int o) {
  SoftBest r;
  r.sb = (uint64_t)__shfl_xor((unsigned long long)v.sb, o, 64);
  r.tag = (uint64_t)__shfl_xor((unsigned long long)v.tag, o, 64);
  return r;
}

// One pass over the live list [s0, s0 + L) of a class, by one wave (BLOCK = false) or by the
// whole block (every thread calls it, with block-uniform arguments).  DECAY: the candidate at
// ppos is retired and the others decay by the pick's box pb; without it (the first pass) nothing
// moves.  Returns the new live count; best is the arg-max over the new list, its position the
// compacted one.  Both are uniform over the wave / block.  wsum: [2][16] ints, wbest: [16]
// entries, block mode only; the caller alternates wbest between passes.
template <bool BLOCK, bool DECAY>
__device__ __forceinline__ int soft_pass(uint64_t* keys, float4* boxes, double* score, int s0, int L, int ppos,
                                         const double* pb, double sigma, double min_score, int* wsum,
                                         SoftBest* wbest, SoftBest& best) {
  constexpr int STEP = BLOCK ? 1024 : 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, me = BLOCK ? (int)threadIdx.x : lane;
  const uint64_t lt = (1ull << lane) - 1ull;
  SoftBest mine = {0ull, 0u};
  int run = 0;  // live candidates written so far, the same in every thread
  for (int t0 = 0, r = 0; t0 < L; t0 += STEP, r ^= 1) {
    const bool valid = t0 + me < L;
    const int q = s0 + (valid ? t0 + me : 0);
    const uint64_t key = keys[q];
    const float4 bq = boxes[q];
    double s = score[q];
    if constexpr (!BLOCK) {  // the tile is in registers before any lane writes into it
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    bool keep = valid;
    if constexpr (DECAY) {
      keep = valid && q != ppos;
      if (keep) {
        const double b[4] = {bq.x, bq.y, bq.z, bq.w};
        const double ov = iou_tf64(pb, b);
        s = s * exp(-(ov * ov) / sigma);
        keep = !(s < min_score);
      }
    }
    const uint64_t bal = __ballot(keep);
    int np = s0 + run + __popcll(bal & lt);
    if constexpr (BLOCK) {
      if (lane == 0) wsum[r * 16 + wave] = __popcll(bal);
      __syncthreads();  // (one per round: the two wsum rows alternate; every read of the round is done)
#pragma unroll
      for (int w = 0; w < 16; ++w) {
        const int t = wsum[r * 16 + w];
        np += (w < wave) ? t : 0;
        run += t;
      }
    } else {
      run += __popcll(bal);
    }
    if (keep) {  // np <= q: never ahead of what this round or tile has read
      if constexpr (DECAY) {
        keys[np] = key;
        boxes[np] = bq;
        score[np] = s;
      }
      const SoftBest c = {(uint64_t)__double_as_longlong(s),
                          ((0xffffffull - (key & 0xffffffull)) << 12) | (uint64_t)np};
      mine = soft_better(mine, c);
    }
    if constexpr (!BLOCK) {  // the next tile, and the caller, read this tile's writes
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine = soft_better(mine, soft_xor(mine, o));
  if constexpr (BLOCK) {
    if (lane == 0) wbest[wave] = mine;
    __syncthreads();
    mine = wbest[lane & 15];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mine = soft_better(mine, soft_xor(mine, o));
  }
  best = mine;
  return run;
}

// Soft-NMS of class c, segment [s0, s1), by one wave or by the whole block.  On return the
// segment's keys are the class's output keys (fp32 score descending | anchor | class) at its
// end and the sentinel before them.
template <bool BLOCK>
__device__ __forceinline__ void soft_class(uint64_t* keys, float4* boxes, double* score, int c, int s0, int s1,
                                           int max_out, double sigma, double min_score, int* wsum,
                                           SoftBest* wbest) {
  const int me = BLOCK ? (int)threadIdx.x : (int)(threadIdx.x & 63), step = BLOCK ? 1024 : 64;
  const double none[4] = {0.0, 0.0, 0.0, 0.0};
  SoftBest best;
  int L = soft_pass<BLOCK, false>(keys, boxes, score, s0, s1 - s0, -1, none, sigma, min_score, wsum, wbest, best);
  int k = 0;
  while (L > 0 && k < max_out) {
    const int pos = (int)(best.tag & 0xfffu);
    const uint64_t anchor = 0xffffffull - (best.tag >> 12);
    const float sc = (float)__longlong_as_double((long long)best.sb);  // the one rounding to fp32
    const uint64_t okey = ((uint64_t)desc_bits(sc) << 32) | (anchor << 8) | (uint64_t)c;
    if (k + 1 < max_out) {  // (the class's last pick decays nobody)
      const float4 pq = boxes[pos];
      const double pb[4] = {pq.x, pq.y, pq.z, pq.w};
      L = soft_pass<BLOCK, true>(keys, boxes, score, s0, L, pos, pb, sigma, min_score, wsum,
                                 wbest + ((k & 1) ? 0 : 16), best);
    } else {
      L = 0;
    }
    if (me == 0) keys[s1 - 1 - k] = okey;  // behind the live list (header)
    ++k;
  }
  for (int q = s0 + me; q < s1 - k; q += step) keys[q] = KEY_SENTINEL;
}

// One 1024-thread block per image.  Dynamic LDS: keys[pcap] (8 B), boxes[cap] (16 B), score[cap]
// (8 B): 128 KiB at cap = 4096.
template <typename T>
__global__ __launch_bounds__(1024) void k_softnms_pc(const float* anchors, edet_pyramid p, int A, const T* box,
                                                     int ldb, int NC, const uint64_t* cand, const int32_t* total,
                                                     int cap, int pcap, int max_out, double sigma, double min_score,
                                                     float* out_boxes, int32_t* out_cls, float* out_scores,
                                                     int32_t* out_count) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int cstart[256], cend[256];
  __shared__ int next_cls;
  __shared__ int wsum[2 * 16];
  __shared__ SoftBest wbest[2 * 16];
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem);
  float4* boxes = reinterpret_cast<float4*>(smem + (size_t)pcap * 8);
  double* score = reinterpret_cast<double*>(smem + (size_t)pcap * 8 + (size_t)cap * 16);
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int m = min(total[n], cap);
  if (m == 0) {  // block-uniform
    if (tid == 0) out_count[n] = 0;
    return;
  }
  if (tid == 0) next_cls = 1;
  const int P = sort_candidates<T>(anchors, p, A, box, ldb, cand + (size_t)n * cap, n, m, keys, boxes, cstart, cend);
  for (int q = tid; q < m; q += blockDim.x)
    score[q] = 1.0 / (1.0 + exp(-(double)desc_float((uint32_t)(keys[q] >> 24))));
  __syncthreads();

  for (;;) {  // small classes, a wave each
    int c = 0;
    if (lane == 0) c = atomicAdd(&next_cls, 1);  // which wave takes a class does not reach the result
    c = __builtin_amdgcn_readfirstlane(c);
    if (c >= NC) break;
    const int s0 = cstart[c], s1 = cend[c];
    if (s1 > s0 && s1 - s0 <= SOFT_WAVE_MAX)
      soft_class<false>(keys, boxes, score, c, s0, s1, max_out, sigma, min_score, wsum, wbest);
  }
  __syncthreads();
  for (int c = 1; c < NC; ++c) {  // large classes, the whole block each
    const int s0 = cstart[c], s1 = cend[c];
    if (s1 - s0 > SOFT_WAVE_MAX) soft_class<true>(keys, boxes, score, c, s0, s1, max_out, sigma, min_score, wsum, wbest);
  }
  __syncthreads();
  bitonic_sort(keys, P);  // score descending, anchor ascending, class ascending; the rest last

  write_detections<T, true>(anchors, p, A, box, ldb, keys, n, m, max_out, out_boxes, out_cls, out_scores, out_count);
}

}  // namespace edet

using namespace edet;

// Gaussian Soft-NMS in place of the hard kernel (validated by edet_detect_per_class_soft)
struct SoftNms {
  double sigma, min_score;
};

// every entry point; select and soft are validated by the caller.  soft == nullptr: hard NMS.
static int detect_per_class_run(int dtype, const float* anchors, const void* box, int ldb, const void* cls, int ldc,
                                const edet_pyramid* p, int A, int NC, int max_candidates, int max_out, float iou_thr,
                                float logit_thr, int metric, int select, const SoftNms* soft, void* scratch,
                                float* out_boxes, int32_t* out_cls, float* out_scores, int32_t* out_count,
                                int32_t* out_total, int32_t* out_overflow, edet_stream_t stream) {
  EDET_REQUIRE(anchors && box && cls && p && scratch && out_boxes && out_cls && out_scores && out_count &&
                   out_total && out_overflow,
               "detect_per_class: null argument");
  EDET_REQUIRE(dtype == EDET_F32 || dtype == EDET_BF16, "detect_per_class: unsupported dtype %d", dtype);
  EDET_REQUIRE(NC >= 2 && NC <= 256, "detect_per_class: NC %d outside 2..256 (class 0 is background, 8 key bits)", NC);
  EDET_REQUIRE(A > 0 && p->nseg >= 1 && p->nseg <= EDET_MAX_SEG, "detect_per_class: bad pyramid or A");
  EDET_REQUIRE(max_candidates >= 1 && max_candidates <= EDET_DETECT_MAX_CANDIDATES,
               "detect_per_class: max_candidates %d outside 1..%d", max_candidates, EDET_DETECT_MAX_CANDIDATES);
  EDET_REQUIRE(max_out >= 1 && max_out <= max_candidates, "detect_per_class: max_out %d outside 1..max_candidates",
               max_out);
  EDET_REQUIRE(ldc >= A * NC, "detect_per_class: ldc %d < A*NC", ldc);
  EDET_REQUIRE(ldb >= 4 * A, "detect_per_class: ldb %d < 4*A", ldb);
  EDET_REQUIRE(metric == EDET_OVERLAP_IOU || metric == EDET_OVERLAP_DIOU, "detect_per_class: unknown metric %d",
               metric);
  EDET_REQUIRE(logit_thr == logit_thr, "detect_per_class: the logit threshold is NaN");
  EDET_REQUIRE(((uintptr_t)scratch & 7) == 0, "detect_per_class: scratch not 8-byte aligned");
  int64_t N = 0;
  int nbi = 0;
  for (int s = 0; s < p->nseg; ++s) {
    N += (int64_t)p->H[s] * p->W[s] * A;
    nbi += cdiv(p->H[s] * p->W[s], DET_CH);
  }
  EDET_REQUIRE(N < (1 << 24), "detect_per_class: %lld anchors per image, the key holds 24 bits", (long long)N);
  EDET_REQUIRE((int64_t)DET_CH * ldc < (1 << 30) && (int64_t)p->batch * nbi < (1 << 30),
               "detect_per_class: problem too large");
  if (p->batch == 0 || N == 0) return EDET_OK;
  uint64_t* cand = (uint64_t*)scratch;
  int32_t* counts = (int32_t*)(cand + (size_t)p->batch * max_candidates);
  // EDET_SELECT_TOPK: per-block better / equal counts, per-image select state and histograms
  const size_t nblk = (size_t)p->batch * nbi;
  int32_t* cgt = counts + nblk;
  int32_t* ceq = cgt + nblk;
  int32_t* state = ceq + nblk;
  int32_t* hist = state + (size_t)p->batch * SEL_STATE;
  const int cap = max_candidates;
  int pcap = 2;  // (at least 16 bytes of keys: the boxes behind them stay 16-byte aligned)
  while (pcap < max_candidates) pcap <<= 1;
  // keys and boxes; Soft-NMS adds an fp64 score per candidate
  const size_t lds = (size_t)pcap * 8 + (size_t)max_candidates * (soft ? 24 : 16);
  EDET_REQUIRE(lds <= 156 * 1024, "detect_per_class: %zu bytes of LDS for %d candidates, a block has 160 KiB",
               lds, max_candidates);  // (the kernels' static LDS is under 4 KiB)
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(p->batch * nbi));
  EDET_DTYPE_DISPATCH(dtype, T, {
    if (lds > 48 * 1024) {
      const void* fn = soft ? reinterpret_cast<const void*>(&k_softnms_pc<T>)
                            : reinterpret_cast<const void*>(&k_nms_pc<T>);
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) {
        set_error("detect_per_class: %zu bytes of LDS: %s", lds, hipGetErrorString(e));
        return EDET_EHIP;
      }
    }
    const T* lg = (const T*)cls;
    if (select == EDET_SELECT_TOPK)
      EDET_LAUNCH((k_cand_count<T, true>), grid, dim3(DET_THREADS), 0, st, lg, ldc, *p, A, NC, nbi, logit_thr, counts,
                  hist);
    else
      EDET_LAUNCH(k_cand_count<T>, grid, dim3(DET_THREADS), 0, st, lg, ldc, *p, A, NC, nbi, logit_thr, counts,
                  (int32_t*)nullptr);
    EDET_LAUNCH(k_cand_write<T>, grid, dim3(DET_THREADS), 0, st, lg, ldc, *p, A, NC, nbi, logit_thr, counts,
                max_candidates, cand, out_total, out_overflow);
    if (select == EDET_SELECT_TOPK) {  // (blocks of an image with total <= cap return at once)
      for (int d = 0; d < Sel<T>::ND; ++d)
        EDET_LAUNCH(k_sel_hist<T>, grid, dim3(DET_THREADS), 0, st, lg, ldc, *p, A, NC, nbi, logit_thr, cap, d,
                    out_total, state, hist);
      EDET_LAUNCH(k_sel_count<T>, grid, dim3(DET_THREADS), 0, st, lg, ldc, *p, A, NC, nbi, logit_thr, cap, out_total,
                  state, hist, cgt, ceq);
      EDET_LAUNCH(k_sel_write<T>, grid, dim3(DET_THREADS), 0, st, lg, ldc, *p, A, NC, nbi, logit_thr, cap, out_total,
                  state, cgt, ceq, cand);
    }
    if (soft)
      EDET_LAUNCH(k_softnms_pc<T>, dim3(p->batch), dim3(1024), lds, st, anchors, *p, A, (const T*)box, ldb, NC, cand,
                  out_total, max_candidates, pcap, max_out, soft->sigma, soft->min_score, out_boxes, out_cls,
                  out_scores, out_count);
    else
      EDET_LAUNCH(k_nms_pc<T>, dim3(p->batch), dim3(1024), lds, st, anchors, *p, A, (const T*)box, ldb, NC, cand,
                  out_total, max_candidates, pcap, max_out, iou_thr, metric == EDET_OVERLAP_DIOU ? 1 : 0, out_boxes,
                  out_cls, out_scores, out_count);
    return check_launch("edet detect_per_class");
  });
}

extern "C" {

int edet_detect_per_class(int dtype, const float* anchors, const void* box, int ldb, const void* cls, int ldc,
                          const edet_pyramid* p, int A, int NC, int max_candidates, int max_out, float iou_thr,
                          float logit_thr, int metric, void* scratch, float* out_boxes, int32_t* out_cls,
                          float* out_scores, int32_t* out_count, int32_t* out_total, int32_t* out_overflow,
                          edet_stream_t stream) {
  return detect_per_class_run(dtype, anchors, box, ldb, cls, ldc, p, A, NC, max_candidates, max_out, iou_thr,
                              logit_thr, metric, EDET_SELECT_FIRST, nullptr, scratch, out_boxes, out_cls, out_scores, out_count,
                              out_total, out_overflow, stream);
}

int edet_detect_per_class_select(int dtype, const float* anchors, const void* box, int ldb, const void* cls, int ldc,
                                 const edet_pyramid* p, int A, int NC, int max_candidates, int max_out, float iou_thr,
                                 float logit_thr, int metric, int select, void* scratch, float* out_boxes,
                                 int32_t* out_cls, float* out_scores, int32_t* out_count, int32_t* out_total,
                                 int32_t* out_overflow, edet_stream_t stream) {
  EDET_REQUIRE(select == EDET_SELECT_FIRST || select == EDET_SELECT_TOPK,
               "detect_per_class: select %d is neither EDET_SELECT_FIRST nor EDET_SELECT_TOPK", select);
  return detect_per_class_run(dtype, anchors, box, ldb, cls, ldc, p, A, NC, max_candidates, max_out, iou_thr,
                              logit_thr, metric, select, nullptr, scratch, out_boxes, out_cls, out_scores, out_count,
                              out_total, out_overflow, stream);
}

int edet_detect_per_class_soft(int dtype, const float* anchors, const void* box, int ldb, const void* cls, int ldc,
                               const edet_pyramid* p, int A, int NC, int max_candidates, int max_out, float logit_thr,
                               int metric, int select, double sigma, double min_score, void* scratch,
                               float* out_boxes, int32_t* out_cls, float* out_scores, int32_t* out_count,
                               int32_t* out_total, int32_t* out_overflow, edet_stream_t stream) {
  EDET_REQUIRE(select == EDET_SELECT_FIRST || select == EDET_SELECT_TOPK,
               "detect_per_class_soft: select %d is neither EDET_SELECT_FIRST nor EDET_SELECT_TOPK", select);
  EDET_REQUIRE(metric == EDET_OVERLAP_IOU, "detect_per_class_soft: metric %d, Soft-NMS decays by the IoU only", metric);
  EDET_REQUIRE(sigma > 0.0 && sigma <= DBL_MAX, "detect_per_class_soft: sigma %g is not positive and finite", sigma);
  EDET_REQUIRE(min_score >= 0.0 && min_score < 1.0, "detect_per_class_soft: min_score %g outside [0, 1)", min_score);
  const SoftNms soft = {sigma, min_score};
  return detect_per_class_run(dtype, anchors, box, ldb, cls, ldc, p, A, NC, max_candidates, max_out, 0.f, logit_thr,
                              metric, select, &soft, scratch, out_boxes, out_cls, out_scores, out_count, out_total,
                              out_overflow, stream);
}

}  // extern "C"
