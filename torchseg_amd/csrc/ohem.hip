// OHEM 2-D cross entropy for gfx950.
//
// Restates ProbOhemCrossEntropy2d.forward (furnace/seg_opr/loss_opr.py:68-98):
//   valid = t != ignore ; prob = softmax(pred, 1) ; mask_prob = prob[t] (1 where
//   invalid) ; thr = max(thresh, k-th smallest mask_prob) with k = min(P,
//   min_kept) ; kept = mask_prob <= thr ; loss = CE(pred, t | valid & kept).
// The reference materialises the softmax, transposes it, runs a full
// torch.sort over P = B*H*W floats and a second log-softmax inside CE
// (>= 6 passes over the logits + an O(P log P) sort).  Here:
//   pass A  one read of the logits: online softmax per pixel -> nll = lse - x_t
//           and lse (8 B/pixel), block partial sums for the `thr == thresh`
//           outcome, and a coarse histogram of the IEEE bit patterns of
//           p_t = exp(-nll) above thresh (p in [0,1] => bit patterns are
//           monotone, so a radix select returns exactly sort(p)[k-1]);
//   decide  (1 block) picks the branch; when the k-th value lies above thresh,
//           1-2 refinement passes over nll (4 B/pixel) pin it bit-exactly and
//           pass C re-sums nll over p <= thr;
//   bwd     one read of logits + one write of dlogits, skipping reads for
//           pixels that were not kept.
// Everything stays on the device (no host sync); all cross-block reductions are
// integer atomics or fixed-order partials, so results are deterministic.
//
// HBM-bound: algorithmic bytes per pixel = C*s (fwd) + 2*C*s (bwd) + ~33 B side
// arrays (labels i64 x2, nll w+r x2, lse w+r).
#include "tsg_dispatch.h"
#include "tsg_resample.h"
#include <math.h>
#include <string.h>

namespace tsg {

constexpr int kT = 256;

struct SelState {
  int32_t branch;       // 0: thr = thresh; 1: thr = k-th value (> thresh); 2: no OHEM
  int32_t pad0;
  int64_t num_valid;
  int64_t n_kept;
  int64_t krem;         // remaining 1-based rank inside the current prefix
  int64_t lo_d;         // lower bound of the current prefix in d-space
  uint32_t thr_bits;    // final threshold (float bits)
  int32_t n_bad;        // labels outside [0, C) other than ignore_label (the reference device-asserts on them)
  double sum;           // sum of w*nll over kept
  double wsum;          // sum of w over kept (denominator when weighted)
};

struct BlkPart {
  float sum_le, sum_valid, wsum_le, wsum_valid;
  int32_t cnt_le_all, cnt_le_valid, cnt_valid, cnt_bad;  // cnt_bad: labels that are neither ignore_label nor in [0, C)
};

// ---- workspace carving ------------------------------------------------------
struct OhemWs {
  SelState* st;
  uint32_t* hist[3];
  BlkPart* part;      // [grid]
  float* csum;        // [grid] pass C
  float* cwsum;       // [grid]
  int32_t* ccnt;      // [grid]
  size_t zero_bytes;  // leading bytes that must be zeroed per call (state + hists)
  size_t total;
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static OhemWs carve(void* base, const tsg_ohem_plan& pl) {
  OhemWs w;
  char* p = (char*)base;
  size_t off = 0;
  w.st = (SelState*)(p + off); off += align_up(sizeof(SelState), 256);
  for (int l = 0; l < 3; ++l) {
    w.hist[l] = (uint32_t*)(p + off);
    off += align_up((size_t)(l < pl.levels ? pl.bins[l] : 0) * sizeof(uint32_t), 256);
  }
  w.zero_bytes = off;
  w.part = (BlkPart*)(p + off); off += align_up((size_t)pl.grid * sizeof(BlkPart), 256);
  w.csum = (float*)(p + off); off += align_up((size_t)pl.grid * sizeof(float), 256);
  w.cwsum = (float*)(p + off); off += align_up((size_t)pl.grid * sizeof(float), 256);
  w.ccnt = (int32_t*)(p + off); off += align_up((size_t)pl.grid * sizeof(int32_t), 256);
  w.total = off;
  return w;
}

// d-space: d = bits(p) - tb - 1 for p > thresh (tb = bits(thresh), or -1 when
// thresh < 0 so that every p >= 0 maps to d >= 0).
static void level_plan(int64_t range, int* levels, int* shift, int* bins) {
  int nb = 0;
  while (((int64_t)1 << nb) < range) ++nb;
  if (range <= 0) { *levels = 0; shift[0] = shift[1] = shift[2] = 0; bins[0] = bins[1] = bins[2] = 0; return; }
  shift[0] = nb > 11 ? nb - 11 : 0;
  bins[0] = (int)((range + ((int64_t)1 << shift[0]) - 1) >> shift[0]);
  if (shift[0] == 0) { *levels = 1; shift[1] = shift[2] = 0; bins[1] = bins[2] = 0; return; }
  shift[1] = shift[0] > 12 ? shift[0] - 12 : 0;
  bins[1] = 1 << (shift[0] - shift[1]);
  if (shift[1] == 0) { *levels = 2; shift[2] = 0; bins[2] = 0; return; }
  shift[2] = 0;
  bins[2] = 1 << shift[1];
  *levels = 3;
}

__device__ __forceinline__ float prob_of_nll(float nll) { return expf(-nll); }

// A label takes part in the loss iff it is not ignore_label AND names a class.  The reference indexes
// prob[target] / weight[target] with it (loss_opr.py:82-83,98), which device-asserts on anything else; here such a
// pixel is dropped like an ignored one and counted (sel[5]), so no kernel ever indexes weight[] / the class loop
// with an unchecked value.
__device__ __forceinline__ bool label_is_class(int64_t lab, int64_t ignore_label, int C) {
  return lab != ignore_label && (uint64_t)lab < (uint64_t)C;
}

template <int LT> struct Lab;
// raw_t / get_raw / widen: a label as the load instruction leaves it in its register(s).  A prefetching loop keeps THAT
// and widens at the use (behind an asm barrier): any arithmetic on a loaded value, the zero-extension included, is
// scheduled right behind the load and drags the s_waitcnt for it along.
template <> struct Lab<TSG_I64> {
  typedef int64_t type;
  typedef int64_t raw_t;
  static __device__ __forceinline__ int64_t get(const void* p, int64_t i) { return ((const int64_t*)p)[i]; }
  static __device__ __forceinline__ raw_t get_raw(const void* p, int64_t i) { return ((const int64_t*)p)[i]; }
  static __device__ __forceinline__ int64_t widen(raw_t r) { asm volatile("" : "+v"(r)); return r; }
};
template <> struct Lab<TSG_U8> {
  typedef uint8_t type;
  typedef uint32_t raw_t;
  static __device__ __forceinline__ int64_t get(const void* p, int64_t i) { return (int64_t)((const uint8_t*)p)[i]; }
  static __device__ __forceinline__ raw_t get_raw(const void* p, int64_t i) { return ((const uint8_t*)p)[i]; }
  static __device__ __forceinline__ int64_t widen(raw_t r) { asm volatile("" : "+v"(r)); return (int64_t)(r & 0xffu); }
};

template <typename T, int V> struct PixVec;
template <> struct PixVec<float, 4> : Vec<float> {};
template <> struct PixVec<bf16_t, 8> : Vec<bf16_t> {};
template <typename T> struct PixVec<T, 1> {
  float v[1];
  __device__ __forceinline__ void load(const T* p) { v[0] = ld1<T>(p); }
  __device__ __forceinline__ void store(T* p) const { st1<T>(p, v[0]); }
};

// per-thread running sums of pass A (both outcomes of the threshold decision are
// prepared, see ohem_decide0) and their deterministic block fold
struct PassAcc {
  float sum_le = 0.f, sum_valid = 0.f, wsum_le = 0.f, wsum_valid = 0.f;
  int cnt_le_all = 0, cnt_le_valid = 0, cnt_valid = 0, cnt_bad = 0;
};

__device__ __forceinline__ void account(PassAcc& a, bool valid, float nl, float w, float thresh,
                                        int64_t tb, int shift0, int bins0, uint32_t* lh) {
  const float pr = valid ? prob_of_nll(nl) : 1.f;  // masked_fill_(~valid, 1), loss_opr.py:81
  if (valid) { a.cnt_valid++; a.sum_valid += w * nl; a.wsum_valid += w; }
  if (pr <= thresh) {
    a.cnt_le_all++;
    if (valid) { a.cnt_le_valid++; a.sum_le += w * nl; a.wsum_le += w; }
  } else if (bins0 > 0) {
    const int64_t d = (int64_t)__float_as_uint(pr) - tb - 1;
    int bin = (int)(d >> shift0);
    bin = bin < 0 ? 0 : (bin >= bins0 ? bins0 - 1 : bin);   // NaN logits must not index outside the histogram
    atomicAdd(&lh[bin], 1u);
  }
}

// flush the LDS histogram and write this block's partial (fixed order); contains barriers
__device__ __forceinline__ void fold_block(PassAcc& a, const uint32_t* lh, int bins0,
                                           uint32_t* __restrict__ hist0, BlkPart* __restrict__ part) {
  __shared__ float fsm[4 * (kT / 64)];
  __shared__ int ism[4 * (kT / 64)];
  const int tid = threadIdx.x;
  __syncthreads();
  for (int i = tid; i < bins0; i += kT) {
    const uint32_t h = lh[i];
    if (h) atomicAdd(&hist0[i], h);
  }
  a.sum_le = wave_sum(a.sum_le); a.sum_valid = wave_sum(a.sum_valid);
  a.wsum_le = wave_sum(a.wsum_le); a.wsum_valid = wave_sum(a.wsum_valid);
  a.cnt_le_all = wave_sum(a.cnt_le_all); a.cnt_le_valid = wave_sum(a.cnt_le_valid); a.cnt_valid = wave_sum(a.cnt_valid);
  a.cnt_bad = wave_sum(a.cnt_bad);
  const int lane = tid & 63, wv = tid >> 6;
  if (lane == 0) {
    fsm[wv * 4 + 0] = a.sum_le; fsm[wv * 4 + 1] = a.sum_valid; fsm[wv * 4 + 2] = a.wsum_le; fsm[wv * 4 + 3] = a.wsum_valid;
    ism[wv * 4 + 0] = a.cnt_le_all; ism[wv * 4 + 1] = a.cnt_le_valid; ism[wv * 4 + 2] = a.cnt_valid; ism[wv * 4 + 3] = a.cnt_bad;
  }
  __syncthreads();
  if (tid == 0) {
    BlkPart bp = {0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0};
    for (int i = 0; i < kT / 64; ++i) {
      bp.sum_le += fsm[i * 4 + 0]; bp.sum_valid += fsm[i * 4 + 1];
      bp.wsum_le += fsm[i * 4 + 2]; bp.wsum_valid += fsm[i * 4 + 3];
      bp.cnt_le_all += ism[i * 4 + 0]; bp.cnt_le_valid += ism[i * 4 + 1]; bp.cnt_valid += ism[i * 4 + 2]; bp.cnt_bad += ism[i * 4 + 3];
    }
    part[blockIdx.x] = bp;
  }
}

// =============================================================================
// pass A
// =============================================================================
template <typename T, int V, int LT>
__global__ __launch_bounds__(kT) void ohem_pass_a(
    const T* __restrict__ logits, const void* __restrict__ labels, int64_t P, int C,
    int64_t HW, int64_t ignore_label, float thresh, int64_t tb, int shift0, int bins0,
    const float* __restrict__ weight, float* __restrict__ nll_out,
    float* __restrict__ lse_out, uint32_t* __restrict__ hist0, BlkPart* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lh[];  // bins0 + reduction scratch
  const int tid = threadIdx.x;
  for (int i = tid; i < bins0; i += kT) lh[i] = 0;
  __syncthreads();

  PassAcc acc;
  const int64_t nvec = P / V;  // V divides HW (checked on the host) hence P
  for (int64_t v = (int64_t)blockIdx.x * kT + tid; v < nvec; v += (int64_t)gridDim.x * kT) {
    const int64_t p0 = v * V;
    const int64_t b = p0 / HW;
    const int64_t q = p0 - b * HW;
    const T* base = logits + (b * C) * HW + q;
    int t[V];
    bool valid[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t lab = Lab<LT>::get(labels, p0 + j);
      valid[j] = label_is_class(lab, ignore_label, C);
      if (!valid[j] && lab != ignore_label) acc.cnt_bad++;
      t[j] = valid[j] ? (int)lab : 0;  // loss_opr.py:72
    }
    float m[V], s[V], xt[V];
    {
      PixVec<T, V> px;
      px.load(base);
#pragma unroll
      for (int j = 0; j < V; ++j) { m[j] = px.v[j]; s[j] = 1.f; xt[j] = px.v[j]; }
    }
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
      PixVec<T, V> px;
      px.load(base + (int64_t)c * HW);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float x = px.v[j];
        if (t[j] == c) xt[j] = x;
        const float mn = fmaxf(m[j], x);
        s[j] = s[j] * __expf(m[j] - mn) + __expf(x - mn);
        m[j] = mn;
      }
    }
    float nl[V], ls[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      ls[j] = m[j] + logf(s[j]);
      float n_ = ls[j] - xt[j];
      n_ = n_ < 0.f ? 0.f : n_;
      nl[j] = valid[j] ? n_ : 0.f;
    }
    // side arrays (vector stores when V is the native width)
    if (V == 4) {
      *reinterpret_cast<float4*>(nll_out + p0) = make_float4(nl[0], nl[1 % V], nl[2 % V], nl[3 % V]);
      *reinterpret_cast<float4*>(lse_out + p0) = make_float4(ls[0], ls[1 % V], ls[2 % V], ls[3 % V]);
    } else if (V == 8) {
      *reinterpret_cast<float4*>(nll_out + p0) = make_float4(nl[0], nl[1 % V], nl[2 % V], nl[3 % V]);
      *reinterpret_cast<float4*>(nll_out + p0 + 4) = make_float4(nl[4 % V], nl[5 % V], nl[6 % V], nl[7 % V]);
      *reinterpret_cast<float4*>(lse_out + p0) = make_float4(ls[0], ls[1 % V], ls[2 % V], ls[3 % V]);
      *reinterpret_cast<float4*>(lse_out + p0 + 4) = make_float4(ls[4 % V], ls[5 % V], ls[6 % V], ls[7 % V]);
    } else {
      nll_out[p0] = nl[0];
      lse_out[p0] = ls[0];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float w = (weight && valid[j]) ? weight[t[j]] : 1.f;
      account(acc, valid[j], nl[j], w, thresh, tb, shift0, bins0, lh);
    }
  }
  fold_block(acc, lh, bins0, hist0, part);
}

// =============================================================================
// decide: single block.  Reduces the block partials (fp64, fixed order), picks
// the branch (loss_opr.py:78-90) and, on the k-th-value branch, walks hist0.
// =============================================================================
// Find the bin that holds rank krem.  Called by ALL 64 lanes of one wave (round 3: the serial walk of one thread over
// up to 4096 bins — a dependent global load per bin — cost 57 + 2 x 159 us per head on trained-like logits, i.e. the whole
// "selection tail" of the k-th-value branch; bench.py's ohem_kth_branch record).  Every lane sums 8 consecutive bins, a
// wave scan locates the lane whose run crosses the rank, that lane walks its 8 bins.  Integers only: the result is the
// one the serial walk gives.
// State hand-over (round 4): the rank and the running prefix come in as REGISTER values of lane 0 and are
// broadcast by shuffles; the crossing lane's results go back to lane 0 by ballot + shuffle, and lane 0 alone writes `st`.
// No lane reads or read-modify-writes global memory another lane wrote a moment earlier (the round-3 version relied on
// the compiler not forwarding non-atomic accesses to a __restrict__ pointer across a fence).  Returns the new prefix
// (valid on lane 0).
__device__ int64_t scan_hist(const uint32_t* hist, int bins, int shift, int64_t krem_lane0, int64_t lo_lane0, SelState* st) {
  constexpr int CH = 8;
  const int lane = threadIdx.x & 63;
  const int64_t r = __shfl(krem_lane0, 0, 64);
  int64_t cum = 0;
  bool done = false, mine = false;
  int64_t my_krem = 0, my_add = 0;
  for (int base = 0; base < bins && !done; base += 64 * CH) {
    uint32_t h[CH];
    int64_t sum = 0;
    const int b0 = base + lane * CH;
#pragma unroll
    for (int j = 0; j < CH; ++j) { h[j] = b0 + j < bins ? hist[b0 + j] : 0u; sum += h[j]; }
    int64_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const int64_t total = __shfl(incl, 63, 64);
    if (cum + total >= r) {                              // wave-uniform: r, cum and total are
      const int64_t excl = incl - sum;
      if (cum + excl < r && cum + incl >= r) {          // exactly one lane: the first whose run reaches the rank
        int64_t c = cum + excl;
        int j = 0;
        for (; j < CH - 1; ++j) {
          if (c + h[j] >= r) break;
          c += h[j];
        }
        mine = true;
        my_krem = r - c;
        my_add = (int64_t)(b0 + j) << shift;
      }
      done = true;
    } else {
      cum += total;
    }
  }
  const unsigned long long who = __ballot(mine);
  int64_t new_krem, add;
  if (who) {
    const int src = __ffsll((long long)who) - 1;
    new_krem = __shfl(my_krem, src, 64);
    add = __shfl(my_add, src, 64);
  } else {                                               // cannot happen when counts are consistent
    new_krem = r - cum;
    add = (int64_t)(bins - 1) << shift;
  }
  const int64_t lo = lo_lane0 + add;
  if (lane == 0) {
    st->krem = new_krem;
    st->lo_d = lo;
  }
  return lo;
}

__global__ __launch_bounds__(kT) void ohem_decide0(
    const BlkPart* __restrict__ part, int grid, const uint32_t* __restrict__ hist0, int bins0,
    int shift0, int levels, int64_t P, int64_t min_kept, float thresh, int64_t tb,
    int weighted, SelState* __restrict__ st) {
  __shared__ double dsm[4][kT / 64];
  __shared__ long long lsm[3][kT / 64];
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  long long c0 = 0, c1 = 0, c2 = 0;
  int nbad = 0;
  // fixed assignment of partials to threads, fixed combine order => deterministic
  for (int i = threadIdx.x; i < grid; i += kT) {
    const BlkPart bp = part[i];
    a0 += bp.sum_le; a1 += bp.sum_valid; a2 += bp.wsum_le; a3 += bp.wsum_valid;
    c0 += bp.cnt_le_all; c1 += bp.cnt_le_valid; c2 += bp.cnt_valid;
    nbad += bp.cnt_bad;
  }
  if (threadIdx.x == 0) st->n_bad = 0;
  __syncthreads();
  if (nbad) atomicAdd(&st->n_bad, nbad);   // integer: order-independent
  a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
  c0 = (long long)wave_sum((double)c0); c1 = (long long)wave_sum((double)c1); c2 = (long long)wave_sum((double)c2);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    dsm[0][wv] = a0; dsm[1][wv] = a1; dsm[2][wv] = a2; dsm[3][wv] = a3;
    lsm[0][wv] = c0; lsm[1][wv] = c1; lsm[2][wv] = c2;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;                         // wave 0 stays: lane 0 decides, all 64 lanes walk the histogram
  int branch = 0;
  int64_t krem0 = 0;                                     // rank inside hist0 (lane 0)
  if (threadIdx.x == 0) {
    a0 = a1 = a2 = a3 = 0; c0 = c1 = c2 = 0;
    for (int i = 0; i < kT / 64; ++i) {
      a0 += dsm[0][i]; a1 += dsm[1][i]; a2 += dsm[2][i]; a3 += dsm[3][i];
      c0 += lsm[0][i]; c1 += lsm[1][i]; c2 += lsm[2][i];
    }
    const int64_t num_valid = c2, cnt_le_all = c0, cnt_le_valid = c1;
    st->num_valid = num_valid;
    st->lo_d = 0;
    const int64_t k = P < min_kept ? P : min_kept;  // loss_opr.py:87
    if (min_kept > num_valid || num_valid == 0 || min_kept <= 0) {
      // loss_opr.py:78-80 (only logs) / :80 num_valid == 0 / :85 min_kept == 0: plain CE
      branch = 2;
      st->n_kept = num_valid;
      st->sum = a1;
      st->wsum = weighted ? a3 : (double)num_valid;
      st->thr_bits = 0x7f800000u;  // +inf: everything valid is kept
    } else if (k <= cnt_le_all || levels == 0) {
      branch = 0;  // k-th smallest <= thresh  =>  threshold stays thresh (loss_opr.py:84,88)
      st->n_kept = cnt_le_valid;
      st->sum = a0;
      st->wsum = weighted ? a2 : (double)cnt_le_valid;
      st->thr_bits = __float_as_uint(thresh);
    } else {
      branch = 1;
      krem0 = k - cnt_le_all;
    }
    st->branch = branch;
  }
  branch = __shfl(branch, 0, 64);
  if (branch != 1) return;
  const int64_t lo = scan_hist(hist0, bins0, shift0, krem0, 0, st);      // lane 0 writes st->krem / st->lo_d
  if (threadIdx.x == 0 && levels == 1) st->thr_bits = (uint32_t)(lo + tb + 1);
}

// refinement level l >= 1: histogram of the sub-bin index of every element
// whose d lies inside the current prefix [lo_d, lo_d + 2^shift_prev).
template <int XF>
__global__ __launch_bounds__(kT) void sel_refine(
    const float* __restrict__ v, int64_t n, float thresh, int64_t tb, int shift_prev,
    int shift, int bins, uint32_t* __restrict__ hist, const SelState* __restrict__ st) {
  if (st->branch != 1) return;
  extern __shared__ __attribute__((aligned(16))) uint32_t lh[];
  for (int i = threadIdx.x; i < bins; i += kT) lh[i] = 0;
  __syncthreads();
  const int64_t lo = st->lo_d, hi = lo + ((int64_t)1 << shift_prev);
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
    const float pr = XF ? prob_of_nll(v[i]) : v[i];
    if (pr > thresh) {
      const int64_t d = (int64_t)__float_as_uint(pr) - tb - 1;
      if (d >= lo && d < hi) {
        int bin = (int)((d - lo) >> shift);
        if (bin < bins) atomicAdd(&lh[bin], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += kT) {
    const uint32_t h = lh[i];
    if (h) atomicAdd(&hist[i], h);
  }
}

__global__ void sel_decide(const uint32_t* __restrict__ hist, int bins, int shift, int last,
                           int64_t tb, SelState* __restrict__ st) {
  if (threadIdx.x >= 64 || blockIdx.x != 0 || st->branch != 1) return;     // one wave walks the histogram
  // written by the previous kernel of this stream (ohem_decide0 / the previous level's sel_decide): plain loads
  const int64_t krem = threadIdx.x == 0 ? st->krem : 0, lo0 = threadIdx.x == 0 ? st->lo_d : 0;
  const int64_t lo = scan_hist(hist, bins, shift, krem, lo0, st);
  if (threadIdx.x == 0 && last) st->thr_bits = (uint32_t)(lo + tb + 1);
}

// pass C: re-sum nll over valid & p <= thr (k-th value branch only)
template <int LT>
__global__ __launch_bounds__(kT) void ohem_pass_c(
    const float* __restrict__ nll, const void* __restrict__ labels, int64_t P, int C,
    int64_t ignore_label, const float* __restrict__ weight, const SelState* __restrict__ st,
    float* __restrict__ csum, float* __restrict__ cwsum, int32_t* __restrict__ ccnt) {
  if (st->branch != 1) return;
  __shared__ float sm[2 * (kT / 64)];
  __shared__ int ism[kT / 64];
  const float thr = __uint_as_float(st->thr_bits);
  float s = 0.f, ws = 0.f;
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < P; i += (int64_t)gridDim.x * kT) {
    const int64_t lab = Lab<LT>::get(labels, i);
    if (label_is_class(lab, ignore_label, C)) {
      const float nl = nll[i];
      if (prob_of_nll(nl) <= thr) {
        const float w = weight ? weight[lab] : 1.f;
        s += w * nl; ws += w; cnt++;
      }
    }
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) ism[threadIdx.x >> 6] = cnt;
  block_sum2(s, ws, sm);  // contains a __syncthreads()
  if (threadIdx.x == 0) {
    int c = 0;
    for (int i = 0; i < kT / 64; ++i) c += ism[i];
    csum[blockIdx.x] = s; cwsum[blockIdx.x] = ws; ccnt[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(kT) void ohem_finish(
    const float* __restrict__ csum, const float* __restrict__ cwsum,
    const int32_t* __restrict__ ccnt, int grid, int weighted, SelState* __restrict__ st,
    float* __restrict__ loss, int32_t* __restrict__ sel) {
  __shared__ double dsm[3][kT / 64];
  if (st->branch == 1) {
    double a = 0, b = 0, c = 0;
    for (int i = threadIdx.x; i < grid; i += kT) { a += csum[i]; b += cwsum[i]; c += ccnt[i]; }
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) { dsm[0][threadIdx.x >> 6] = a; dsm[1][threadIdx.x >> 6] = b; dsm[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
      a = b = c = 0;
      for (int i = 0; i < kT / 64; ++i) { a += dsm[0][i]; b += dsm[1][i]; c += dsm[2][i]; }
      st->sum = a;
      st->n_kept = (int64_t)c;
      st->wsum = weighted ? b : c;
    }
  }
  if (threadIdx.x == 0) {
    loss[0] = (float)(st->sum / st->wsum);  // 0/0 -> NaN like CrossEntropyLoss over no pixels
    sel[0] = (int32_t)st->thr_bits;
    sel[1] = (int32_t)(st->n_kept > 0x7fffffffLL ? 0x7fffffff : st->n_kept);
    sel[2] = (int32_t)(st->num_valid > 0x7fffffffLL ? 0x7fffffff : st->num_valid);
    sel[3] = st->branch;
    sel[5] = st->n_bad;
    // denominator as float for the backward pass
    reinterpret_cast<float*>(sel)[4] = (float)st->wsum;
    sel[6] = 0;  // the two spare words of sel[8] (include/tsg_hip.h): written, so the whole tensor is defined
    sel[7] = 0;
  }
}

// =============================================================================
// backward
// =============================================================================
template <typename T, int V, int LT>
__global__ __launch_bounds__(kT) void ohem_bwd_k(
    const T* __restrict__ logits, const void* __restrict__ labels, int64_t P, int C, int64_t HW,
    int64_t ignore_label, const float* __restrict__ weight, const float* __restrict__ nll,
    const float* __restrict__ lse, const int32_t* __restrict__ sel,
    const float* __restrict__ gscale, T* __restrict__ dlogits) {
  const float thr = __uint_as_float((uint32_t)sel[0]);
  const int branch = sel[3];
  const float denom = reinterpret_cast<const float*>(sel)[4];
  const float g = gscale[0] / denom;
  const int64_t nvec = P / V;
  for (int64_t v = (int64_t)blockIdx.x * kT + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * kT) {
    const int64_t p0 = v * V;
    const int64_t b = p0 / HW;
    const int64_t q = p0 - b * HW;
    const int64_t boff = (b * C) * HW + q;
    float coef[V], ls[V];
    int t[V];
    bool any = false;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t lab = Lab<LT>::get(labels, p0 + j);
      const bool valid = label_is_class(lab, ignore_label, C);
      t[j] = valid ? (int)lab : -1;
      bool kept = valid;
      if (valid && branch != 2) kept = prob_of_nll(nll[p0 + j]) <= thr;
      const float w = (weight && valid) ? weight[lab] : 1.f;
      coef[j] = kept ? g * w : 0.f;
      ls[j] = lse[p0 + j];
      any |= kept;
    }
    if (any) {
#pragma unroll 4
      for (int c = 0; c < C; ++c) {
        PixVec<T, V> px;
        px.load(logits + boff + (int64_t)c * HW);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float sm = __expf(px.v[j] - ls[j]);
          px.v[j] = coef[j] * (sm - (t[j] == c ? 1.f : 0.f));
        }
        px.store(dlogits + boff + (int64_t)c * HW);
      }
    } else {
      PixVec<T, V> z;
#pragma unroll
      for (int j = 0; j < V; ++j) z.v[j] = 0.f;
      for (int c = 0; c < C; ++c) z.store(dlogits + boff + (int64_t)c * HW);
    }
  }
}

// =============================================================================
// Fused head: bilinear (align_corners=True) upsample of the low-resolution logits
// evaluated INSIDE the OHEM kernels, so the full-resolution logits (59.8 M
// elements per image for BiSeNet's three heads) are never written or re-read
// (SURVEY.md §8f-1).  z is [B, C, IH, IW]; the virtual logits are [B, C, OH, OW].
//
// Both directions are "column walkers": a thread owns ONE output column ox and
// walks down output rows.  Per class it keeps the horizontally interpolated source
// row H0[c] (row y0) and the row difference D[c] = H1[c] - H0[c] in registers (in
// log2 units: z is multiplied by log2(e) when it is staged in LDS), so a logit
// costs one FMA, v_c = fma(ly, D[c], H0[c]), and the softmax one v_exp_f32 per
// class.  H0 / D change only when y0 advances (every ~scale rows) and are then
// rebuilt from the LDS copy of the two source rows — never from their old values,
// so a pixel's logits do not depend on how the rows were banded.  The class count
// is a compile-time pad CP (classes >= C hold -1e30: exp2 gives 0), the loops have
// no per-class branches.
//   forward : tile = 256 columns x 32 rows; the z window of the tile (<= 6 x 34
//             source pixels x CP) sits in LDS; max / sum-exp2 / log2 in registers;
//             the target logit is re-evaluated from the window with the same
//             expressions (4 LDS reads) instead of a CP-long select chain.
//             HBM: label read + nll / lse write.
//   backward: block = RB source rows x SB source columns of dz, threads = every
//             output column whose taps touch them (neighbouring blocks overlap by
//             one source column / row: each dz element has exactly one owner, no
//             atomics, fixed summation order).  g_c = coef*(softmax_c - [c==t]) is
//             folded into the vertical transposed taps in registers (accA / accB);
//             when a source row is complete the block applies the horizontal
//             transposed taps through LDS and stores the dz row.  The one-hot is
//             a row of an LDS table (ds_read_b128), not a compare chain.
// =============================================================================
constexpr int kFwdBand = 32;                 // output rows per forward tile
constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;
constexpr float kNegBig = -1.0e30f;

typedef __attribute__((ext_vector_type(2))) float up_f2;

struct UpFwdGeom { int C, IH, IW, OH, OW; float sy, sx; int WR, WC, xblocks, bands, hist_words; };

__device__ __forceinline__ void src_index0(float scale, int dst, int in_size, int& i0, int& i1, float& l1) {
  src_index(scale, dst, in_size, i0, i1, l1);
  if (i1 == i0) l1 = 0.f;                    // last source row / column: both taps coincide, weight 1
}

template <typename T, int LT, int CP>
__global__ __launch_bounds__(kT) void ohem_up_fwd_k(
    const T* __restrict__ z, const void* __restrict__ labels, int64_t B, UpFwdGeom g,
    int64_t ignore_label, float thresh, int64_t tb, int shift0, int bins0,
    const float* __restrict__ weight, float* __restrict__ nll_out, float* __restrict__ lse_out,
    uint32_t* __restrict__ hist0, BlkPart* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lh[];       // [hist_words] histogram
  float* Zw = reinterpret_cast<float*>(lh + g.hist_words);            // [CP][WR][WC] window of z * log2(e)
  uint8_t* lab_s = reinterpret_cast<uint8_t*>(Zw + CP * g.WR * g.WC); // [kFwdBand][kT] labels (255 = ignored)
  const int tid = threadIdx.x;
  for (int i = tid; i < bins0; i += kT) lh[i] = 0;
  PassAcc acc;
  const int C = g.C, IH = g.IH, IW = g.IW, OH = g.OH, OW = g.OW, WR = g.WR, WC = g.WC;
  const int64_t total = B * g.bands * (int64_t)g.xblocks;
  const int64_t plane = (int64_t)IH * IW;
  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int xb = (int)(tile % g.xblocks);
    const int band = (int)((tile / g.xblocks) % g.bands);
    const int64_t b = tile / ((int64_t)g.xblocks * g.bands);
    const int oy_beg = band * kFwdBand;
    const int oy_end = oy_beg + kFwdBand < OH ? oy_beg + kFwdBand : OH;
    const int ox = xb * kT + tid;
    const bool live = ox < OW;
    int ys_lo, xs_lo, t1; float tf;
    src_index0(g.sy, oy_beg, IH, ys_lo, t1, tf);
    src_index0(g.sx, xb * kT, IW, xs_lo, t1, tf);
    const T* zb = z + b * C * plane;
    __syncthreads();                                   // the previous tile's readers are done (also orders lh init)
    for (int i = tid; i < CP * WR * WC; i += kT) {
      const int c = i / (WR * WC);
      const int rr = (i / WC) % WR, xx = i % WC;
      const int yy = ys_lo + rr < IH ? ys_lo + rr : IH - 1;
      const int xg = xs_lo + xx < IW ? xs_lo + xx : IW - 1;
      Zw[i] = c < C ? ld1<T>(zb + c * plane + (int64_t)yy * IW + xg) * kLog2e : kNegBig;
    }
    // labels of the whole tile: kFwdBand independent loads in flight per thread; each thread only ever reads
    // back its own column
#pragma unroll 1
    for (int u0 = 0; u0 < kFwdBand; u0 += 8) {
      int64_t lab[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int oy = oy_beg + u0 + u;
        lab[u] = (live && oy < oy_end) ? Lab<LT>::get(labels, (b * OH + oy) * (int64_t)OW + ox) : ignore_label;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool is_cls = label_is_class(lab[u], ignore_label, C);
        if (!is_cls && lab[u] != ignore_label) acc.cnt_bad++;
        lab_s[(u0 + u) * kT + tid] = is_cls ? (uint8_t)lab[u] : (uint8_t)255;
      }
    }
    __syncthreads();
    if (!live) continue;
    int x0, x1; float lx;
    src_index0(g.sx, ox, IW, x0, x1, lx);
    const int xl0 = x0 - xs_lo, xl1 = x1 - xs_lo;
    up_f2 H0[CP / 2], D[CP / 2];                       // class pairs: the lerp / subtract / sum chain runs on v_pk_* (two classes per instruction)
    int cy0 = -1, ro0 = 0, ro1 = 0;
    for (int oy = oy_beg; oy < oy_end; ++oy) {
      int y0, y1; float ly;
      src_index0(g.sy, oy, IH, y0, y1, ly);
      y0 = __builtin_amdgcn_readfirstlane(y0);
      y1 = __builtin_amdgcn_readfirstlane(y1);
      if (y0 != cy0) {
        ro0 = (y0 - ys_lo) * WC; ro1 = (y1 - ys_lo) * WC;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          const float* zr = Zw + c * WR * WC;
          const float a0 = zr[ro0 + xl0], a1 = zr[ro0 + xl1], b0 = zr[ro1 + xl0], b1 = zr[ro1 + xl1];
          const float h0 = __builtin_fmaf(lx, a1 - a0, a0), h1 = __builtin_fmaf(lx, b1 - b0, b0);
          if (c & 1) { H0[c >> 1].y = h0; D[c >> 1].y = h1 - h0; } else { H0[c >> 1].x = h0; D[c >> 1].x = h1 - h0; }
        }
        cy0 = y0;
      }
      up_f2 v[CP / 2];
      const up_f2 ly2 = {ly, ly};
      float m = kNegBig;
#pragma unroll
      for (int c = 0; c < CP / 2; ++c) {
        v[c] = __builtin_elementwise_fma(ly2, D[c], H0[c]);
        m = fmaxf(m, fmaxf(v[c].x, v[c].y));
      }
      const up_f2 m2 = {m, m};
      up_f2 s2 = {0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CP / 2; ++c) {
        const up_f2 d = v[c] - m2;
        s2 += up_f2{__builtin_amdgcn_exp2f(d.x), __builtin_amdgcn_exp2f(d.y)};
      }
      const float ssum = s2.x + s2.y;
      const float l2 = m + __builtin_amdgcn_logf(ssum);
      const int lab = lab_s[(oy - oy_beg) * kT + tid];
      const bool valid = lab != 255;
      const int t = valid ? lab : 0;
      float xt;
      {  // the target logit, by the expressions that produced v[t]
        const float* zr = Zw + t * WR * WC;
        const float a0 = zr[ro0 + xl0], a1 = zr[ro0 + xl1], b0 = zr[ro1 + xl0], b1 = zr[ro1 + xl1];
        const float h0 = __builtin_fmaf(lx, a1 - a0, a0), h1 = __builtin_fmaf(lx, b1 - b0, b0);
        xt = __builtin_fmaf(ly, h1 - h0, h0);
      }
      float nl = (l2 - xt) * kLn2;
      nl = nl < 0.f ? 0.f : nl;
      nl = valid ? nl : 0.f;
      const int64_t gp = (b * OH + oy) * (int64_t)OW + ox;
      nll_out[gp] = nl;
      lse_out[gp] = l2 * kLn2;
      const float w = (weight && valid) ? weight[t] : 1.f;
      account(acc, valid, nl, w, thresh, tb, shift0, bins0, lh);
    }
  }
  fold_block(acc, lh, bins0, hist0, part);
}

// ---- forward, second form (round 5; VERDICT r4 item 4: the first form spent 2.8x the exponential floor on index
// arithmetic).  Same tile (256 columns x 32 rows), same results up to the rounding of the log-sum-exp shift; what changed:
//   * the z window sits in LDS PIXEL-major, [WR x WC][CP]: the four taps of a column are four pixels, and a rebuild of
//     H0 / D reads each as CP / 4 ds_read_b128 (20 LDS instructions for 20 classes; the class-major window took 80
//     ds_read_b32 with an address per class).  Pixels 80 B apart: 16-byte reads of 8 distinct pixels per wave fall on
//     disjoint bank groups;
//   * the window is staged by (class, source row) pairs per WAVE with the source column on the lanes: no integer division
//     per element (the first form: two divisions and a modulo by run-time values for each of its 16 elements per thread);
//   * the softmax shift is an upper BOUND of the pixel's logits instead of their maximum: M = the largest class maximum of
//     the four tap pixels (one pass over the window per tile), folded into H0 when H0 / D are rebuilt, so that
//     v_c = fma(ly, D_c, H0_c) already is logit - M: no 10-step v_max3 chain and no 10 packed subtractions per pixel.  An
//     interpolated logit never exceeds the largest tap logit, so exp2(v_c) <= 1; should every exp2 underflow (taps that
//     disagree by > 100 in log2 units about which class is large) the wave redoes the row with the exact maximum;
//   * the row's (y0, ly) come from a 32-entry LDS table filled once per tile (they were recomputed on the VALU by every
//     thread for every row), nll / lse addresses advance by a row stride.
template <typename T, int LT, int CP>
__global__ __launch_bounds__(kT) void ohem_up_fwd2_k(
    const T* __restrict__ z, const void* __restrict__ labels, int64_t B, UpFwdGeom g,
    int64_t ignore_label, float thresh, int64_t tb, int shift0, int bins0,
    const float* __restrict__ weight, float* __restrict__ nll_out, float* __restrict__ lse_out,
    uint32_t* __restrict__ hist0, BlkPart* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lh[];       // [hist_words] histogram
  const int C = g.C, IH = g.IH, IW = g.IW, OH = g.OH, OW = g.OW, WR = g.WR, WC = g.WC;
  const int npix = WR * WC;
  float* Zw = reinterpret_cast<float*>(lh + g.hist_words);            // [npix][CP] window of z * log2(e), pixel-major
  float* Zmax = Zw + (size_t)npix * CP;                               // [npix] class maximum of each window pixel
  int* yro = reinterpret_cast<int*>(Zmax + ((npix + 3) & ~3));        // [kFwdBand] window pixel offset of the row's y0
  float* yly = reinterpret_cast<float*>(yro + kFwdBand);              // [kFwdBand] lambda_y of the row
  float* wtab = yly + kFwdBand;                                       // [32] class weights (1 without a weight vector): no
  //                                                                     global load, hence no vmcnt wait, in the row loop
  uint8_t* lab_s = reinterpret_cast<uint8_t*>(wtab + 32);             // [kFwdBand][kT] labels (255 = ignored)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < bins0; i += kT) lh[i] = 0;
  if (tid < 32) wtab[tid] = (weight && tid < g.C) ? weight[tid] : 1.f;
  PassAcc acc;
  const int64_t total = B * g.bands * (int64_t)g.xblocks;
  const int64_t plane = (int64_t)IH * IW;
  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int xb = (int)(tile % g.xblocks);
    const int band = (int)((tile / g.xblocks) % g.bands);
    const int64_t b = tile / ((int64_t)g.xblocks * g.bands);
    const int oy_beg = band * kFwdBand;
    const int oy_end = oy_beg + kFwdBand < OH ? oy_beg + kFwdBand : OH;
    const int ox = xb * kT + tid;
    const bool live = ox < OW;
    int ys_lo, xs_lo, t1; float tf;
    src_index0(g.sy, oy_beg, IH, ys_lo, t1, tf);
    src_index0(g.sx, xb * kT, IW, xs_lo, t1, tf);
    const T* zb = z + b * C * plane;
    __syncthreads();                                   // the previous tile's readers are done (also orders lh init)
    // window: wave wv takes the (class, row) pairs wv, wv + 4, ...; lanes = source columns.  EIGHT pairs' loads are in
    // flight per wave before the first LDS write (one load -> one write per iteration was a chain of 30 L2 round trips per
    // tile and held the VALU at 0.68 busy: profiles/r05_heads.txt)
    for (int x0s = 0; x0s < WC; x0s += 64) {
      const int xx = x0s + lane;
      const int xg = xs_lo + xx < IW ? xs_lo + xx : IW - 1;
      const bool xin = xx < WC;
      int c = 0, rr = wv;
      while (rr >= WR) { rr -= WR; ++c; }
      while (c < CP) {
        float val[8];
        int off[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          // UNCONDITIONAL loads from clamped addresses, the condition applied to the value: a load inside a divergent
          // branch is followed by s_waitcnt vmcnt(0) at the end of that branch, i.e. one memory round trip per element
          const bool on = c < CP;
          const int yy = ys_lo + rr < IH ? ys_lo + rr : IH - 1;
          const int cc = c < C ? c : C - 1;
          const float raw = ld1<T>(zb + (int64_t)cc * plane + (int64_t)yy * IW + xg) * kLog2e;
          val[u] = c < C ? raw : kNegBig;
          off[u] = (on && xin) ? (rr * WC + xx) * CP + c : -1;
          rr += kT / 64;
          while (rr >= WR) { rr -= WR; ++c; }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (off[u] >= 0) Zw[off[u]] = val[u];
      }
    }
    if (tid < kFwdBand) {
      int y0, y1; float ly;
      const int oy = oy_beg + tid < OH ? oy_beg + tid : OH - 1;
      src_index0(g.sy, oy, IH, y0, y1, ly);
      yro[tid] = (y0 - ys_lo) * WC;
      yly[tid] = ly;
    }
    // labels of the whole tile: kFwdBand independent loads in flight per thread; each thread only ever reads
    // back its own column
#pragma unroll 1
    for (int u0 = 0; u0 < kFwdBand; u0 += 16) {
      int64_t lab[16];
      const int oxc = ox < OW ? ox : OW - 1;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int oy = oy_beg + u0 + u;
        const int oyc = oy < OH ? oy : OH - 1;
        const int64_t v = Lab<LT>::get(labels, (b * OH + oyc) * (int64_t)OW + oxc);     // unconditional, clamped (see above)
        lab[u] = (live && oy < oy_end) ? v : ignore_label;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const bool is_cls = label_is_class(lab[u], ignore_label, C);
        if (!is_cls && lab[u] != ignore_label) acc.cnt_bad++;
        lab_s[(u0 + u) * kT + tid] = is_cls ? (uint8_t)lab[u] : (uint8_t)255;
      }
    }
    __syncthreads();
    for (int p = tid; p < npix; p += kT) {             // class maximum of every window pixel (padding classes hold -1e30)
      const float4* zp = reinterpret_cast<const float4*>(Zw + (size_t)p * CP);
      float m = kNegBig;
#pragma unroll
      for (int q = 0; q < CP / 4; ++q) { const float4 t = zp[q]; m = fmaxf(fmaxf(m, fmaxf(t.x, t.y)), fmaxf(t.z, t.w)); }
      Zmax[p] = m;
    }
    __syncthreads();
    if (!live) continue;
    int x0, x1; float lx;
    src_index0(g.sx, ox, IW, x0, x1, lx);
    const int xl0 = x0 - xs_lo;                        // x1 = x0 + 1 except on the last source column, where lx = 0 and the
    //                                                    window's clamped copy of that column sits at xl0 + 1
    up_f2 H0[CP / 2], D[CP / 2];                       // H0 already holds (row-y0 logit - M)
    const up_f2 lx2 = {lx, lx};
    float M = 0.f;
    int cro = -1, p00 = 0;
    float* nll_p = nll_out + (b * OH + oy_beg) * (int64_t)OW + ox;
    float* lse_p = lse_out + (b * OH + oy_beg) * (int64_t)OW + ox;
    const int nrows = oy_end - oy_beg;
    for (int r = 0; r < nrows; ++r, nll_p += OW, lse_p += OW) {
      const int ro = __builtin_amdgcn_readfirstlane(yro[r]);
      const float ly = yly[r];
      if (ro != cro) {
        p00 = (ro + xl0) * CP;
        const float* zm = Zmax + ro + xl0;
        M = fmaxf(fmaxf(zm[0], zm[1]), fmaxf(zm[WC], zm[WC + 1]));
        const float4* A0 = reinterpret_cast<const float4*>(Zw + p00);
        const float4* A1 = reinterpret_cast<const float4*>(Zw + p00 + CP);
        const float4* B0 = reinterpret_cast<const float4*>(Zw + p00 + WC * CP);
        const float4* B1 = reinterpret_cast<const float4*>(Zw + p00 + WC * CP + CP);
        const up_f2 M2 = {M, M};
#pragma unroll
        for (int q = 0; q < CP / 4; ++q) {
          const float4 a0 = A0[q], a1 = A1[q], b0 = B0[q], b1 = B1[q];
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const up_f2 a0p = k ? up_f2{a0.z, a0.w} : up_f2{a0.x, a0.y};
            const up_f2 a1p = k ? up_f2{a1.z, a1.w} : up_f2{a1.x, a1.y};
            const up_f2 b0p = k ? up_f2{b0.z, b0.w} : up_f2{b0.x, b0.y};
            const up_f2 b1p = k ? up_f2{b1.z, b1.w} : up_f2{b1.x, b1.y};
            const up_f2 h0 = __builtin_elementwise_fma(lx2, a1p - a0p, a0p);
            const up_f2 h1 = __builtin_elementwise_fma(lx2, b1p - b0p, b0p);
            H0[q * 2 + k] = h0 - M2;
            D[q * 2 + k] = h1 - h0;
          }
        }
        cro = ro;
      }
      up_f2 v[CP / 2];
      const up_f2 ly2 = {ly, ly};
      up_f2 s2 = {0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CP / 2; ++c) {
        v[c] = __builtin_elementwise_fma(ly2, D[c], H0[c]);
        s2 += up_f2{__builtin_amdgcn_exp2f(v[c].x), __builtin_amdgcn_exp2f(v[c].y)};
      }
      float ssum = s2.x + s2.y;
      float lr = __builtin_amdgcn_logf(ssum);          // log2(sum exp2(logit - M))
      if (__builtin_amdgcn_ballot_w64(!(ssum >= 1.0e-30f)) != 0) {
        // every term underflowed somewhere in this wave (or a NaN): the row again with the exact maximum
        float m = kNegBig;
#pragma unroll
        for (int c = 0; c < CP / 2; ++c) m = fmaxf(m, fmaxf(v[c].x, v[c].y));
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CP / 2; ++c) s += __builtin_amdgcn_exp2f(v[c].x - m) + __builtin_amdgcn_exp2f(v[c].y - m);
        lr = m + __builtin_amdgcn_logf(s);
      }
      const int lab = lab_s[r * kT + tid];
      const bool valid = lab != 255;
      const int t = valid ? lab : 0;
      float xt;
      {  // the target logit (- M), by the expressions that produced v[t]
        const float a0 = Zw[p00 + t], a1 = Zw[p00 + CP + t], b0 = Zw[p00 + WC * CP + t], b1 = Zw[p00 + WC * CP + CP + t];
        const float h0 = __builtin_fmaf(lx, a1 - a0, a0), h1 = __builtin_fmaf(lx, b1 - b0, b0);
        xt = __builtin_fmaf(ly, h1 - h0, h0 - M);
      }
      float nl = (lr - xt) * kLn2;
      nl = nl < 0.f ? 0.f : nl;
      nl = valid ? nl : 0.f;
      *nll_p = nl;
      *lse_p = (lr + M) * kLn2;
      const float w = wtab[t];
      account(acc, valid, nl, w, thresh, tb, shift0, bins0, lh);
    }
  }
  fold_block(acc, lh, bins0, hist0, part);
}

struct UpBwdGeom { int C, IH, IW, OH, OW; float sy, sx; int RB, SB, XS; };

constexpr int kWideMaxC = 256;

// WIDE (33..256 classes): with lse saved the classes are independent, so a block takes one chunk of CP classes, [c0,
// c0 + Cc), the chunk being part of blockIdx.z (nchunk per image).  z / dz keep the full C stride.
template <typename T, int LT, int CP, int NTMAX, bool WIDE>
__global__ __launch_bounds__(NTMAX) void ohem_up_bwd_k(
    const T* __restrict__ z, const void* __restrict__ labels, UpBwdGeom g, int nchunk, int64_t ignore_label,
    const float* __restrict__ weight, const float* __restrict__ nll, const float* __restrict__ lse,
    const int32_t* __restrict__ sel, const float* __restrict__ gscale, T* __restrict__ dz) {
  constexpr int VP = CP + 1;                          // odd row stride: column-major writes and class-major reads both spread over the banks
  constexpr int OHR = WIDE ? CP + 1 : CP;             // one-hot rows; WIDE: row CP (target outside the chunk) is zero
  constexpr int WT = WIDE ? kWideMaxC : CP;           // weight table entries: every class a label can name
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int NT = blockDim.x, tid = threadIdx.x;
  const int C = g.C, IH = g.IH, IW = g.IW, OH = g.OH, OW = g.OW, XS = g.XS;
  float* oh = smem;                                   // [OHR][CP] one-hot rows (16-byte aligned rows: CP % 4 == 0)
  float* Zr = oh + OHR * CP;                          // [2][CP][XS] the two live source rows * log2(e)
  float* lxs = Zr + 2 * CP * XS;                      // [NT] lambda_x of every column of the block
  float* Vs = lxs + NT;                               // [NT][VP] a completed source row, before the horizontal taps
  int* xst = reinterpret_cast<int*>(Vs + NT * VP);    // [XS + 2] first column whose x0 is xs_lo + j
  float* wtab = reinterpret_cast<float*>(xst + XS + 2);   // [WT] class weight: read per pixel from LDS, so that the row
  //                                                         loop holds no global load whose wait would also wait for the
  //                                                         prefetched next row (round 5: SQ_WAIT_ANY 0.54 was this)
  const int s0 = blockIdx.x * g.SB, s1 = s0 + g.SB < IW ? s0 + g.SB : IW;
  const int r0 = blockIdx.y * g.RB, r1 = r0 + g.RB < IH ? r0 + g.RB : IH;
  const int64_t b = WIDE ? blockIdx.z / nchunk : blockIdx.z;
  const int c0 = WIDE ? (int)(blockIdx.z % nchunk) * CP : 0;          // this block's classes: [c0, c0 + Cc)
  const int Cc = WIDE ? (C - c0 < CP ? C - c0 : CP) : C;
  int xlo, xhi, tmp;
  footprint(g.sx, s0, OW, xlo, tmp);
  footprint(g.sx, s1 - 1, OW, tmp, xhi);
  const int nact = xhi - xlo + 1;                     // <= NT (host)
  const bool live = tid < nact;
  const int ox = live ? xlo + tid : xhi;
  int x0, x1, xs_lo; float lx, tf;
  src_index0(g.sx, ox, IW, x0, x1, lx);
  src_index0(g.sx, xlo, IW, xs_lo, tmp, tf);
  const int xl0 = x0 - xs_lo, xl1 = x1 - xs_lo;
  lxs[tid] = live ? lx : 0.f;
  for (int i = tid; i < OHR * CP; i += NT) oh[i] = (i / CP == i % CP) ? 1.f : 0.f;
  for (int j = tid; j < XS + 2; j += NT) xst[j] = nact;
  if constexpr (WIDE) { for (int i = tid; i < WT; i += NT) wtab[i] = (weight && i < C) ? weight[i] : 1.f; }
  else if (tid < WT) wtab[tid] = (weight && tid < C) ? weight[tid] : 1.f;
  __syncthreads();
  if (live) {
    int p0 = -1, p1; float pf;
    if (tid > 0) src_index0(g.sx, ox - 1, IW, p0, p1, pf);
    if (p0 != x0) xst[xl0] = tid;                     // OW >= 2 IW: x0 advances by at most 1 per column
  }
  const float thr = __uint_as_float((uint32_t)sel[0]);
  const int branch = sel[3];
  const float gs = gscale[0] / reinterpret_cast<const float*>(sel)[4];
  const int64_t plane = (int64_t)IH * IW;
  const T* zb = z + (b * C + c0) * plane;
  // output rows whose y0 lies in [r0-1, r1-1]
  int oy_lo = 0, oy_hi = OH - 1;
  if (g.sy > 0.f) {
    const float inv = 1.f / g.sy;
    const int l = (int)ceilf((float)(r0 - 1) * inv) - 1;
    const int h = (int)floorf((float)r1 * inv) + 1;
    oy_lo = l < 0 ? 0 : l;
    oy_hi = h > OH - 1 ? OH - 1 : h;
  }
  // class pairs in even-aligned register pairs: the per-pixel chain (lerp, subtract lse, subtract one-hot, two
  // accumulations) runs on v_pk_fma_f32 / v_pk_add_f32, two classes per instruction; only the exp2 stays scalar
  up_f2 H0[CP / 2], D[CP / 2], accA[CP / 2], accB[CP / 2];
#pragma unroll
  for (int c = 0; c < CP / 2; ++c) { accA[c] = up_f2{0.f, 0.f}; accB[c] = up_f2{0.f, 0.f}; H0[c] = up_f2{0.f, 0.f}; D[c] = up_f2{0.f, 0.f}; }
  int cur = -2;                                       // source row accA belongs to (accB: cur + 1)
  int staged0 = -1, staged1 = -1;                     // source rows held by the two ring slots

  auto flush = [&](int row, const up_f2 (&a)[CP / 2]) {   // block-uniform
    if (row < r0 || row >= r1) return;
    __syncthreads();                                  // the previous horizontal pass has read Vs
#pragma unroll
    for (int c = 0; c < CP / 2; ++c) {
      Vs[tid * VP + 2 * c] = live ? a[c].x : 0.f;
      Vs[tid * VP + 2 * c + 1] = live ? a[c].y : 0.f;
    }
    __syncthreads();
    const int nS = s1 - s0;
    for (int idx = tid; idx < Cc * nS; idx += NT) {
      const int c = idx % Cc, s = s0 + idx / Cc, j = s - xs_lo;
      float sum = 0.f;
      const int xa = xst[j], xb = xst[j + 1];
      for (int x = xa; x < xb; ++x) sum = __builtin_fmaf(1.f - lxs[x], Vs[x * VP + c], sum);
      if (j >= 1) {
        const int xp = xst[j - 1];
        for (int x = xp; x < xa; ++x) sum = __builtin_fmaf(lxs[x], Vs[x * VP + c], sum);
      }
      st1<T>(dz + ((b * C + c0 + c) * IH + row) * (int64_t)IW + s, sum);
    }
  };
  auto stage = [&](int slot, int y) {
    for (int i = tid; i < CP * XS; i += NT) {
      const int c = i / XS, xx = i % XS;
      const int xg = xs_lo + xx < IW ? xs_lo + xx : IW - 1;
      Zr[slot * CP * XS + i] = c < Cc ? ld1<T>(zb + c * plane + (int64_t)y * IW + xg) * kLog2e : kNegBig;
    }
  };
  struct Side { typename Lab<LT>::raw_t lab; float nl, ls; };
  auto load_side = [&](int oy) {
    Side sd;
    const int64_t gp = (b * OH + oy) * (int64_t)OW + ox;
    // unconditional (ox is clamped) and NOT touched here: a load inside a divergent branch is waited for at the end of that
    // branch, and so is a loaded value the moment anything (even `live ? v : ignore`) consumes it — either way the
    // prefetch of the next row degenerated into one exposed memory round trip per row (round 5: SQ_WAIT_ANY 0.54).
    // `live` is applied where the label is used.
    sd.lab = Lab<LT>::get_raw(labels, gp);
    sd.nl = nll[gp];
    sd.ls = lse[gp];
    return sd;
  };
  Side nxt = load_side(oy_lo);
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    const Side sd = nxt;
    if (oy < oy_hi) nxt = load_side(oy + 1);
    int y0, y1; float ly;
    src_index0(g.sy, oy, IH, y0, y1, ly);
    y0 = __builtin_amdgcn_readfirstlane(y0);
    y1 = __builtin_amdgcn_readfirstlane(y1);
    if (y0 < r0 - 1 || y0 > r1 - 1) continue;
    if (y0 != cur) {
      if (cur >= 0) {
        flush(cur, accA);
        if (y0 == cur + 1) {
#pragma unroll
          for (int c = 0; c < CP / 2; ++c) { accA[c] = accB[c]; accB[c] = up_f2{0.f, 0.f}; }
        } else {
          flush(cur + 1, accB);
#pragma unroll
          for (int c = 0; c < CP / 2; ++c) { accA[c] = up_f2{0.f, 0.f}; accB[c] = up_f2{0.f, 0.f}; }
        }
      }
      __syncthreads();                                // everybody has built H0 / D from the rows about to be replaced
      if (((y0 & 1) ? staged1 : staged0) != y0) { stage(y0 & 1, y0); if (y0 & 1) staged1 = y0; else staged0 = y0; }
      if (y1 != y0 && ((y1 & 1) ? staged1 : staged0) != y1) { stage(y1 & 1, y1); if (y1 & 1) staged1 = y1; else staged0 = y1; }
      __syncthreads();
      const float* za = Zr + (y0 & 1) * CP * XS;
      const float* zc = Zr + (y1 & 1) * CP * XS;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float a0 = za[c * XS + xl0], a1 = za[c * XS + xl1], b0 = zc[c * XS + xl0], b1 = zc[c * XS + xl1];
        const float h0 = __builtin_fmaf(lx, a1 - a0, a0), h1 = __builtin_fmaf(lx, b1 - b0, b0);
        if (c & 1) { H0[c >> 1].y = h0; D[c >> 1].y = h1 - h0; } else { H0[c >> 1].x = h0; D[c >> 1].x = h1 - h0; }
      }
      cur = y0;
    }
    const int64_t lab = Lab<LT>::widen(sd.lab);
    const bool valid = live && label_is_class(lab, ignore_label, C);
    bool kept = valid;
    if (valid && branch != 2) kept = prob_of_nll(sd.nl) <= thr;
    const int t = valid ? (int)lab : 0;
    const float coef = kept ? gs * wtab[t] : 0.f;
    if (__builtin_amdgcn_ballot_w64(coef != 0.f) == 0) continue;      // nothing kept in this wave's 64 columns
    const float l2 = sd.ls * kLog2e;
    const float ca = coef - ly * coef, cb = ly * coef;
    const int ohrow = !WIDE ? t : (valid && (unsigned)(t - c0) < (unsigned)CP) ? t - c0 : CP;   // CP: the zero row
    const float4* ohr = reinterpret_cast<const float4*>(oh + ohrow * CP);
    const up_f2 ly2 = {ly, ly}, l22 = {l2, l2}, ca2 = {ca, ca}, cb2 = {cb, cb};
#pragma unroll
    for (int c4 = 0; c4 < CP / 4; ++c4) {
      const float4 o = ohr[c4];
      const up_f2 ov[2] = {up_f2{o.x, o.y}, up_f2{o.z, o.w}};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int c = c4 * 2 + k;
        const up_f2 v = __builtin_elementwise_fma(ly2, D[c], H0[c]) - l22;
        const up_f2 e = up_f2{__builtin_amdgcn_exp2f(v.x), __builtin_amdgcn_exp2f(v.y)} - ov[k];
        accA[c] = __builtin_elementwise_fma(ca2, e, accA[c]);
        accB[c] = __builtin_elementwise_fma(cb2, e, accB[c]);
      }
    }
  }
  if (cur >= 0) { flush(cur, accA); flush(cur + 1, accB); }
}

// =============================================================================
// Fused head for 33 <= C <= 256 classes (ADE20K: 150).  The narrow kernels above keep every class of a pixel in
// registers; here the classes are walked in chunks of CP.
//   forward : the same 256 x 32 tile.  Per chunk the z window of CP classes is staged in LDS (pixel-major, as in
//             ohem_up_fwd2_k) and every row of the tile folds the chunk into an ONLINE softmax state held in registers
//             per row: running maximum m[r] and sum s[r] of exp2(logit - m[r]), rescaled when the maximum moves: exact,
//             no underflow case.  The target logit is taken from the window of the chunk that holds the target class,
//             with the expressions that produce v[t].  The row loop is unrolled (the state is indexed by the row).
//             Labels sit in LDS as 16-bit values (0xffff = takes no part): class 255 is a class when C = 256.
//   backward: ohem_up_bwd_k<..., WIDE = true> above, one block per class chunk.  One owner per dz element.
// =============================================================================
constexpr int kLabNone = 0xffff;

template <typename T, int LT, int CP>
__global__ __launch_bounds__(kT) void ohem_upw_fwd_k(
    const T* __restrict__ z, const void* __restrict__ labels, int64_t B, UpFwdGeom g,
    int64_t ignore_label, float thresh, int64_t tb, int shift0, int bins0,
    const float* __restrict__ weight, float* __restrict__ nll_out, float* __restrict__ lse_out,
    uint32_t* __restrict__ hist0, BlkPart* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lh[];       // [hist_words] histogram
  const int C = g.C, IH = g.IH, IW = g.IW, OH = g.OH, OW = g.OW, WR = g.WR, WC = g.WC;
  const int npix = WR * WC;
  float* Zw = reinterpret_cast<float*>(lh + g.hist_words);            // [npix][CP] window of one class chunk of z * log2(e)
  int* yro = reinterpret_cast<int*>(Zw + (size_t)npix * CP);          // [kFwdBand] window pixel offset of the row's y0
  float* yly = reinterpret_cast<float*>(yro + kFwdBand);              // [kFwdBand] lambda_y of the row
  float* wtab = yly + kFwdBand;                                       // [kWideMaxC] class weights (1 without a weight vector)
  uint16_t* lab_s = reinterpret_cast<uint16_t*>(wtab + kWideMaxC);    // [kFwdBand][kT] labels (kLabNone = takes no part)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < bins0; i += kT) lh[i] = 0;
  for (int i = tid; i < kWideMaxC; i += kT) wtab[i] = (weight && i < C) ? weight[i] : 1.f;
  PassAcc acc;
  const int64_t total = B * g.bands * (int64_t)g.xblocks;
  const int64_t plane = (int64_t)IH * IW;
  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int xb = (int)(tile % g.xblocks);
    const int band = (int)((tile / g.xblocks) % g.bands);
    const int64_t b = tile / ((int64_t)g.xblocks * g.bands);
    const int oy_beg = band * kFwdBand;
    const int oy_end = oy_beg + kFwdBand < OH ? oy_beg + kFwdBand : OH;
    const int ox = xb * kT + tid;
    const bool live = ox < OW;
    int ys_lo, xs_lo, t1; float tf;
    src_index0(g.sy, oy_beg, IH, ys_lo, t1, tf);
    src_index0(g.sx, xb * kT, IW, xs_lo, t1, tf);
    const T* zb = z + b * C * plane;
    __syncthreads();                                   // the previous tile's readers are done (also orders lh / wtab init)
    if (tid < kFwdBand) {
      int y0, y1; float ly;
      const int oy = oy_beg + tid < OH ? oy_beg + tid : OH - 1;
      src_index0(g.sy, oy, IH, y0, y1, ly);
      yro[tid] = (y0 - ys_lo) * WC;
      yly[tid] = ly;
    }
#pragma unroll 1
    for (int u0 = 0; u0 < kFwdBand; u0 += 16) {
      int64_t lab[16];
      const int oxc = ox < OW ? ox : OW - 1;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int oy = oy_beg + u0 + u;
        const int oyc = oy < OH ? oy : OH - 1;
        const int64_t v = Lab<LT>::get(labels, (b * OH + oyc) * (int64_t)OW + oxc);     // unconditional, clamped
        lab[u] = (live && oy < oy_end) ? v : ignore_label;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const bool is_cls = label_is_class(lab[u], ignore_label, C);
        if (!is_cls && lab[u] != ignore_label) acc.cnt_bad++;
        lab_s[(u0 + u) * kT + tid] = is_cls ? (uint16_t)lab[u] : (uint16_t)kLabNone;
      }
    }
    int x0, x1; float lx;
    src_index0(g.sx, live ? ox : OW - 1, IW, x0, x1, lx);
    const int xl0 = x0 - xs_lo;                        // x1 = x0 + 1 except on the last source column, where lx = 0 and the
    //                                                    window's clamped copy of that column sits at xl0 + 1
    const up_f2 lx2 = {lx, lx};
    const int nrows = oy_end - oy_beg;
    float m[kFwdBand], s[kFwdBand], xt[kFwdBand];      // per row: running maximum, sum of exp2(logit - m), target logit
#pragma unroll
    for (int r = 0; r < kFwdBand; ++r) { m[r] = kNegBig; s[r] = 0.f; xt[r] = 0.f; }
#pragma unroll 1
    for (int c0 = 0; c0 < C; c0 += CP) {
      if (c0) __syncthreads();                         // the previous chunk's readers are done
      // window of classes [c0, c0 + CP): wave wv takes the (class, row) pairs wv, wv + 4, ...; lanes = source columns;
      // eight pairs' loads in flight per wave, unconditional from clamped addresses (see ohem_up_fwd2_k)
      for (int x0s = 0; x0s < WC; x0s += 64) {
        const int xx = x0s + lane;
        const int xg = xs_lo + xx < IW ? xs_lo + xx : IW - 1;
        const bool xin = xx < WC;
        int c = 0, rr = wv;
        while (rr >= WR) { rr -= WR; ++c; }
        while (c < CP) {
          float val[8];
          int off[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const bool on = c < CP;
            const int yy = ys_lo + rr < IH ? ys_lo + rr : IH - 1;
            const int cg = c0 + c;
            const int cc = cg < C ? cg : C - 1;
            const float raw = ld1<T>(zb + (int64_t)cc * plane + (int64_t)yy * IW + xg) * kLog2e;
            val[u] = cg < C ? raw : kNegBig;
            off[u] = (on && xin) ? (rr * WC + xx) * CP + c : -1;
            rr += kT / 64;
            while (rr >= WR) { rr -= WR; ++c; }
          }
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (off[u] >= 0) Zw[off[u]] = val[u];
        }
      }
      __syncthreads();
      if (live) {
        up_f2 H0[CP / 2], D[CP / 2];
        int cro = -1, p00 = 0;
#pragma unroll
        for (int r = 0; r < kFwdBand; ++r) {
          if (r < nrows) {
            const int ro = __builtin_amdgcn_readfirstlane(yro[r]);
            const float ly = yly[r];
            if (ro != cro) {
              p00 = (ro + xl0) * CP;
              const float4* A0 = reinterpret_cast<const float4*>(Zw + p00);
              const float4* A1 = reinterpret_cast<const float4*>(Zw + p00 + CP);
              const float4* B0 = reinterpret_cast<const float4*>(Zw + p00 + WC * CP);
              const float4* B1 = reinterpret_cast<const float4*>(Zw + p00 + WC * CP + CP);
#pragma unroll
              for (int q = 0; q < CP / 4; ++q) {
                const float4 a0 = A0[q], a1 = A1[q], b0 = B0[q], b1 = B1[q];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                  const up_f2 a0p = k ? up_f2{a0.z, a0.w} : up_f2{a0.x, a0.y};
                  const up_f2 a1p = k ? up_f2{a1.z, a1.w} : up_f2{a1.x, a1.y};
                  const up_f2 b0p = k ? up_f2{b0.z, b0.w} : up_f2{b0.x, b0.y};
                  const up_f2 b1p = k ? up_f2{b1.z, b1.w} : up_f2{b1.x, b1.y};
                  const up_f2 h0 = __builtin_elementwise_fma(lx2, a1p - a0p, a0p);
                  const up_f2 h1 = __builtin_elementwise_fma(lx2, b1p - b0p, b0p);
                  H0[q * 2 + k] = h0;
                  D[q * 2 + k] = h1 - h0;
                }
              }
              cro = ro;
            }
            up_f2 v[CP / 2];
            const up_f2 ly2 = {ly, ly};
            float mc = kNegBig;
#pragma unroll
            for (int c = 0; c < CP / 2; ++c) {
              v[c] = __builtin_elementwise_fma(ly2, D[c], H0[c]);
              mc = fmaxf(mc, fmaxf(v[c].x, v[c].y));
            }
            const float mn = fmaxf(m[r], mc);
            const up_f2 mn2 = {mn, mn};
            up_f2 s2 = {0.f, 0.f};
#pragma unroll
            for (int c = 0; c < CP / 2; ++c) {
              const up_f2 d = v[c] - mn2;
              s2 += up_f2{__builtin_amdgcn_exp2f(d.x), __builtin_amdgcn_exp2f(d.y)};
            }
            s[r] = __builtin_fmaf(s[r], __builtin_amdgcn_exp2f(m[r] - mn), s2.x + s2.y);
            m[r] = mn;
            // the target logit, by the expressions that produced v[t - c0], when this chunk holds the target class
            const int tl = (int)lab_s[r * kT + tid] - c0;
            const bool mine = (unsigned)tl < (unsigned)CP;
            const int tt = mine ? tl : 0;
            const float a0 = Zw[p00 + tt], a1 = Zw[p00 + CP + tt], b0 = Zw[p00 + WC * CP + tt], b1 = Zw[p00 + WC * CP + CP + tt];
            const float h0 = __builtin_fmaf(lx, a1 - a0, a0), h1 = __builtin_fmaf(lx, b1 - b0, b0);
            const float xv = __builtin_fmaf(ly, h1 - h0, h0);
            xt[r] = mine ? xv : xt[r];
          }
        }
      }
    }
    if (live) {
      float* nll_p = nll_out + (b * OH + oy_beg) * (int64_t)OW + ox;
      float* lse_p = lse_out + (b * OH + oy_beg) * (int64_t)OW + ox;
#pragma unroll
      for (int r = 0; r < kFwdBand; ++r) {
        if (r < nrows) {
          const float l2 = m[r] + __builtin_amdgcn_logf(s[r]);
          const int lab = lab_s[r * kT + tid];
          const bool valid = lab != kLabNone;
          const int t = valid ? lab : 0;
          float nl = (l2 - xt[r]) * kLn2;
          nl = nl < 0.f ? 0.f : nl;
          nl = valid ? nl : 0.f;
          nll_p[(int64_t)r * OW] = nl;
          lse_p[(int64_t)r * OW] = l2 * kLn2;
          account(acc, valid, nl, wtab[t], thresh, tb, shift0, bins0, lh);
        }
      }
    }
  }
  fold_block(acc, lh, bins0, hist0, part);
}

static int up_class_pad(int C) { return C <= 8 ? 8 : C <= 16 ? 16 : C <= 20 ? 20 : C <= 24 ? 24 : 32; }
// 4 register arrays of CP floats per thread.  TSG_HEAD_BWD_NT=512|1024: threads (= output columns) per backward block
static int up_bwd_ntmax(int CP) {
  static const int forced = tsg_env_int("TSG_HEAD_BWD_NT", 0);
  const int lim = CP <= 20 ? 1024 : 512;
  return (forced == 512 || forced == 256) ? (forced < lim ? forced : lim) : lim;
}

static UpFwdGeom up_fwd_geom(int C, int IH, int IW, int OH, int OW, int bins0) {
  UpFwdGeom g;
  g.C = C; g.IH = IH; g.IW = IW; g.OH = OH; g.OW = OW;
  g.sy = ac_scale(IH, OH); g.sx = ac_scale(IW, OW);
  g.WR = (int)floorf(g.sy * (float)(kFwdBand - 1)) + 3;
  g.WC = (int)floorf(g.sx * (float)(kT - 1)) + 3;
  g.xblocks = (OW + kT - 1) / kT;
  g.bands = (OH + kFwdBand - 1) / kFwdBand;
  g.hist_words = ((bins0 > 0 ? bins0 : 1) + 3) / 4 * 4;
  return g;
}
static size_t up_fwd_lds(const UpFwdGeom& g, int CP) {
  return (size_t)g.hist_words * 4 + (size_t)CP * g.WR * g.WC * 4 + (size_t)((g.WR * g.WC + 3) & ~3) * 4 +
         (size_t)kFwdBand * 8 + 32 * 4 + (size_t)kFwdBand * kT;
}
// TSG_HEAD_FWD=2|1 (default 2): the forward form (ohem_up_fwd2_k / the round-3 ohem_up_fwd_k)
static int up_fwd_form() {
  static const int v = tsg_env_int("TSG_HEAD_FWD", 2);
  return v == 1 ? 1 : 2;
}

// backward tiling: the fewest column tiles whose output-column footprint fits one block
struct UpBwdCfg { UpBwdGeom g; int k, NT; size_t lds; bool ok; };
static UpBwdCfg up_bwd_cfg(int64_t B, int C, int IH, int IW, int OH, int OW) {
  UpBwdCfg cf;
  cf.ok = false;
  const int CP = up_class_pad(C), ntmax = up_bwd_ntmax(CP);
  UpBwdGeom& g = cf.g;
  g.C = C; g.IH = IH; g.IW = IW; g.OH = OH; g.OW = OW;
  g.sy = ac_scale(IH, OH); g.sx = ac_scale(IW, OW);
  for (int k = 1; k <= IW; ++k) {
    const int SB = (IW + k - 1) / k;
    int need = 0;
    for (int s0 = 0; s0 < IW; s0 += SB) {
      const int s1 = s0 + SB < IW ? s0 + SB : IW;
      int lo, hi, t;
      footprint(g.sx, s0, OW, lo, t);
      footprint(g.sx, s1 - 1, OW, t, hi);
      if (hi - lo + 1 > need) need = hi - lo + 1;
    }
    if (need > ntmax) continue;
    const int NT = (need + 63) / 64 * 64;
    const int XS = SB + 5;
    const size_t lds = ((size_t)CP * CP + 2 * (size_t)CP * XS + NT + (size_t)NT * (CP + 1) + XS + 2 + CP + 4) * 4;
    if (lds > 150 * 1024) continue;
    g.SB = SB; g.XS = XS;
    cf.k = (IW + SB - 1) / SB; cf.NT = NT; cf.lds = lds; cf.ok = true;
    break;
  }
  if (!cf.ok) return cf;
  g.RB = 8;
  while (g.RB > 2 && (int64_t)cf.k * ((IH + g.RB - 1) / g.RB) * B < 256) g.RB /= 2;   // one block per CU at least
  return cf;
}

// only genuine up-sampling is fused: at least 2x both ways, scales in (0, 0.5]
static bool up_geom_ok(int IH, int IW, int OH, int OW) {
  if (IH < 1 || IW < 1 || OH < 2 * IH || OW < 2 * IW) return false;
  const float sx = ac_scale(IW, OW), sy = ac_scale(IH, OH);
  return !(sx <= 0.f || sy <= 0.f || sx > 0.5f || sy > 0.5f);
}

static bool up_fused_ok(int C, int IH, int IW, int OH, int OW) {
  if (C > 32 || C < 1 || !up_geom_ok(IH, IW, OH, OW)) return false;
  // the forward's LDS window (z under a 256 x 32 output tile) must leave room for several blocks per CU
  if (up_fwd_lds(up_fwd_geom(C, IH, IW, OH, OW, 2048), up_class_pad(C)) > 64 * 1024) return false;
  return up_bwd_cfg(1, C, IH, IW, OH, OW).ok;
}

// ---- wide (33..256 classes) -----------------------------------------------------
constexpr int kWideBwdCP = 32;
static size_t upw_fwd_lds(const UpFwdGeom& g, int CP) {
  return (size_t)g.hist_words * 4 + (size_t)CP * g.WR * g.WC * 4 + (size_t)kFwdBand * 8 + (size_t)kWideMaxC * 4 +
         (size_t)kFwdBand * kT * 2;
}
// the forward's class chunk: the largest whose window leaves room for two blocks per CU (0: none does)
static int upw_fwd_cp(int C, int IH, int IW, int OH, int OW) {
  const UpFwdGeom g = up_fwd_geom(C, IH, IW, OH, OW, 2048);
  if (upw_fwd_lds(g, 32) <= 64 * 1024) return 32;
  if (upw_fwd_lds(g, 16) <= 64 * 1024) return 16;
  return 0;
}
// the WIDE backward's LDS: up_bwd_cfg's figure + the zero one-hot row + a weight table of kWideMaxC instead of CP entries
static size_t upw_bwd_lds(const UpBwdCfg& cf) { return cf.lds + (size_t)kWideMaxC * 4; }

static bool up_wide_ok(int C, int IH, int IW, int OH, int OW) {
  if (C <= 32 || C > kWideMaxC || !up_geom_ok(IH, IW, OH, OW)) return false;
  if (upw_fwd_cp(C, IH, IW, OH, OW) == 0) return false;
  return up_bwd_cfg(1, C, IH, IW, OH, OW).ok;
}

static int pixel_grid(int64_t nvec) {
  int64_t g = (nvec + kT - 1) / kT;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

static int64_t thresh_tb(float thresh) {
  if (thresh < 0.f) return -1;
  union { float f; uint32_t u; } cv;
  cv.f = thresh;
  return (int64_t)cv.u;
}

}  // namespace tsg

using namespace tsg;

static int ohem_select_tail(const tsg_ohem_plan& pl, OhemWs& w, const void* labels, int ltype,
                            int64_t ignore_label, float thresh, int64_t min_kept, const float* weight,
                            float* nll, float* loss, int32_t* sel, int64_t tb, hipStream_t st) {
  const int bins0 = pl.levels > 0 ? pl.bins[0] : 0;
  hipLaunchKernelGGL(ohem_decide0, dim3(1), dim3(kT), 0, st, w.part, pl.grid, w.hist[0], bins0,
                     pl.shift[0], pl.levels, pl.P, min_kept, thresh, tb, weight ? 1 : 0, w.st);
  TSG_CHECK_LAUNCH();
  for (int l = 1; l < pl.levels; ++l) {
    hipLaunchKernelGGL((sel_refine<1>), dim3(pl.grid), dim3(kT), (size_t)pl.bins[l] * 4, st, nll, pl.P,
                       thresh, tb, pl.shift[l - 1], pl.shift[l], pl.bins[l], w.hist[l], w.st);
    TSG_CHECK_LAUNCH();
    hipLaunchKernelGGL(sel_decide, dim3(1), dim3(64), 0, st, w.hist[l], pl.bins[l], pl.shift[l],
                       l == pl.levels - 1 ? 1 : 0, tb, w.st);
    TSG_CHECK_LAUNCH();
  }
  if (ltype == TSG_I64)
    hipLaunchKernelGGL((ohem_pass_c<TSG_I64>), dim3(pl.grid), dim3(kT), 0, st, nll, labels, pl.P, pl.C,
                       ignore_label, weight, w.st, w.csum, w.cwsum, w.ccnt);
  else
    hipLaunchKernelGGL((ohem_pass_c<TSG_U8>), dim3(pl.grid), dim3(kT), 0, st, nll, labels, pl.P, pl.C,
                       ignore_label, weight, w.st, w.csum, w.cwsum, w.ccnt);
  TSG_CHECK_LAUNCH();
  hipLaunchKernelGGL(ohem_finish, dim3(1), dim3(kT), 0, st, w.csum, w.cwsum, w.ccnt, pl.grid,
                     weight ? 1 : 0, w.st, loss, sel);
  TSG_CHECK_LAUNCH();
  return 0;
}

// mask_prob of loss_opr.py:81-83 as the selection kernels see it: the target-class probability recomputed from
// nll with the SAME device expression (prob_of_nll), 1 for pixels that take no part.
template <int LT>
__global__ __launch_bounds__(kT) void target_prob_k(const float* __restrict__ nll, const void* __restrict__ labels,
                                                    int64_t P, int C, int64_t ignore_label, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < P; i += (int64_t)gridDim.x * kT)
    out[i] = label_is_class(Lab<LT>::get(labels, i), ignore_label, C) ? prob_of_nll(nll[i]) : 1.f;
}

template <typename T, int LT, int CP, int NTMAX, bool WIDE>
static int launch_up_bwd(const UpBwdCfg& cf, int64_t B, const void* z, const void* labels, int64_t ignore_label,
                         const float* weight, const float* nll, const float* lse, const int32_t* sel,
                         const float* gscale, void* dz, hipStream_t st) {
  static size_t granted = 0;                            // dynamic LDS above 64 KB has to be requested once
  const int nchunk = WIDE ? (cf.g.C + CP - 1) / CP : 1;
  if (WIDE && B * nchunk > 65535) return TSG_E_SHAPE;
  const size_t lds = WIDE ? upw_bwd_lds(cf) : cf.lds;
  if (lds > 64 * 1024 && lds > granted) {
    TSG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ohem_up_bwd_k<T, LT, CP, NTMAX, WIDE>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    granted = lds;
  }
  dim3 grid((unsigned)cf.k, (unsigned)((cf.g.IH + cf.g.RB - 1) / cf.g.RB), (unsigned)(B * nchunk));
  hipLaunchKernelGGL((ohem_up_bwd_k<T, LT, CP, NTMAX, WIDE>), grid, dim3(cf.NT), lds, st, (const T*)z, labels, cf.g, nchunk,
                     ignore_label, weight, nll, lse, sel, gscale, (T*)dz);
  TSG_CHECK_LAUNCH();
  return 0;
}

extern "C" {

int tsg_ohem_make_plan(int64_t B, int C, int64_t HW, float thresh, tsg_ohem_plan* plan) {
  if (!plan) return TSG_E_NULL;
  if (B <= 0 || C <= 0 || HW <= 0) return TSG_E_SHAPE;
  if (!(thresh == thresh)) return TSG_E_SHAPE;
  plan->P = B * HW;
  plan->C = C;
  plan->grid = pixel_grid(plan->P / 4);
  const int64_t tb = thresh_tb(thresh);
  const int64_t range = (int64_t)0x3f800000 - tb;  // number of distinct p in (thresh, 1]
  level_plan(range, &plan->levels, plan->shift, plan->bins);
  plan->thresh_bits = thresh < 0.f ? 0u : (uint32_t)tb;
  OhemWs w = carve(nullptr, *plan);
  plan->ws_bytes = w.total;
  return 0;
}

int tsg_ohem_fwd(const void* logits, int dtype, const void* labels, int ltype, int64_t B, int C,
                 int64_t HW, int64_t ignore_label, float thresh, int64_t min_kept,
                 const float* weight, float* nll, float* lse, float* loss, int32_t* sel,
                 void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !labels || !nll || !lse || !loss || !sel || !ws) return TSG_E_NULL;
  if (dtype != TSG_F32 && dtype != TSG_BF16) return TSG_E_DTYPE;
  if (ltype != TSG_I64 && ltype != TSG_U8) return TSG_E_DTYPE;
  tsg_ohem_plan pl;
  int e = tsg_ohem_make_plan(B, C, HW, thresh, &pl);
  if (e) return e;
  if (ws_bytes < pl.ws_bytes) return TSG_E_WS;
  if (!aligned16(ws)) return TSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  OhemWs w = carve(ws, pl);
  TSG_HIP(hipMemsetAsync(ws, 0, w.zero_bytes, st));
  const int64_t tb = thresh_tb(thresh);
  const int native = native_vec(dtype);
  const bool vec = (HW % native == 0) && aligned16(logits) && aligned16(nll) && aligned16(lse);
  const int bins0 = pl.levels > 0 ? pl.bins[0] : 0;
  static const size_t pa_throttle = (size_t)tsg_env_int("TSG_OHEM_FWD_LDS", 0);
  size_t sh = (size_t)(bins0 > 0 ? bins0 : 1) * sizeof(uint32_t);
  if (sh < pa_throttle) sh = pa_throttle;
  return with_elem_vec(dtype, vec, [&](auto t, auto v) { return with_label(ltype, [&](auto lt) {
    typedef typename decltype(t)::type T;
    hipLaunchKernelGGL((ohem_pass_a<T, v(), lt()>), dim3(pl.grid), dim3(kT), sh, st, (const T*)logits, labels, pl.P, C, HW,
                       ignore_label, thresh, tb, pl.shift[0], bins0, weight, nll, lse, w.hist[0], w.part);
    TSG_CHECK_LAUNCH();
    return ohem_select_tail(pl, w, labels, ltype, ignore_label, thresh, min_kept, weight, nll, loss, sel, tb, st);
  }); });
}

int tsg_ohem_bwd(const void* logits, int dtype, const void* labels, int ltype, int64_t B, int C,
                 int64_t HW, int64_t ignore_label, const float* weight, const float* nll,
                 const float* lse, const int32_t* sel, const float* gscale, void* dlogits,
                 void* ws, void* stream) {
  (void)ws;
  if (!logits || !labels || !nll || !lse || !sel || !gscale || !dlogits) return TSG_E_NULL;
  if (dtype != TSG_F32 && dtype != TSG_BF16) return TSG_E_DTYPE;
  if (ltype != TSG_I64 && ltype != TSG_U8) return TSG_E_DTYPE;
  if (B <= 0 || C <= 0 || HW <= 0) return TSG_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t P = B * HW;
  const int native = native_vec(dtype);
  const bool vec = (HW % native == 0) && aligned16(logits) && aligned16(dlogits);
  const int V = vec ? native : 1;
  const int grid = pixel_grid(P / V);
  // occupancy throttle (tuning knob): unused dynamic LDS caps the resident waves per CU
  // (measured on MI355X, 16x19x1024^2 bf16: 0 B -> 407 us, 40 KB (4 blocks/CU) -> 354 us, 64 KB -> 476 us: with 38
  //  concurrent 2-MB-strided class planes per block, fewer resident blocks thrash DRAM pages / L2 less)
  static const size_t throttle = (size_t)tsg_env_int("TSG_OHEM_BWD_LDS", 40000);
  return with_elem_vec(dtype, vec, [&](auto t, auto v) { return with_label(ltype, [&](auto lt) {
    typedef typename decltype(t)::type T;
    hipLaunchKernelGGL((ohem_bwd_k<T, v(), lt()>), dim3(grid), dim3(kT), throttle, st, (const T*)logits, labels, P, C, HW,
                       ignore_label, weight, nll, lse, sel, gscale, (T*)dlogits);
    TSG_CHECK_LAUNCH();
    return 0;
  }); });
}

// ---- fused upsample + OHEM ------------------------------------------------------
int tsg_ohem_up_supported(int C, int IH, int IW, int OH, int OW, float thresh) {
  (void)thresh;
  return up_fused_ok(C, IH, IW, OH, OW) ? 1 : 0;
}

int tsg_ohem_up_wide_supported(int C, int IH, int IW, int OH, int OW) {
  return up_wide_ok(C, IH, IW, OH, OW) ? 1 : 0;
}

size_t tsg_ohem_up_bwd_ws_bytes(int64_t B, int C, int IH, int OW) {
  if (B <= 0 || C <= 0 || IH <= 0 || OW <= 0) return 0;
  return 256;                                          // the backward needs no scratch any more; kept for the ABI
}

int tsg_ohem_up_fwd(const void* z, int dtype, const void* labels, int ltype, int64_t B, int C, int IH,
                    int IW, int OH, int OW, int64_t ignore_label, float thresh, int64_t min_kept,
                    const float* weight, float* nll, float* lse, float* loss, int32_t* sel, void* ws,
                    size_t ws_bytes, void* stream) {
  if (!z || !labels || !nll || !lse || !loss || !sel || !ws) return TSG_E_NULL;
  if (dtype != TSG_F32 && dtype != TSG_BF16) return TSG_E_DTYPE;
  if (ltype != TSG_I64 && ltype != TSG_U8) return TSG_E_DTYPE;
  const bool wide = C > 32;
  if (IH <= 0 || IW <= 0 || !(wide ? up_wide_ok(C, IH, IW, OH, OW) : up_fused_ok(C, IH, IW, OH, OW))) return TSG_E_SHAPE;
  tsg_ohem_plan pl;
  int e = tsg_ohem_make_plan(B, C, (int64_t)OH * OW, thresh, &pl);
  if (e) return e;
  if (ws_bytes < pl.ws_bytes) return TSG_E_WS;
  if (!aligned16(ws)) return TSG_E_ALIGN;
  const int bins0 = pl.levels > 0 ? pl.bins[0] : 0;
  hipStream_t st = (hipStream_t)stream;
  OhemWs w = carve(ws, pl);
  TSG_HIP(hipMemsetAsync(ws, 0, w.zero_bytes, st));
  const int64_t tb = thresh_tb(thresh);
  const UpFwdGeom g = up_fwd_geom(C, IH, IW, OH, OW, bins0);
  if (wide) {
    if (B * ((C + kWideBwdCP - 1) / kWideBwdCP) > 65535) return TSG_E_SHAPE;   // the backward's grid.z: refuse here, not after the forward
    const int WCP = upw_fwd_cp(C, IH, IW, OH, OW);
    const size_t wsh = upw_fwd_lds(g, WCP);
    return with_elem(dtype, [&](auto t) { return with_label(ltype, [&](auto lt) { return with_int<32, 16>(WCP, [&](auto cp) {
      typedef typename decltype(t)::type T;
      hipLaunchKernelGGL((ohem_upw_fwd_k<T, lt(), cp()>), dim3(pl.grid), dim3(kT), wsh, st, (const T*)z, labels, B, g,
                         ignore_label, thresh, tb, pl.shift[0], bins0, weight, nll, lse, w.hist[0], w.part);
      TSG_CHECK_LAUNCH();
      return ohem_select_tail(pl, w, labels, ltype, ignore_label, thresh, min_kept, weight, nll, loss, sel, tb, st);
    }); }); });
  }
  const int CP = up_class_pad(C);
  const size_t sh = up_fwd_lds(g, CP);
  const bool form2 = up_fwd_form() == 2;
  return with_elem(dtype, [&](auto t) { return with_label(ltype, [&](auto lt) { return with_int<8, 16, 20, 24, 32>(CP, [&](auto cp) {
    typedef typename decltype(t)::type T;
    if (form2)
      hipLaunchKernelGGL((ohem_up_fwd2_k<T, lt(), cp()>), dim3(pl.grid), dim3(kT), sh, st, (const T*)z, labels, B, g,
                         ignore_label, thresh, tb, pl.shift[0], bins0, weight, nll, lse, w.hist[0], w.part);
    else
      hipLaunchKernelGGL((ohem_up_fwd_k<T, lt(), cp()>), dim3(pl.grid), dim3(kT), sh, st, (const T*)z, labels, B, g,
                         ignore_label, thresh, tb, pl.shift[0], bins0, weight, nll, lse, w.hist[0], w.part);
    TSG_CHECK_LAUNCH();
    return ohem_select_tail(pl, w, labels, ltype, ignore_label, thresh, min_kept, weight, nll, loss, sel, tb, st);
  }); }); });
}

int tsg_ohem_up_bwd(const void* z, int dtype, const void* labels, int ltype, int64_t B, int C, int IH,
                    int IW, int OH, int OW, int64_t ignore_label, const float* weight, const float* nll,
                    const float* lse, const int32_t* sel, const float* gscale, void* dz, void* ws,
                    size_t ws_bytes, void* stream) {
  (void)ws; (void)ws_bytes;
  if (!z || !labels || !nll || !lse || !sel || !gscale || !dz) return TSG_E_NULL;
  if (dtype != TSG_F32 && dtype != TSG_BF16) return TSG_E_DTYPE;
  if (ltype != TSG_I64 && ltype != TSG_U8) return TSG_E_DTYPE;
  const bool wide = C > 32;
  if (B <= 0 || !(wide ? up_wide_ok(C, IH, IW, OH, OW) : up_fused_ok(C, IH, IW, OH, OW))) return TSG_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const UpBwdCfg cf = up_bwd_cfg(wide ? B * ((C + kWideBwdCP - 1) / kWideBwdCP) : B, C, IH, IW, OH, OW);
  if (!cf.ok) return TSG_E_SHAPE;
  return with_elem(dtype, [&](auto t) { return with_label(ltype, [&](auto lt) {
    typedef typename decltype(t)::type T;
    if (wide) return launch_up_bwd<T, lt(), kWideBwdCP, 512, true>(cf, B, z, labels, ignore_label, weight, nll, lse, sel, gscale, dz, st);
    return with_int<8, 16, 20, 24, 32>(up_class_pad(C), [&](auto cp) {         // NTMAX: 1024 threads up to 20 padded classes
      return launch_up_bwd<T, lt(), cp(), (cp() <= 20 ? 1024 : 512), false>(cf, B, z, labels, ignore_label, weight, nll, lse, sel, gscale, dz, st);
    });
  }); });
}

// ---- standalone exact k-th order statistic -----------------------------------
static void kth_plan(tsg_ohem_plan* pl, int64_t n) {
  pl->P = n;
  pl->C = 1;
  pl->grid = pixel_grid(n);
  level_plan((int64_t)1 << 31, &pl->levels, pl->shift, pl->bins);  // all non-negative floats
  OhemWs w = carve(nullptr, *pl);
  pl->ws_bytes = w.total;
}

size_t tsg_kth_ws_bytes(int64_t n) {
  tsg_ohem_plan pl;
  kth_plan(&pl, n);
  return pl.ws_bytes;
}

__global__ void kth_init(SelState* st, int64_t k) {
  st->branch = 1; st->krem = k; st->lo_d = 0;
}
__global__ void kth_out(const SelState* st, float* out) { out[0] = __uint_as_float(st->thr_bits); }

int tsg_ohem_target_prob(const float* nll, const void* labels, int ltype, int64_t P, int C, int64_t ignore_label,
                         float* prob, void* stream) {
  if (!nll || !labels || !prob) return TSG_E_NULL;
  if (P <= 0 || C <= 0) return TSG_E_SHAPE;
  if (ltype != TSG_I64 && ltype != TSG_U8) return TSG_E_DTYPE;
  const int grid = (int)((P + kT - 1) / kT < 4096 ? (P + kT - 1) / kT : 4096);
  if (ltype == TSG_I64)
    hipLaunchKernelGGL((target_prob_k<TSG_I64>), dim3(grid), dim3(kT), 0, (hipStream_t)stream, nll, labels, P, C, ignore_label, prob);
  else
    hipLaunchKernelGGL((target_prob_k<TSG_U8>), dim3(grid), dim3(kT), 0, (hipStream_t)stream, nll, labels, P, C, ignore_label, prob);
  TSG_CHECK_LAUNCH();
  return 0;
}

// level 0 of the standalone select is a refine over the whole range
int tsg_kth_value(const float* v, int64_t n, int64_t k, float* out, void* ws, size_t ws_bytes,
                  void* stream) {
  if (!v || !out || !ws) return TSG_E_NULL;
  if (n <= 0 || k < 1 || k > n) return TSG_E_SHAPE;
  tsg_ohem_plan pl;
  kth_plan(&pl, n);
  if (ws_bytes < pl.ws_bytes) return TSG_E_WS;
  hipStream_t st = (hipStream_t)stream;
  OhemWs w = carve(ws, pl);
  TSG_HIP(hipMemsetAsync(ws, 0, w.zero_bytes, st));
  hipLaunchKernelGGL(kth_init, dim3(1), dim3(1), 0, st, w.st, k);
  const int64_t tb = -1;
  int prev_shift = 31;
  for (int l = 0; l < pl.levels; ++l) {
    hipLaunchKernelGGL((sel_refine<0>), dim3(pl.grid), dim3(kT), (size_t)pl.bins[l] * 4, st, v, n,
                       -1.0f, tb, prev_shift, pl.shift[l], pl.bins[l], w.hist[l], w.st);
    TSG_CHECK_LAUNCH();
    hipLaunchKernelGGL(sel_decide, dim3(1), dim3(64), 0, st, w.hist[l], pl.bins[l], pl.shift[l],
                       l == pl.levels - 1 ? 1 : 0, tb, w.st);
    TSG_CHECK_LAUNCH();
    prev_shift = pl.shift[l];
  }
  hipLaunchKernelGGL(kth_out, dim3(1), dim3(1), 0, st, w.st, out);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
