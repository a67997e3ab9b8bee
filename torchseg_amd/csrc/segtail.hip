// The tail of a segmentation evaluation in one pass, for gfx950.
//
// Restates what an evaluated window costs in the reference after the network's last convolution
// (model/bisenet/*/network.py: `F.log_softmax(F.interpolate(logits, scale_factor=8, mode='bilinear',
// align_corners=True), dim=1)`; furnace/engine/evaluator.py:255-273 adds the flipped pass and takes exp, :226-242 adds
// the window into the score map).  Unfused that is five full-resolution fp32 passes per window; here the low-resolution
// logits are read (they stay L2-resident) and the full-resolution map is written once (logprob) or read-modify-written
// once (accum).
//
// Interpolated logit: exactly the taps, weights and operation order of tsg_upsample_bilinear_ac_fwd (tsg_resample.h),
//   v = (1-ly) * ((1-lx) z[y0][x0] + lx z[y0][x1]) + ly * ((1-lx) z[y1][x0] + lx z[y1][x1]),
// evaluated in fp32 straight from the bf16 / fp32 taps (no intermediate rounding).  log_softmax over the C classes of
// one pixel in two passes over the classes (an online max / sum-of-exp, then v - lse), all in fp32 registers; the
// taps of the second pass are re-read from cache rather than held, so any C is served by the same registers.
//
// A thread owns V adjacent output columns of RB output rows (logprob) or of one destination row (accum).  The
// horizontal tap indices and weights of its columns are computed once and shared by every class and row; the vertical
// ones once per row.  Stores are one 16-byte vector per class plane when the row width allows it (V = 4), else scalar.
// No atomics: every output element is produced by exactly one thread in a fixed order, so results are bit-reproducible.
#include "tsg_dispatch.h"
#include "tsg_resample.h"

namespace tsg {
namespace {

constexpr int kT = 256;
constexpr int kMaxC = 256;
constexpr int kSlots = 2;            // covering windows whose log-sum-exp a thread holds at once (accum)

template <typename T> __device__ __forceinline__ float tapld(const T* p);
template <> __device__ __forceinline__ float tapld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float tapld<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }

template <int V> struct F32Out;
template <> struct F32Out<4> {
  static __device__ __forceinline__ void st(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
  static __device__ __forceinline__ void ld(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
};
template <> struct F32Out<2> {
  static __device__ __forceinline__ void st(float* p, const float (&v)[2]) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  }
  static __device__ __forceinline__ void ld(const float* p, float (&v)[2]) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  }
};
template <> struct F32Out<1> {
  static __device__ __forceinline__ void st(float* p, const float (&v)[1]) { *p = v[0]; }
  static __device__ __forceinline__ void ld(const float* p, float (&v)[1]) { v[0] = *p; }
};

// horizontal taps of V columns; columns past `ncols` are clamped to the last valid one (computed, never stored)
template <int V>
struct ColTaps {
  int x0[V], x1[V];
  float lx[V];
};

// the interpolated logit of V columns of one output row of one class plane
template <typename T, int V>
__device__ __forceinline__ void interp(const T* __restrict__ plane, int w, int y0, int y1, float ly,
                                       const ColTaps<V>& ct, float (&v)[V]) {
  const T* r0 = plane + (int64_t)y0 * w;
  const T* r1 = plane + (int64_t)y1 * w;
  const float hy = 1.f - ly;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float h0 = (1.f - ct.lx[j]) * tapld<T>(r0 + ct.x0[j]) + ct.lx[j] * tapld<T>(r0 + ct.x1[j]);
    const float h1 = (1.f - ct.lx[j]) * tapld<T>(r1 + ct.x0[j]) + ct.lx[j] * tapld<T>(r1 + ct.x1[j]);
    v[j] = hy * h0 + ly * h1;
  }
}

// online log-sum-exp over the C class planes of V pixels: returns lse = m + log(sum exp(v - m))
template <typename T, int V>
__device__ __forceinline__ void logsumexp(const T* __restrict__ img, int64_t plane, int C, int w, int y0, int y1,
                                          float ly, const ColTaps<V>& ct, float (&lse)[V]) {
  float m[V], s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { m[j] = -INFINITY; s[j] = 0.f; }
  for (int c = 0; c < C; ++c) {
    float v[V];
    interp<T, V>(img + c * plane, w, y0, y1, ly, ct, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (v[j] > m[j]) {
        s[j] = s[j] * expf(m[j] - v[j]) + 1.f;
        m[j] = v[j];
      } else {
        s[j] += expf(v[j] - m[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) lse[j] = m[j] + logf(s[j]);
}

// ---- log_softmax(interp(z), 1) -> out [N, C, H, W] fp32 -------------------------------------------------------------
// thread = V columns x RB rows of one image; a wave spans 64 column groups of the same rows
template <typename T, int V, int RB>
__global__ __launch_bounds__(kT) void seg_logprob(const T* __restrict__ z, float* __restrict__ out, int N, int C, int h,
                                                  int w, int H, int W, float sy, float sx) {
  const int vpr = (W + V - 1) / V;
  const int bands = (H + RB - 1) / RB;
  const int64_t total = (int64_t)N * bands * vpr;
  const int64_t plane = (int64_t)h * w, oplane = (int64_t)H * W;
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
    const int vx = (int)(i % vpr);
    const int64_t t = i / vpr;
    const int band = (int)(t % bands);
    const int n = (int)(t / bands);
    ColTaps<V> ct;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int ox = vx * V + j < W ? vx * V + j : W - 1;
      src_index(sx, ox, w, ct.x0[j], ct.x1[j], ct.lx[j]);
    }
    const T* img = z + (int64_t)n * C * plane;
    float* o = out + (int64_t)n * C * oplane;
    const int oy_end = (band + 1) * RB < H ? (band + 1) * RB : H;
    for (int oy = band * RB; oy < oy_end; ++oy) {
      int y0, y1; float ly;
      src_index(sy, oy, h, y0, y1, ly);
      float lse[V];
      logsumexp<T, V>(img, plane, C, w, y0, y1, ly, ct, lse);
      const int64_t orow = (int64_t)oy * W + (int64_t)vx * V;
      for (int c = 0; c < C; ++c) {
        float v[V];
        interp<T, V>(img + c * plane, w, y0, y1, ly, ct, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = v[j] - lse[j];
        if (V == 1 || vx * V + V <= W) {
          F32Out<V>::st(o + c * oplane + orow, v);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (vx * V + j < W) o[c * oplane + orow + j] = v[j];
        }
      }
    }
  }
}

// ---- dst[:, oy+r, ox+c] (+)= exp(lp[:, t+r, l+c] + lp_flip[:, t+r, W-1-(l+c)]) over the windows of a batch -------------
// geom [N][6] = (oy, ox, t, l, rows, cols).  Thread = V adjacent columns of one row of the region [by0, by1) x [bx0, bx1)
// of dst; it visits the windows in batch order and adds every covering window's term to ONE read of dst, in that order
// (the reference's `data[...] += score` loop, window by window).  Windows are taken kSlots at a time: the log-sum-exps of
// a group are held in registers, and a pixel covered by more than kSlots windows of one batch reads dst again between
// groups -- the same summation order.  accumulate = 0: a pixel's first covering window writes (dst is not read until
// then); pixels no window covers are left as they are.
template <typename T, int V, bool FLIP>
__global__ __launch_bounds__(kT) void seg_accum(const T* __restrict__ z, const T* __restrict__ zf,
                                                const int32_t* __restrict__ geom, float* __restrict__ dst, int N, int C,
                                                int h, int w, int H, int W, int Hd, int Wd, int by0, int bx0, int bh,
                                                int bw, int accumulate, float sy, float sx) {
  const int vpr = (bw + V - 1) / V;
  const int64_t total = (int64_t)bh * vpr;
  const int64_t plane = (int64_t)h * w, dplane = (int64_t)Hd * Wd;
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
    const int dy = by0 + (int)(i / vpr);
    const int dx0 = bx0 + (int)(i % vpr) * V;
    int ncols = bx0 + bw - dx0;                    // columns of this thread inside the region (and so inside dst)
    ncols = ncols < V ? ncols : V;
    float* drow = dst + (int64_t)dy * Wd + dx0;
    const unsigned full = (1u << ncols) - 1u;
    unsigned written = accumulate ? full : 0u;     // columns whose dst value is live (read, then added to)
    int k = 0;
    while (k < N) {
      // the next (up to) kSlots covering windows, in batch order
      int win[kSlots];
      unsigned cov[kSlots];
      int ns = 0;
      for (; k < N && ns < kSlots; ++k) {
        const int32_t* g = geom + 6 * k;
        const int oy = g[0], ox = g[1], tt = g[2], ll = g[3], rows = g[4], cols = g[5];
        const int r = dy - oy;
        unsigned msk = 0;
        if (r >= 0 && r < rows && tt + r >= 0 && tt + r < H) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const int cc = dx0 + j - ox;
            if (j < ncols && cc >= 0 && cc < cols && ll + cc >= 0 && ll + cc < W) msk |= 1u << j;
          }
        }
        if (!__any(msk != 0u)) continue;          // wave-uniform window list: window bases stay scalar
        win[ns] = k;
        cov[ns] = msk;
        ++ns;
      }
      if (ns == 0) break;
      // per slot: row taps, column taps (clamped where a column is not covered), log-sum-exp
      ColTaps<V> ct[kSlots], cf[kSlots];
      int y0[kSlots], y1[kSlots];
      float ly[kSlots], lse[kSlots][V], lsef[kSlots][V];
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        if (s >= ns) break;
        const int32_t* g = geom + 6 * win[s];
        int wy = g[2] + (dy - g[0]);
        wy = wy < 0 ? 0 : (wy > H - 1 ? H - 1 : wy);     // lanes the window does not cover: computed, never stored
        src_index(sy, wy, h, y0[s], y1[s], ly[s]);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          int wx = g[3] + (dx0 + j - g[1]);
          wx = wx < 0 ? 0 : (wx > W - 1 ? W - 1 : wx);
          src_index(sx, wx, w, ct[s].x0[j], ct[s].x1[j], ct[s].lx[j]);
          if (FLIP) src_index(sx, W - 1 - wx, w, cf[s].x0[j], cf[s].x1[j], cf[s].lx[j]);
        }
        const int64_t nb = (int64_t)win[s] * C * plane;
        logsumexp<T, V>(z + nb, plane, C, w, y0[s], y1[s], ly[s], ct[s], lse[s]);
        if (FLIP) logsumexp<T, V>(zf + nb, plane, C, w, y0[s], y1[s], ly[s], cf[s], lsef[s]);
      }
      unsigned after = written;
      for (int s = 0; s < ns; ++s) after |= cov[s];
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        float* p = drow + c * dplane;
        float acc[V];
        if (V > 1 && written == (1u << V) - 1u) {
          F32Out<V>::ld(p, acc);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] = (written >> j & 1u) ? p[j] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
          if (s >= ns) break;
          const int64_t off = ((int64_t)win[s] * C + c) * plane;
          float v[V];
          interp<T, V>(z + off, w, y0[s], y1[s], ly[s], ct[s], v);
          float e[V];
#pragma unroll
          for (int j = 0; j < V; ++j) e[j] = v[j] - lse[s][j];
          if (FLIP) {
            float vf[V];
            interp<T, V>(zf + off, w, y0[s], y1[s], ly[s], cf[s], vf);
#pragma unroll
            for (int j = 0; j < V; ++j) e[j] = e[j] + (vf[j] - lsef[s][j]);
          }
          // a pixel not yet written starts from 0: 0 + x == x, the value a plain write of x stores
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (cov[s] >> j & 1u) acc[j] = acc[j] + expf(e[j]);
        }
        if (V > 1 && after == (1u << V) - 1u) {
          F32Out<V>::st(p, acc);
        } else {
          // only live columns are stored: a pixel no window of the batch covers keeps its value
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (after >> j & 1u) p[j] = acc[j];
        }
      }
      written = after;
    }
  }
}

int grid_for(int64_t total) {
  int64_t b = (total + kT - 1) / kT;
  const int64_t cap = 256LL * 64;                 // 64 blocks per CU is far past saturation; grid-stride beyond
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

bool shape_ok(int dtype, int C, int h, int w, int H, int W) {
  return (dtype == TSG_F32 || dtype == TSG_BF16) && C >= 1 && C <= kMaxC && h >= 1 && w >= 1 && H >= 1 && W >= 1;
}

}  // namespace
}  // namespace tsg

using namespace tsg;

extern "C" int tsg_seg_tail_logprob_supported(int dtype, int C, int h, int w, int H, int W) {
  return shape_ok(dtype, C, h, w, H, W) ? 1 : 0;
}

extern "C" int tsg_seg_tail_logprob(const void* z, int dtype, int64_t N, int C, int h, int w, int H, int W, float* out,
                                    void* stream) {
  if (!z || !out) return TSG_E_NULL;
  if (!shape_ok(dtype, C, h, w, H, W) || N < 1 || N > (1 << 20)) return TSG_E_SHAPE;
  if (((uintptr_t)out & 15) != 0) return TSG_E_ALIGN;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  hipStream_t s = (hipStream_t)stream;
  constexpr int RB = 4;
  const int64_t bands = (H + RB - 1) / RB;
  return with_elem(dtype, [&](auto t) { return with_flag(W % 4 == 0, [&](auto v4) {     // 4 columns per thread, or 1
    typedef typename decltype(t)::type T;
    constexpr int V = v4() ? 4 : 1;
    const int64_t total = N * bands * (W / V);
    hipLaunchKernelGGL((seg_logprob<T, V, RB>), dim3(grid_for(total)), dim3(kT), 0, s, (const T*)z, out, (int)N, C, h, w, H, W,
                       sy, sx);
    TSG_CHECK_LAUNCH();
    return 0;
  }); });
}

extern "C" int tsg_seg_tail_accum_supported(int dtype, int C, int h, int w, int H, int W, int Hd, int Wd) {
  return shape_ok(dtype, C, h, w, H, W) && Hd >= 1 && Wd >= 1 ? 1 : 0;
}

template <typename T, int V>
static void launch_accum(const void* z, const void* zf, const int32_t* geom, float* dst, int N, int C, int h, int w,
                         int H, int W, int Hd, int Wd, int by0, int bx0, int bh, int bw, int acc, float sy, float sx,
                         hipStream_t s) {
  // with the flipped term a 4-column thread needs ~250 VGPRs (one wave per SIMD): 2 columns (8-byte access) instead
  constexpr int VF = V > 2 ? 2 : V;
  if (zf)
    hipLaunchKernelGGL((seg_accum<T, VF, true>), dim3(grid_for((int64_t)bh * ((bw + VF - 1) / VF))), dim3(kT), 0, s, (const T*)z, (const T*)zf, geom,
                       dst, N, C, h, w, H, W, Hd, Wd, by0, bx0, bh, bw, acc, sy, sx);
  else
    hipLaunchKernelGGL((seg_accum<T, V, false>), dim3(grid_for((int64_t)bh * ((bw + V - 1) / V))), dim3(kT), 0, s, (const T*)z, (const T*)nullptr,
                       geom, dst, N, C, h, w, H, W, Hd, Wd, by0, bx0, bh, bw, acc, sy, sx);
}

extern "C" int tsg_seg_tail_accum(const void* z, const void* zflip, int dtype, int64_t N, int C, int h, int w, int H,
                                  int W, const int32_t* geom, float* dst, int Hd, int Wd, int by0, int by1, int bx0,
                                  int bx1, int accumulate, void* stream) {
  if (!z || !geom || !dst) return TSG_E_NULL;
  if (!tsg_seg_tail_accum_supported(dtype, C, h, w, H, W, Hd, Wd) || N < 1 || N > 4096) return TSG_E_SHAPE;
  if (by0 < 0 || bx0 < 0 || by1 > Hd || bx1 > Wd || by0 > by1 || bx0 > bx1) return TSG_E_SHAPE;
  if (by0 == by1 || bx0 == bx1) return 0;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  hipStream_t s = (hipStream_t)stream;
  // 16-byte dst access needs every row start and the region's first column on a 4-float boundary
  const bool vec = Wd % 4 == 0 && bx0 % 4 == 0 && ((uintptr_t)dst & 15) == 0;
  const int bh = by1 - by0, bw = bx1 - bx0;
  return with_elem(dtype, [&](auto t) { return with_flag(vec, [&](auto v4) {
    launch_accum<typename decltype(t)::type, v4() ? 4 : 1>(z, zflip, geom, dst, (int)N, C, h, w, H, W, Hd, Wd, by0, bx0, bh, bw,
                                                           accumulate, sy, sx, s);
    TSG_CHECK_LAUNCH();
    return 0;
  }); });
}
