// Depthwise 3x3 convolution (padding 1, dilation 1, stride 1 or 2, no bias): forward, data gradient, weight gradient.
//
// The 51 `nn.Conv2d(C, C, 3, s, 1, groups=C, bias=False)` layers of Xception39 (furnace/base_model/xception.py,
// SeparableConvBnRelu.conv1) on channels_last activations [B,H,W,C], C % 8 == 0.  A lane owns 8 consecutive channels (one
// 16-byte bf16 access, two for fp32) of a run of output pixels along W.  The filter is read as the fp32 parameter
// [C,1,3,3] (element c*9 + kh*3 + kw), so no cast launch is needed.
//
// Two modes, chosen by the activation dtype:
//   bf16: bf16 in / bf16 out, fp32 accumulation, one rounding at the store;
//   fp32: the parity mode, fp32 in / fp32 out, exact products and fp64 accumulation (as csrc/convf32.hip), one rounding.
//
// Every sum runs in a fixed order (taps kh-major, pixels in a shape-determined order), no float atomics anywhere: outputs
// are bit-identical from run to run.  The weight gradient writes per-block partials [P][9][C] (fp32 in bf16 mode, fp64 in
// fp32 mode) and folds them in a second launch; P comes from the shape alone (dw_slices), never from a device query.
#include "tsg_common.h"

namespace tsg {

constexpr int DW_THREADS = 256;

// 8 channels of one pixel as floats
template <typename T> struct DwIo;
template <> struct DwIo<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  template <typename A>
  static __device__ __forceinline__ void store(bf16_t* p, const A* a) {
    uint4 t;
    t.x = pack2_bf16((float)a[0], (float)a[1]);
    t.y = pack2_bf16((float)a[2], (float)a[3]);
    t.z = pack2_bf16((float)a[4], (float)a[5]);
    t.w = pack2_bf16((float)a[6], (float)a[7]);
    *reinterpret_cast<uint4*>(p) = t;
  }
};
template <> struct DwIo<float> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  template <typename A>
  static __device__ __forceinline__ void store(float* p, const A* a) {
    *reinterpret_cast<float4*>(p) = make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4((float)a[4], (float)a[5], (float)a[6], (float)a[7]);
  }
};

// Forward (FLIP = false) and the stride-1 data gradient (FLIP = true: the same convolution with the filter turned 180
// degrees, by indexing).  Lane = (b, oh, run of R output columns, 8 channels), channel groups fastest.  The 3 input rows
// under the run are loaded once each ((R-1)*S + 3 columns) and reused by every tap from registers.
template <typename T, typename A, int S, bool FLIP, int R>
__global__ __launch_bounds__(DW_THREADS) void dw_fwd_k(const T* __restrict__ x, const float* __restrict__ w,
                                                       T* __restrict__ y, int H, int W, int C, int OH, int OW,
                                                       int64_t nlanes) {
  constexpr int NCOL = (R - 1) * S + 3;
  const int64_t i = (int64_t)blockIdx.x * DW_THREADS + threadIdx.x;
  if (i >= nlanes) return;
  const int nvec = C >> 3, nrun = (OW + R - 1) / R;
  const int cv = (int)(i % nvec);
  int64_t t = i / nvec;
  const int run = (int)(t % nrun);
  t /= nrun;
  const int oh = (int)(t % OH);
  const int64_t b = t / OH;
  const int c0 = cv * 8, ow0 = run * R;

  float wt[9][8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k][c] = w[(int64_t)(c0 + c) * 9 + (FLIP ? 8 - k : k)];

  A acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[r][c] = (A)0;

#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = oh * S - 1 + kh;
    if (ih < 0 || ih >= H) continue;
    const T* row = x + ((b * H + ih) * (int64_t)W) * C + c0;
    float xr[NCOL][8];
#pragma unroll
    for (int j = 0; j < NCOL; ++j) {
      const int iw = ow0 * S - 1 + j;
      if (iw >= 0 && iw < W) {
        DwIo<T>::load(row + (int64_t)iw * C, xr[j]);
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) xr[j][c] = 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] += (A)xr[r * S + kw][c] * (A)wt[kh * 3 + kw][c];
  }
  T* out = y + ((b * OH + oh) * (int64_t)OW) * C + c0;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (ow0 + r < OW) DwIo<T>::store(out + (int64_t)(ow0 + r) * C, acc[r]);
}

// Stride-2 data gradient: a gather by output parity.  dx[ih, iw] sums dy[(ih + 1 - kh) / 2, (iw + 1 - kw) / 2] w[kh, kw]
// over the taps whose divisions are exact and in range: 1, 2 or 4 of them.  Lane = (b, ih, iw, 8 channels).
template <typename T, typename A>
__global__ __launch_bounds__(DW_THREADS) void dw_dgrad_s2_k(const T* __restrict__ dy, const float* __restrict__ w,
                                                            T* __restrict__ dx, int H, int W, int C, int OH, int OW,
                                                            int64_t nlanes) {
  const int64_t i = (int64_t)blockIdx.x * DW_THREADS + threadIdx.x;
  if (i >= nlanes) return;
  const int nvec = C >> 3;
  const int cv = (int)(i % nvec);
  int64_t t = i / nvec;
  const int iw = (int)(t % W);
  t /= W;
  const int ih = (int)(t % H);
  const int64_t b = t / H;
  const int c0 = cv * 8;
  A acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = (A)0;
  // kh with (ih + 1 - kh) even: kh = 1 when ih is even, kh = 0 and 2 when ih is odd (same for kw)
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ny = ih + 1 - kh;
    if (ny < 0 || (ny & 1)) continue;
    const int oh = ny >> 1;
    if (oh >= OH) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int nx = iw + 1 - kw;
      if (nx < 0 || (nx & 1)) continue;
      const int ow = nx >> 1;
      if (ow >= OW) continue;
      float g[8];
      DwIo<T>::load(dy + ((b * OH + oh) * (int64_t)OW + ow) * C + c0, g);
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] += (A)g[c] * (A)w[(int64_t)(c0 + c) * 9 + kh * 3 + kw];
    }
  }
  DwIo<T>::store(dx + ((b * H + ih) * (int64_t)W + iw) * C + c0, acc);
}

// Weight-gradient geometry: a block is NV lanes across channel groups x NP = 256 / NV lanes across output pixels; blockIdx.y
// is one of P pixel slices.  Everything here is a function of the shape alone.
struct DwWrw {
  int nvec, nv, np, gx, P;
  int64_t npix, per_slice;
};

static DwWrw dw_wrw_geom(int64_t B, int C, int OH, int OW) {
  DwWrw g;
  g.nvec = C / 8;
  g.nv = 1;
  while (g.nv * 2 <= g.nvec && g.nv < 32) g.nv *= 2;
  g.np = DW_THREADS / g.nv;
  g.gx = (g.nvec + g.nv - 1) / g.nv;
  g.npix = B * OH * OW;
  // about 8 pixels per lane, at most ~1024 blocks in all
  int64_t P = (g.npix + (int64_t)g.np * 8 - 1) / ((int64_t)g.np * 8);
  const int64_t cap = 1024 / g.gx > 0 ? 1024 / g.gx : 1;
  if (P > cap) P = cap;
  if (P < 1) P = 1;
  g.P = (int)P;
  g.per_slice = (g.npix + P - 1) / P;
  return g;
}

// part[slice][tap][c] = sum over the slice's output pixels of dy[p, c] x[tap(p), c]; pixels of a slice are walked
// lane-strided, the NP lanes of a channel group then summed by a fixed tree in LDS.
template <typename T, typename A>
__global__ __launch_bounds__(DW_THREADS) void dw_wgrad_k(const T* __restrict__ x, const T* __restrict__ dy,
                                                         A* __restrict__ part, int H, int W, int C, int OH, int OW, int S,
                                                         DwWrw g) {
  __shared__ A red[DW_THREADS][8];
  const int tid = threadIdx.x;
  const int tc = tid % g.nv, tp = tid / g.nv;
  const int cv = blockIdx.x * g.nv + tc;
  const bool ok = cv < g.nvec;
  const int c0 = cv * 8;
  const int64_t p0 = (int64_t)blockIdx.y * g.per_slice;
  const int64_t p1 = p0 + g.per_slice < g.npix ? p0 + g.per_slice : g.npix;

  A acc[9][8];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[k][c] = (A)0;

  if (ok) {
    for (int64_t p = p0 + tp; p < p1; p += g.np) {
      const int ow = (int)(p % OW);
      const int64_t q = p / OW;
      const int oh = (int)(q % OH);
      const int64_t b = q / OH;
      float gv[8];
      DwIo<T>::load(dy + p * C + c0, gv);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int ih = oh * S - 1 + kh;
        if (ih < 0 || ih >= H) continue;
        const T* row = x + ((b * H + ih) * (int64_t)W) * C + c0;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int iw = ow * S - 1 + kw;
          if (iw < 0 || iw >= W) continue;
          float xv[8];
          DwIo<T>::load(row + (int64_t)iw * C, xv);
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[kh * 3 + kw][c] += (A)gv[c] * (A)xv[c];
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int c = 0; c < 8; ++c) red[tid][c] = acc[k][c];
    __syncthreads();
    for (int s = g.np >> 1; s > 0; s >>= 1) {
      if (tp < s) {
#pragma unroll
        for (int c = 0; c < 8; ++c) red[tid][c] += red[tid + s * g.nv][c];
      }
      __syncthreads();
    }
    if (tp == 0 && ok) {
      A* dst = part + ((int64_t)blockIdx.y * 9 + k) * C + c0;
#pragma unroll
      for (int c = 0; c < 8; ++c) dst[c] = red[tc][c];
    }
    __syncthreads();
  }
}

// dw[c, tap] = sum_{s < P} part[s][tap][c] in fp64, in slice order; one rounding to fp32
template <typename A>
__global__ __launch_bounds__(DW_THREADS) void dw_wgrad_fold_k(const A* __restrict__ part, float* __restrict__ dw, int C,
                                                              int P) {
  const int i = blockIdx.x * DW_THREADS + threadIdx.x;
  if (i >= 9 * C) return;
  const int k = i / C, c = i % C;
  double s = 0.0;
  for (int j = 0; j < P; ++j) s += (double)part[((int64_t)j * 9 + k) * C + c];
  dw[(int64_t)c * 9 + k] = (float)s;
}

}  // namespace tsg

using namespace tsg;

static inline int dw_out(int n, int stride) { return (n - 1) / stride + 1; }

static int dw_check(int dtype, int64_t B, int H, int W, int C, int stride) {
  if (dtype != TSG_F32 && dtype != TSG_BF16) return TSG_E_DTYPE;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || (stride != 1 && stride != 2)) return TSG_E_SHAPE;
  if (B * (int64_t)H * W * C > ((int64_t)1 << 40)) return TSG_E_SHAPE;
  return 0;
}

static inline bool dw_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T, typename A>
static int dw_fwd_launch(const void* x, const float* w, void* y, int64_t B, int H, int W, int C, int stride, bool flip,
                         hipStream_t st) {
  const int OH = dw_out(H, stride), OW = dw_out(W, stride);
  constexpr int R = sizeof(T) == 2 ? 4 : 2;
  const int64_t nlanes = B * OH * (int64_t)((OW + R - 1) / R) * (C / 8);
  const int64_t nb = (nlanes + DW_THREADS - 1) / DW_THREADS;
  if (nb > 0x7fffffff) return TSG_E_SHAPE;
  const T* xp = (const T*)x;
  T* yp = (T*)y;
  if (stride == 2)
    hipLaunchKernelGGL((dw_fwd_k<T, A, 2, false, R>), dim3((unsigned)nb), dim3(DW_THREADS), 0, st, xp, w, yp, H, W, C, OH,
                       OW, nlanes);
  else if (flip)
    hipLaunchKernelGGL((dw_fwd_k<T, A, 1, true, R>), dim3((unsigned)nb), dim3(DW_THREADS), 0, st, xp, w, yp, H, W, C, OH,
                       OW, nlanes);
  else
    hipLaunchKernelGGL((dw_fwd_k<T, A, 1, false, R>), dim3((unsigned)nb), dim3(DW_THREADS), 0, st, xp, w, yp, H, W, C, OH,
                       OW, nlanes);
  TSG_CHECK_LAUNCH();
  return 0;
}

template <typename T, typename A>
static int dw_dgrad_s2_launch(const void* dy, const float* w, void* dx, int64_t B, int H, int W, int C, hipStream_t st) {
  const int OH = dw_out(H, 2), OW = dw_out(W, 2);
  const int64_t nlanes = B * H * (int64_t)W * (C / 8);
  const int64_t nb = (nlanes + DW_THREADS - 1) / DW_THREADS;
  if (nb > 0x7fffffff) return TSG_E_SHAPE;
  hipLaunchKernelGGL((dw_dgrad_s2_k<T, A>), dim3((unsigned)nb), dim3(DW_THREADS), 0, st, (const T*)dy, w, (T*)dx, H, W,
                     C, OH, OW, nlanes);
  TSG_CHECK_LAUNCH();
  return 0;
}

template <typename T, typename A>
static int dw_wgrad_launch(const void* x, const void* dy, float* dw, int64_t B, int H, int W, int C, int stride, void* ws,
                           hipStream_t st) {
  const int OH = dw_out(H, stride), OW = dw_out(W, stride);
  const DwWrw g = dw_wrw_geom(B, C, OH, OW);
  hipLaunchKernelGGL((dw_wgrad_k<T, A>), dim3((unsigned)g.gx, (unsigned)g.P), dim3(DW_THREADS), 0, st, (const T*)x,
                     (const T*)dy, (A*)ws, H, W, C, OH, OW, stride, g);
  TSG_CHECK_LAUNCH();
  hipLaunchKernelGGL((dw_wgrad_fold_k<A>), dim3((unsigned)((9 * C + DW_THREADS - 1) / DW_THREADS)), dim3(DW_THREADS), 0,
                     st, (const A*)ws, dw, C, g.P);
  TSG_CHECK_LAUNCH();
  return 0;
}

extern "C" {

int tsg_dwconv3x3_supported(int dtype, int C, int kh, int kw, int stride, int pad, int dilation, int groups, int H,
                            int W) {
  return (dtype == TSG_F32 || dtype == TSG_BF16) && C > 0 && (C & 7) == 0 && kh == 3 && kw == 3 &&
         (stride == 1 || stride == 2) && pad == 1 && dilation == 1 && groups == C && H > 0 && W > 0;
}

size_t tsg_dwconv3x3_wgrad_ws_bytes(int64_t B, int H, int W, int C, int stride, int dtype) {
  if (dw_check(dtype, B, H, W, C, stride)) return 0;
  const DwWrw g = dw_wrw_geom(B, C, dw_out(H, stride), dw_out(W, stride));
  return (size_t)g.P * 9 * C * (dtype == TSG_F32 ? sizeof(double) : sizeof(float));
}

int tsg_dwconv3x3_fwd(const void* x, const float* w, void* y, int dtype, int64_t B, int H, int W, int C, int stride,
                      void* stream) {
  if (!x || !w || !y) return TSG_E_NULL;
  int e = dw_check(dtype, B, H, W, C, stride);
  if (e) return e;
  if (!dw_aligned(x) || !dw_aligned(y)) return TSG_E_ALIGN;
  return dtype == TSG_BF16 ? dw_fwd_launch<bf16_t, float>(x, w, y, B, H, W, C, stride, false, (hipStream_t)stream)
                           : dw_fwd_launch<float, double>(x, w, y, B, H, W, C, stride, false, (hipStream_t)stream);
}

int tsg_dwconv3x3_dgrad(const void* dy, const float* w, void* dx, int dtype, int64_t B, int H, int W, int C, int stride,
                        void* stream) {
  if (!dy || !w || !dx) return TSG_E_NULL;
  int e = dw_check(dtype, B, H, W, C, stride);
  if (e) return e;
  if (!dw_aligned(dy) || !dw_aligned(dx)) return TSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (stride == 1)
    return dtype == TSG_BF16 ? dw_fwd_launch<bf16_t, float>(dy, w, dx, B, H, W, C, 1, true, st)
                             : dw_fwd_launch<float, double>(dy, w, dx, B, H, W, C, 1, true, st);
  return dtype == TSG_BF16 ? dw_dgrad_s2_launch<bf16_t, float>(dy, w, dx, B, H, W, C, st)
                           : dw_dgrad_s2_launch<float, double>(dy, w, dx, B, H, W, C, st);
}

int tsg_dwconv3x3_wgrad(const void* x, const void* dy, float* dw, int dtype, int64_t B, int H, int W, int C, int stride,
                        void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !dw || !ws) return TSG_E_NULL;
  int e = dw_check(dtype, B, H, W, C, stride);
  if (e) return e;
  if (!dw_aligned(x) || !dw_aligned(dy) || !dw_aligned(ws)) return TSG_E_ALIGN;
  if (ws_bytes < tsg_dwconv3x3_wgrad_ws_bytes(B, H, W, C, stride, dtype)) return TSG_E_WS;
  hipStream_t st = (hipStream_t)stream;
  return dtype == TSG_BF16 ? dw_wgrad_launch<bf16_t, float>(x, dy, dw, B, H, W, C, stride, ws, st)
                           : dw_wgrad_launch<float, double>(x, dy, dw, B, H, W, C, stride, ws, st);
}

}  // extern "C"
