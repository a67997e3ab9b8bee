// Xception's separable unit in inference form, one launch:
//
//   y = relu?( a * (W_p . dw3x3(x, W_d)) + b (+ residual) )
//
// `SeparableConvBnRelu` of furnace/base_model/xception.py:10-26 has no BatchNorm between its depthwise 3x3 convolution
// and its point-wise ConvBnRelu, so with running statistics the unit is the line above and the depthwise result t never
// has to leave the compute unit.  This replaces tsg_dwconv3x3_fwd + the vendor 1x1 convolution + tsg_bn_apply_fwd (with
// the shortcut addition and ReLU of Block.forward, xception.py:29-63, on a block's last unit): 3 launches and 5-6 passes
// over memory become one launch that reads x (and the residual) once and writes y once.
//
// Operands channels_last: x [B,H,W,C_in], y and residual [B,OH,OW,C_out]; padding 1, dilation 1, stride 1 or 2;
// C_in % 8 == 0 in [8, 256], C_out % 16 == 0 in [16, 256] (csrc/sep_geom.h states the plan and the packed constants).
//
// A block owns a strip of TP consecutive output pixels and all their output channels:
//   1. thread (pixel, 8 channels) forms t the way dw_fwd_k does (fp32 filter, taps kh-major, fp32 accumulation, one
//      rounding to bf16) and stores the 16 bytes to the LDS row of its pixel, rows [pixel][C_in rounded up to 16] with
//      one 16-byte slot of padding between rows (the row stride is an odd number of slots: the 32 rows a fragment read
//      touches fall on different banks); the thread of the last group zeroes the K padding of its row;
//   2. each wave takes (32 output channels) x (32 pixels) tiles: v_mfma_f32_32x32x16_bf16 with the packed W_p as the A
//      operand (one coalesced 16-byte global read per lane and K step, L2-resident) and t as the B operand (one 16-byte
//      LDS read), fp32 accumulation over C_in in ascending K steps;
//   3. epilogue from the accumulators: a lane holds 16 consecutive output channels of one pixel (sep_row_cout), computes
//      fmaf(a, u, b) (+ float(residual)), ReLU, rounds once to bf16 and stores 32 contiguous bytes.
// TSG_F32 (the parity mode) keeps t in fp64 in LDS and runs the point-wise sum and the affine on the VALU in fp64: exact
// products, fp64 accumulation, W_p not rounded, one rounding to fp32.  It exists for parity, not for speed.
//
// No atomics, no sum split across blocks, no device query: results are bit-identical from launch to launch.  No host
// synchronisation and no allocation: the launches can be captured in a graph.
#include "sep_geom.h"
#include "tsg_mfma.h"

namespace tsg {

struct SepArgs {
  int H, W, Cin, Cout, OH, OW, S, nvec, KP, NKS, MT, relu;
  int64_t npix;
  uint32_t ab_off, wp_off;
};

// the eight channels of one pixel, raw: 16 bytes of bf16 or 32 bytes of fp32
template <typename T> struct SepRaw;
template <> struct SepRaw<bf16_t> {
  uint4 v;
  __device__ __forceinline__ void zero() { v = make_uint4(0, 0, 0, 0); }
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void unpack(float* f) const {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(w[i] << 16);
      f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
};
template <> struct SepRaw<float> {
  float4 lo, hi;
  __device__ __forceinline__ void zero() { lo = hi = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void load(const float* p) {
    lo = *reinterpret_cast<const float4*>(p);
    hi = *reinterpret_cast<const float4*>(p + 4);
  }
  __device__ __forceinline__ void unpack(float* f) const {
    f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
    f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
  }
};

// the filter of channel group cv from the pack: wt[tap][8]
__device__ __forceinline__ void sep_load_filter(const float* __restrict__ wd, int cv, float (&wt)[9][8]) {
  const float4* src = reinterpret_cast<const float4*>(wd + (size_t)cv * 72);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float4 lo = src[2 * k], hi = src[2 * k + 1];
    wt[k][0] = lo.x; wt[k][1] = lo.y; wt[k][2] = lo.z; wt[k][3] = lo.w;
    wt[k][4] = hi.x; wt[k][5] = hi.y; wt[k][6] = hi.z; wt[k][7] = hi.w;
  }
}

// t[p][cv 8 .. cv 8 + 7] of output pixel p < npix: the nine taps are fetched first (a tap outside the image is never read
// and counts as zero), then summed kh-major in A, product and sum rounded separately as in dw_fwd_k
template <typename T, typename A>
__device__ __forceinline__ void sep_dw8(const T* __restrict__ x, const float (&wt)[9][8], const SepArgs& g, int64_t p,
                                        int cv, A (&acc)[8]) {
  const int ow = (int)(p % g.OW);
  const int64_t q = p / g.OW;
  const int oh = (int)(q % g.OH);
  const int64_t b = q / g.OH;
  SepRaw<T> raw[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = oh * g.S - 1 + kh;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int iw = ow * g.S - 1 + kw;
      if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
        raw[kh * 3 + kw].load(x + ((b * g.H + ih) * (int64_t)g.W + iw) * g.Cin + cv * 8);
      else
        raw[kh * 3 + kw].zero();
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float xv[8];
    raw[k].unpack(xv);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] += (A)xv[c] * (A)wt[k][c];
  }
}

// ---- bf16: t in LDS as bf16, the point-wise product on the matrix cores
template <int TP>
__global__ __launch_bounds__(SEP_THREADS) void sep_fwd_bf16_k(const bf16_t* __restrict__ x,
                                                              const unsigned char* __restrict__ pack,
                                                              const bf16_t* __restrict__ res, bf16_t* __restrict__ y,
                                                              SepArgs g) {
  __shared__ __attribute__((aligned(16))) bf16_t tl[TP * (SEP_CIN_MAX + SEP_LDS_PAD)];
  const int tid = threadIdx.x;
  const int ldr = g.KP + SEP_LDS_PAD;
  const int64_t p0 = (int64_t)blockIdx.x * TP;

  {  // 1. the strip's t rows
    const int npl = SEP_THREADS / g.nvec;                  // pixel lanes; the threads past npl * nvec have no group
    const int pl = tid / g.nvec, cv = tid - pl * g.nvec;
    if (pl < npl) {
      float wt[9][8];
      sep_load_filter(reinterpret_cast<const float*>(pack), cv, wt);
      for (int pp = pl; pp < TP; pp += npl) {
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.f;
        if (p0 + pp < g.npix) sep_dw8<bf16_t, float>(x, wt, g, p0 + pp, cv, acc);
        uint4 o;
        o.x = pack2_bf16(acc[0], acc[1]);
        o.y = pack2_bf16(acc[2], acc[3]);
        o.z = pack2_bf16(acc[4], acc[5]);
        o.w = pack2_bf16(acc[6], acc[7]);
        *reinterpret_cast<uint4*>(tl + pp * ldr + cv * 8) = o;
        if (cv == g.nvec - 1 && g.KP != g.Cin)              // C_in % 16 == 8: the K padding multiplies packed zeros
          *reinterpret_cast<uint4*>(tl + pp * ldr + g.Cin) = make_uint4(0, 0, 0, 0);
      }
    }
  }
  __syncthreads();

  // 2. tiles of 32 output channels x 32 pixels, 3. epilogue
  constexpr int NT = TP / 32;
  const int wave = tid >> 6, lane = tid & 63, n = lane & 31, h = lane >> 5;
  const float* ab = reinterpret_cast<const float*>(pack + g.ab_off);
  const bf16x8* wp = reinterpret_cast<const bf16x8*>(pack + g.wp_off);
  for (int tile = wave; tile < g.MT * NT; tile += SEP_THREADS / 64) {
    const int mt = tile / NT, nt = tile - mt * NT;
    const bf16x8* ap = wp + (size_t)mt * g.NKS * 64 + lane;
    const bf16_t* bp = tl + (nt * 32 + n) * ldr + h * 8;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int ks = 0; ks < g.NKS; ++ks) {
      const bf16x8 a = ap[ks * 64];
      const bf16x8 b = *reinterpret_cast<const lds_bf16x8*>(bp + ks * 16);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
    const int64_t p = p0 + nt * 32 + n;
    const int co0 = mt * 32 + h * 16;                      // register r of this lane is output channel co0 + r
    if (p >= g.npix || co0 >= g.Cout) continue;
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 a4 = *reinterpret_cast<const float4*>(ab + co0 + 4 * q);
      const float4 b4 = *reinterpret_cast<const float4*>(ab + g.Cout + co0 + 4 * q);
      v[4 * q + 0] = fmaf(a4.x, acc[4 * q + 0], b4.x);
      v[4 * q + 1] = fmaf(a4.y, acc[4 * q + 1], b4.y);
      v[4 * q + 2] = fmaf(a4.z, acc[4 * q + 2], b4.z);
      v[4 * q + 3] = fmaf(a4.w, acc[4 * q + 3], b4.w);
    }
    const int64_t off = p * g.Cout + co0;
    if (res) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        SepRaw<bf16_t> rr;
        rr.load(res + off + 8 * q);
        float rf[8];
        rr.unpack(rf);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[8 * q + c] += rf[c];
      }
    }
    if (g.relu) {
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      uint4 o;
      o.x = pack2_bf16(v[8 * q + 0], v[8 * q + 1]);
      o.y = pack2_bf16(v[8 * q + 2], v[8 * q + 3]);
      o.z = pack2_bf16(v[8 * q + 4], v[8 * q + 5]);
      o.w = pack2_bf16(v[8 * q + 6], v[8 * q + 7]);
      *reinterpret_cast<uint4*>(y + off + 8 * q) = o;
    }
  }
}

// ---- fp32 parity mode: t in LDS as fp64, everything after it on the VALU in fp64
__global__ __launch_bounds__(SEP_THREADS) void sep_fwd_f32_k(const float* __restrict__ x,
                                                             const unsigned char* __restrict__ pack,
                                                             const float* __restrict__ res, float* __restrict__ y,
                                                             SepArgs g) {
  __shared__ double tl[SEP_TP_F32 * SEP_CIN_MAX];
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * SEP_TP_F32;
  {
    const int npl = SEP_THREADS / g.nvec;
    const int pl = tid / g.nvec, cv = tid - pl * g.nvec;
    if (pl < npl) {
      float wt[9][8];
      sep_load_filter(reinterpret_cast<const float*>(pack), cv, wt);
      for (int pp = pl; pp < SEP_TP_F32; pp += npl) {
        double acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.0;
        if (p0 + pp < g.npix) sep_dw8<float, double>(x, wt, g, p0 + pp, cv, acc);
#pragma unroll
        for (int c = 0; c < 8; ++c) tl[pp * g.Cin + cv * 8 + c] = acc[c];
      }
    }
  }
  __syncthreads();
  const float* ab = reinterpret_cast<const float*>(pack + g.ab_off);
  const float* wpt = reinterpret_cast<const float*>(pack + g.wp_off);      // [C_in][C_out]
  for (int o = tid; o < SEP_TP_F32 * g.Cout; o += SEP_THREADS) {
    const int pp = o / g.Cout, co = o - pp * g.Cout;
    const int64_t p = p0 + pp;
    if (p >= g.npix) break;
    const double* t = tl + pp * g.Cin;
    double u = 0.0;
    for (int ci = 0; ci < g.Cin; ++ci) u += (double)wpt[(size_t)ci * g.Cout + co] * t[ci];
    double v = (double)ab[co] * u + (double)ab[g.Cout + co];
    if (res) v += (double)res[p * g.Cout + co];
    if (g.relu && !(v > 0.0)) v = 0.0;
    y[p * g.Cout + co] = (float)v;
  }
}

// the pack of sep_geom.h from W_d [C_in,1,3,3], W_p [C_out,C_in,1,1] and rows 0, 1 of a fwd_pack [3][C_out]
__global__ __launch_bounds__(SEP_THREADS) void sep_pack_k(const float* __restrict__ wd, const float* __restrict__ wp,
                                                          const float* __restrict__ fwd_pack,
                                                          unsigned char* __restrict__ pack, int Cin, int Cout, int NKS,
                                                          int MT, uint32_t ab_off, uint32_t wp_off, int bf16) {
  const int n_wd = Cin * 9, n_ab = 2 * Cout, n_wp = bf16 ? MT * NKS * 512 : Cin * Cout;
  float* o_wd = reinterpret_cast<float*>(pack);
  float* o_ab = reinterpret_cast<float*>(pack + ab_off);
  for (int i = blockIdx.x * SEP_THREADS + threadIdx.x; i < n_wd + n_ab + n_wp; i += gridDim.x * SEP_THREADS) {
    if (i < n_wd) {
      const int cv = i / 72, r = i - cv * 72, tap = r >> 3, e = r & 7;
      o_wd[i] = wd[(cv * 8 + e) * 9 + tap];
    } else if (i < n_wd + n_ab) {
      o_ab[i - n_wd] = fwd_pack[i - n_wd];
    } else if (bf16) {
      const int j = i - n_wd - n_ab;
      const int e = j & 7, lane = (j >> 3) & 63, blk = j >> 9, ks = blk % NKS, mt = blk / NKS;
      const int co = mt * 32 + sep_row_cout(lane & 31), ci = ks * 16 + (lane >> 5) * 8 + e;
      reinterpret_cast<bf16_t*>(pack + wp_off)[j] = (co < Cout && ci < Cin) ? f32_to_bf16(wp[co * Cin + ci]) : (bf16_t)0;
    } else {
      const int j = i - n_wd - n_ab;
      const int ci = j / Cout, co = j - ci * Cout;
      reinterpret_cast<float*>(pack + wp_off)[j] = wp[co * Cin + ci];
    }
  }
}

}  // namespace tsg

using namespace tsg;

static SepArgs sep_args(const SepGeom& g, int relu) {
  SepArgs a;
  a.H = g.H; a.W = g.W; a.Cin = g.Cin; a.Cout = g.Cout; a.OH = g.OH; a.OW = g.OW; a.S = g.stride;
  a.nvec = g.nvec; a.KP = g.KP; a.NKS = g.NKS; a.MT = g.MT; a.relu = relu ? 1 : 0;
  a.npix = g.npix; a.ab_off = (uint32_t)g.ab_off; a.wp_off = (uint32_t)g.wp_off;
  return a;
}

extern "C" {

int tsg_sepconv_supported(int dtype, int Cin, int Cout, int stride, int H, int W) {
  return (dtype == TSG_F32 || dtype == TSG_BF16) && sep_shape_ok(Cin, Cout, stride, 1, H, W);
}

size_t tsg_sepconv_pack_bytes(int dtype, int Cin, int Cout) {
  SepGeom g;
  if ((dtype != TSG_F32 && dtype != TSG_BF16) || !sep_pack_layout(&g, Cin, Cout, dtype == TSG_BF16)) return 0;
  return g.pack_bytes;
}

int tsg_sepconv_pack(const float* wd, const float* wp, const float* fwd_pack, int dtype, int Cin, int Cout, void* pack,
                     void* stream) {
  if (!wd || !wp || !fwd_pack || !pack) return TSG_E_NULL;
  if (dtype != TSG_F32 && dtype != TSG_BF16) return TSG_E_DTYPE;
  SepGeom g;
  if (!sep_pack_layout(&g, Cin, Cout, dtype == TSG_BF16)) return TSG_E_SHAPE;
  if (!aligned16(pack)) return TSG_E_ALIGN;
  const int total = (int)((g.pack_bytes - g.wp_off) / (dtype == TSG_BF16 ? 2 : 4)) + Cin * 9 + 2 * Cout;
  hipLaunchKernelGGL(sep_pack_k, dim3((unsigned)ceil_div_i(total, SEP_THREADS)), dim3(SEP_THREADS), 0,
                     (hipStream_t)stream, wd, wp, fwd_pack, (unsigned char*)pack, Cin, Cout, g.NKS, g.MT,
                     (uint32_t)g.ab_off, (uint32_t)g.wp_off, dtype == TSG_BF16 ? 1 : 0);
  TSG_CHECK_LAUNCH();
  return 0;
}

int tsg_sepconv_fwd(const void* x, const void* pack, const void* residual, void* y, int dtype, int64_t B, int H, int W,
                    int Cin, int Cout, int stride, int relu, void* stream) {
  if (!x || !pack || !y) return TSG_E_NULL;
  if (dtype != TSG_F32 && dtype != TSG_BF16) return TSG_E_DTYPE;
  SepGeom g;
  if (!sep_geom(&g, Cin, Cout, stride, B, H, W, dtype == TSG_BF16)) return TSG_E_SHAPE;
  if (!aligned16(x) || !aligned16(pack) || !aligned16(y) || (residual && !aligned16(residual))) return TSG_E_ALIGN;
  const SepArgs a = sep_args(g, relu);
  const unsigned char* pk = (const unsigned char*)pack;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.grid), block(SEP_THREADS);
  if (dtype == TSG_F32)
    hipLaunchKernelGGL(sep_fwd_f32_k, grid, block, 0, st, (const float*)x, pk, (const float*)residual, (float*)y, a);
  else if (g.TP == SEP_TP_BIG)
    hipLaunchKernelGGL(sep_fwd_bf16_k<SEP_TP_BIG>, grid, block, 0, st, (const bf16_t*)x, pk, (const bf16_t*)residual,
                       (bf16_t*)y, a);
  else
    hipLaunchKernelGGL(sep_fwd_bf16_k<SEP_TP_SMALL>, grid, block, 0, st, (const bf16_t*)x, pk, (const bf16_t*)residual,
                       (bf16_t*)y, a);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
