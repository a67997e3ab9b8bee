// First convolution of the ResNet-v1c deep stem: Conv2d(3, 64, kernel 3, stride 2, padding 1, bias=False) on a
// [B,3,H,W] image (furnace/base_model/resnet.py:111, ResNet._stem c[0]; FCN, PSPNet, PSANet, DFN and BiSeNet-R101
// build it with deep_stem=True).  The image needs no gradient, so the training step is forward + weight gradient.
// Both are implicit GEMMs with K = 27 taps padded to 32 (two k-steps of mfma_f32_32x32x16_bf16); the MFMA work is
// tiny (3.5 GFLOP at 16 x 512^2) and the kernels are bound by HBM:
//
//   forward : reads x (B*3*H*W*2 bytes) and writes y [B,OH,OW,64] (B*OH*OW*128 bytes): 25.2 + 134.2 MB at 16 x 512^2.
//   wgrad   : reads x and dy [B,OH,OW,64]: 25.2 + 134.2 MB, writes per-block partials (2 MB) that a second kernel
//             folds in a fixed order (fp64) => deterministic, no atomics.
//
// Tap order k = ic * 9 + kh * 3 + kw (the [64,3,3,3] weight flattened), k = 27..31 zero.  A block covers an output
// tile of 4 rows (one per wave) x 32 columns; its input patch (3 channels x 9 rows x 65 columns, zero outside the
// image) is staged in LDS, and each lane gathers the 8 taps of its MFMA fragment from there.
//
// x: NCHW bf16 (any H, W).  y / dy: NHWC bf16 (channels_last).  w / dw: fp32 [64,3,3,3].
#include "tsg_mfma.h"

namespace tsg {

namespace {

constexpr int DS_OC = 64;
constexpr int DS_KP = 32;                      // padded GEMM-K: 27 taps + 5 zero
constexpr int DS_TH = 4, DS_TW = 32;           // output tile: 4 rows (one per wave) x 32 columns
constexpr int DS_PR = 2 * DS_TH + 1;           // 9 input rows per channel
constexpr int DS_PC = 2 * DS_TW + 2;           // 66 input columns (65 used), origin column 2*ow0 - 1
constexpr int DS_NP = 3 * DS_PR * DS_PC;       // 1782 patch elements
constexpr int DS_NPF = (DS_NP + 255) / 256;    // 7 per thread
constexpr int DS_OS = DS_OC + 8;               // LDS row of one output pixel: 64 oc + 8 pad (144 B, 16-B multiple)
constexpr int DS_DS = DS_TH * DS_TW + 8;       // LDS row of dy^T: 128 pixels + 8 pad
constexpr int DS_NPART = 512;                  // persistent blocks of the weight gradient (2 per CU)

struct DsGeom {
  int B, H, W, OH, OW, tiles_h, tiles_w, ntiles;
};

struct DsTile { int b, oh0, ow0; };
__device__ __forceinline__ DsTile ds_tile(const DsGeom& g, int tile) {
  DsTile t;
  t.ow0 = (tile % g.tiles_w) * DS_TW;
  t.oh0 = ((tile / g.tiles_w) % g.tiles_h) * DS_TH;
  t.b = tile / (g.tiles_w * g.tiles_h);
  return t;
}

// patch element u of this thread: channel ic, row 2*oh0 - 1 + rr, column 2*ow0 - 1 + cc; zero outside the image
__device__ __forceinline__ void ds_fetch_patch(const bf16_t* __restrict__ x, const DsGeom& g, const DsTile& t, int tid,
                                               bf16_t (&rp)[DS_NPF]) {
  const int ih0 = 2 * t.oh0 - 1, iw0 = 2 * t.ow0 - 1;
#pragma unroll
  for (int u = 0; u < DS_NPF; ++u) {
    const int idx = tid + 256 * u;
    const int ic = idx / (DS_PR * DS_PC), rem = idx % (DS_PR * DS_PC), rr = rem / DS_PC, cc = rem % DS_PC;
    const int ih = ih0 + rr, iw = iw0 + cc;
    rp[u] = 0;
    if (idx < DS_NP && cc < DS_PC - 1 && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
      rp[u] = x[(((int64_t)t.b * 3 + ic) * g.H + ih) * g.W + iw];
  }
}

__device__ __forceinline__ void ds_store_patch(bf16_t* patch, int tid, const bf16_t (&rp)[DS_NPF]) {
#pragma unroll
  for (int u = 0; u < DS_NPF; ++u)
    if (tid + 256 * u < DS_NP) patch[tid + 256 * u] = rp[u];
}

// offset of tap k inside the patch relative to (row 2*wave, column 2*pixel); -1 for the zero taps 27..31
__device__ __forceinline__ int ds_tap_off(int k) {
  if (k >= 27) return -1;
  const int ic = k / 9, kh = (k / 3) % 3, kw = k % 3;
  return (ic * DS_PR + kh) * DS_PC + kw;
}

// 8 patch elements (zero where off < 0) -> one bf16x8 fragment
__device__ __forceinline__ bf16x8 ds_gather8(const bf16_t* base, const int (&off)[8], int stride) {
  union { uint32_t u[4]; bf16x8 v; } f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t lo = off[2 * j] >= 0 ? base[off[2 * j] + stride * (2 * j)] : 0u;
    const uint32_t hi = off[2 * j + 1] >= 0 ? base[off[2 * j + 1] + stride * (2 * j + 1)] : 0u;
    f.u[j] = lo | (hi << 16);
  }
  return f.v;
}

// ---------------------------------------------------------------- weights -> bf16 [64][32]
__global__ void ds_pack_w(const float* __restrict__ w, bf16_t* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= DS_OC * DS_KP) return;
  const int oc = i / DS_KP, k = i % DS_KP;
  wp[i] = f32_to_bf16(k < 27 ? w[oc * 27 + k] : 0.f);
}

// ---------------------------------------------------------------- forward
// Wave `wr` computes tile row wr: D[oc][pixel] = W[oc][k] * im2col[k][pixel], two 32-oc halves x two k-steps.  The
// tile is re-laid as [pixel][oc] through LDS so that every lane stores 16 B of NHWC.
__global__ __launch_bounds__(256) void ds_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp,
                                                bf16_t* __restrict__ y, DsGeom g) {
  __shared__ __attribute__((aligned(16))) bf16_t patch[DS_NP + 2];              // 3568 B
  __shared__ __attribute__((aligned(16))) bf16_t outs[DS_TH * DS_TW * DS_OS];    // 18432 B
  const int tid = threadIdx.x, lane = tid & 63, wr = tid >> 6, half = lane >> 5, p = lane & 31;
  const DsTile t = ds_tile(g, blockIdx.x);

  bf16_t rp[DS_NPF];
  ds_fetch_patch(x, g, t, tid, rp);
  bf16x8 fw[2][2];                                     // [k-step][oc half]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
      fw[ks][mt] = *reinterpret_cast<const bf16x8*>(wp + (mt * 32 + p) * DS_KP + ks * 16 + half * 8);
  ds_store_patch(patch, tid, rp);
  __syncthreads();

  f32x16 acc[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
  const bf16_t* base = patch + 2 * wr * DS_PC + 2 * p;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    int off[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) off[j] = ds_tap_off(ks * 16 + half * 8 + j);
    const bf16x8 fb = ds_gather8(base, off, 0);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[ks][mt], fb, acc[mt], 0, 0, 0);
  }
  // acc[mt][r]: oc = 32 mt + (r & 3) + 8 (r >> 2) + 4 half, pixel = (row wr, column p)
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      uint2 v;
      v.x = pack2_bf16(acc[mt][4 * gq + 0], acc[mt][4 * gq + 1]);
      v.y = pack2_bf16(acc[mt][4 * gq + 2], acc[mt][4 * gq + 3]);
      *reinterpret_cast<uint2*>(outs + (wr * DS_TW + p) * DS_OS + 32 * mt + 8 * gq + 4 * half) = v;
    }
  __syncthreads();
  // thread -> (pixel column spl, 16-B part spart) of each tile row: a wave stores 1 KB of consecutive NHWC bytes
  const int spl = tid >> 3, spart = tid & 7;
  if (t.ow0 + spl < g.OW) {
    bf16_t* yt = y + (((int64_t)t.b * g.OH + t.oh0) * g.OW + t.ow0 + spl) * DS_OC + spart * 8;
#pragma unroll
    for (int qd = 0; qd < DS_TH; ++qd)
      if (t.oh0 + qd < g.OH)
        *reinterpret_cast<uint4*>(yt + (int64_t)qd * g.OW * DS_OC) =
            *reinterpret_cast<const uint4*>(outs + (qd * DS_TW + spl) * DS_OS + spart * 8);
  }
}

// ---------------------------------------------------------------- forward + BatchNorm (+ ReLU), inference form
// ds_fwd_k with the eval-mode BatchNorm of the layer behind it (ResNet._stem c[1], c[2]) applied to the fp32
// accumulators: y = bf16(relu?(fma(a[oc], u, b[oc]))), one rounding, at the store into the LDS image.  ab = rows 0 and 1
// of tsg_bn_affine's pack ([2][64] fp32, 16-byte aligned).  A lane's 32 channels are eight runs of four
// (32 mt + 8 gq + 4 half ..): eight float4 loads per row, issued with the patch fetch, before the MFMAs.  The only
// traffic ds_fwd_k does not have is those 512 bytes per block (cache hits); the separate BatchNorm pass over y is gone.
// __launch_bounds__(256, 4): the 64 coefficient registers on top of ds_fwd_k's 72 gave 136 = three blocks per CU; bounded
// the kernel takes 122, spill-free, four blocks per CU (a bound of 5 spills 24 registers).
__global__ __launch_bounds__(256, 4) void ds_bnact_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp,
                                                      const float* __restrict__ ab, bf16_t* __restrict__ y, DsGeom g,
                                                      int relu) {
  __shared__ __attribute__((aligned(16))) bf16_t patch[DS_NP + 2];              // 3568 B
  __shared__ __attribute__((aligned(16))) bf16_t outs[DS_TH * DS_TW * DS_OS];    // 18432 B
  const int tid = threadIdx.x, lane = tid & 63, wr = tid >> 6, half = lane >> 5, p = lane & 31;
  const DsTile t = ds_tile(g, blockIdx.x);

  bf16_t rp[DS_NPF];
  ds_fetch_patch(x, g, t, tid, rp);
  bf16x8 fw[2][2];                                     // [k-step][oc half]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
      fw[ks][mt] = *reinterpret_cast<const bf16x8*>(wp + (mt * 32 + p) * DS_KP + ks * 16 + half * 8);
  float4 ca[2][4], cb[2][4];                           // a, b of channels 32 mt + 8 gq + 4 half + 0..3
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      ca[mt][gq] = *reinterpret_cast<const float4*>(ab + 32 * mt + 8 * gq + 4 * half);
      cb[mt][gq] = *reinterpret_cast<const float4*>(ab + DS_OC + 32 * mt + 8 * gq + 4 * half);
    }
  ds_store_patch(patch, tid, rp);
  __syncthreads();

  f32x16 acc[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
  const bf16_t* base = patch + 2 * wr * DS_PC + 2 * p;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    int off[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) off[j] = ds_tap_off(ks * 16 + half * 8 + j);
    const bf16x8 fb = ds_gather8(base, off, 0);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[ks][mt], fb, acc[mt], 0, 0, 0);
  }
  // acc[mt][r]: oc = 32 mt + (r & 3) + 8 (r >> 2) + 4 half, pixel = (row wr, column p)
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      float v[4];
      v[0] = fmaf(ca[mt][gq].x, acc[mt][4 * gq + 0], cb[mt][gq].x);
      v[1] = fmaf(ca[mt][gq].y, acc[mt][4 * gq + 1], cb[mt][gq].y);
      v[2] = fmaf(ca[mt][gq].z, acc[mt][4 * gq + 2], cb[mt][gq].z);
      v[3] = fmaf(ca[mt][gq].w, acc[mt][4 * gq + 3], cb[mt][gq].w);
      if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
      }
      uint2 o;
      o.x = pack2_bf16(v[0], v[1]);
      o.y = pack2_bf16(v[2], v[3]);
      *reinterpret_cast<uint2*>(outs + (wr * DS_TW + p) * DS_OS + 32 * mt + 8 * gq + 4 * half) = o;
    }
  __syncthreads();
  // thread -> (pixel column spl, 16-B part spart) of each tile row: a wave stores 1 KB of consecutive NHWC bytes
  const int spl = tid >> 3, spart = tid & 7;
  if (t.ow0 + spl < g.OW) {
    bf16_t* yt = y + (((int64_t)t.b * g.OH + t.oh0) * g.OW + t.ow0 + spl) * DS_OC + spart * 8;
#pragma unroll
    for (int qd = 0; qd < DS_TH; ++qd)
      if (t.oh0 + qd < g.OH)
        *reinterpret_cast<uint4*>(yt + (int64_t)qd * g.OW * DS_OC) =
            *reinterpret_cast<const uint4*>(outs + (qd * DS_TW + spl) * DS_OS + spart * 8);
  }
}

// ---------------------------------------------------------------- weight gradient
// D[oc][k] = sum_pixel dy^T[oc][pixel] * im2col[pixel][k]: the GEMM K axis is the pixel axis.  dy is transposed
// through LDS; wave wr sums the 32 pixels of tile row wr (two k-steps of 16) for both oc halves.  Persistent blocks
// keep the accumulators in registers over their tiles (the next tile's dy and patch are in flight during the MFMAs),
// then fold the four waves in a fixed order into one partial [64][32] per block.
__global__ __launch_bounds__(256) void ds_wrw_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                float* __restrict__ part, DsGeom g) {
  __shared__ __attribute__((aligned(16))) bf16_t patch[DS_NP + 2];
  __shared__ __attribute__((aligned(16))) bf16_t dyT[DS_OC * DS_DS];             // 17408 B: [oc][pixel of the tile]
  __shared__ __attribute__((aligned(16))) float red[4 * DS_OC * DS_KP];          // 32768 B
  const int tid = threadIdx.x, lane = tid & 63, wr = tid >> 6, half = lane >> 5, p = lane & 31;
  const int spl = tid >> 3, spart = tid & 7;           // dy staging: pixel column spl, 8 channels spart * 8 ..

  const int toff = ds_tap_off(p);                      // this lane's tap (GEMM column)
  int off[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) off[j] = toff;
  const bf16_t* base = patch + 2 * wr * DS_PC + 2 * (half * 8);

  f32x16 acc[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

  bf16_t rp[DS_NPF];
  uint4 rd[DS_TH];
  auto fetch = [&](int tile) {
    const DsTile t = ds_tile(g, tile);
    const bool colok = t.ow0 + spl < g.OW;
    const bf16_t* src = dy + (((int64_t)t.b * g.OH + t.oh0) * g.OW + t.ow0 + spl) * DS_OC + spart * 8;
#pragma unroll
    for (int qd = 0; qd < DS_TH; ++qd)
      rd[qd] = (colok && t.oh0 + qd < g.OH) ? *reinterpret_cast<const uint4*>(src + (int64_t)qd * g.OW * DS_OC)
                                            : make_uint4(0, 0, 0, 0);
    ds_fetch_patch(x, g, t, tid, rp);
  };

  int tile = blockIdx.x;
  if (tile < g.ntiles) fetch(tile);
  for (; tile < g.ntiles; tile += gridDim.x) {
    __syncthreads();                                   // the previous tile's fragment reads are done
    ds_store_patch(patch, tid, rp);
#pragma unroll
    for (int qd = 0; qd < DS_TH; ++qd) {
      const uint32_t wd[4] = {rd[qd].x, rd[qd].y, rd[qd].z, rd[qd].w};
      bf16_t* col = dyT + (spart * 8) * DS_DS + qd * DS_TW + spl;
#pragma unroll
      for (int e = 0; e < 8; ++e) col[e * DS_DS] = (bf16_t)((e & 1) ? (wd[e >> 1] >> 16) : (wd[e >> 1] & 0xffffu));
    }
    __syncthreads();
    if (tile + (int)gridDim.x < g.ntiles) fetch(tile + gridDim.x);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {                   // pixels 16 ks + 8 half + j of tile row wr
      const bf16x8 fb = ds_gather8(base + 2 * 16 * ks, off, 2);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const bf16x8 fa =
            *reinterpret_cast<const bf16x8*>(dyT + (32 * mt + p) * DS_DS + wr * DS_TW + 16 * ks + 8 * half);
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[mt], 0, 0, 0);
      }
    }
  }
  // acc[mt][r]: oc = 32 mt + (r & 3) + 8 (r >> 2) + 4 half, tap = p
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * half;
      red[(wr * DS_OC + oc) * DS_KP + p] = acc[mt][r];
    }
  __syncthreads();
  float* out = part + (int64_t)blockIdx.x * DS_OC * DS_KP;
  for (int i = tid; i < DS_OC * DS_KP; i += 256) {
    const int n = DS_OC * DS_KP;
    out[i] = (red[i] + red[n + i]) + (red[2 * n + i] + red[3 * n + i]);
  }
}

// dw[oc][k] = sum over the per-block partials, fixed order, fp64.  A block folds 16 consecutive entries of the [64][32]
// partial: thread (entry c, slice s) sums partials s, s + 16, ...; the 16 slices are added in order.  128 blocks, so that
// the 2 MB of partials are read chip-wide (32 blocks of 4 slices took 39 us at 512 partials).
constexpr int DS_FOLD_E = 16, DS_FOLD_S = 16;
__global__ __launch_bounds__(256) void ds_wrw_fold(const float* __restrict__ part, int nparts, float* __restrict__ dw) {
  __shared__ double sm[DS_FOLD_S][DS_FOLD_E];
  const int c = threadIdx.x % DS_FOLD_E, s = threadIdx.x / DS_FOLD_E, e = blockIdx.x * DS_FOLD_E + c;
  double a = 0.0;
  for (int b = s; b < nparts; b += DS_FOLD_S) a += (double)part[(int64_t)b * DS_OC * DS_KP + e];
  sm[s][c] = a;
  __syncthreads();
  if (threadIdx.x < DS_FOLD_E) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < DS_FOLD_S; ++q) t += sm[q][c];
    const int oc = e / DS_KP, k = e % DS_KP;
    if (k < 27) dw[oc * 27 + k] = (float)t;
  }
}

size_t ds_align(size_t v) { return (v + 255) / 256 * 256; }
constexpr size_t DS_WP_BYTES = (size_t)DS_OC * DS_KP * sizeof(bf16_t);

bool ds_geom(int64_t B, int64_t H, int64_t W, DsGeom* g) {
  if (B <= 0 || H <= 0 || W <= 0 || H > 0x7fffffffLL || W > 0x7fffffffLL) return false;
  const int64_t OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int64_t th = (OH + DS_TH - 1) / DS_TH, tw = (OW + DS_TW - 1) / DS_TW;
  if (B * th * tw > 0x7fffffffLL) return false;
  g->B = (int)B; g->H = (int)H; g->W = (int)W; g->OH = (int)OH; g->OW = (int)OW;
  g->tiles_h = (int)th; g->tiles_w = (int)tw; g->ntiles = (int)(B * th * tw);
  return true;
}

}  // namespace

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_stem3_conv_supported(int dtype, int Cin, int Cout, int kh, int kw, int stride, int pad, int dilation,
                             int groups, int64_t H, int64_t W) {
  return dtype == TSG_BF16 && Cin == 3 && Cout == DS_OC && kh == 3 && kw == 3 && stride == 2 && pad == 1 &&
         dilation == 1 && groups == 1 && H > 0 && W > 0 && H <= 0x7fffffffLL && W <= 0x7fffffffLL;
}

size_t tsg_stem3_conv_ws_bytes(void) {
  return ds_align(DS_WP_BYTES) + (size_t)DS_NPART * DS_OC * DS_KP * sizeof(float);
}

int tsg_stem3_conv_fwd(const void* x, const float* w, void* y, int64_t B, int64_t H, int64_t W, void* ws,
                       size_t ws_bytes, void* stream) {
  if (!x || !w || !y || !ws) return TSG_E_NULL;
  DsGeom g;
  if (!ds_geom(B, H, W, &g)) return TSG_E_SHAPE;
  if (ws_bytes < ds_align(DS_WP_BYTES)) return TSG_E_WS;
  if (!aligned16(y) || !aligned16(ws) || (((uintptr_t)x) & 1u)) return TSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  bf16_t* wp = (bf16_t*)ws;
  hipLaunchKernelGGL(ds_pack_w, dim3((DS_OC * DS_KP + 255) / 256), dim3(256), 0, st, w, wp);
  TSG_CHECK_LAUNCH();
  hipLaunchKernelGGL(ds_fwd_k, dim3(g.ntiles), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)wp, (bf16_t*)y, g);
  TSG_CHECK_LAUNCH();
  return 0;
}

int tsg_stem3_conv_bnact_supported(int dtype, int64_t B, int64_t H, int64_t W) {
  DsGeom g;
  return dtype == TSG_BF16 && ds_geom(B, H, W, &g);
}

size_t tsg_stem3_conv_bnact_filter_bytes(void) { return DS_WP_BYTES; }

int tsg_stem3_conv_bnact_pack(const float* w, void* wp, void* stream) {
  if (!w || !wp) return TSG_E_NULL;
  if (!aligned16(wp) || (((uintptr_t)w) & 3u)) return TSG_E_ALIGN;
  hipLaunchKernelGGL(ds_pack_w, dim3((DS_OC * DS_KP + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)wp);
  TSG_CHECK_LAUNCH();
  return 0;
}

int tsg_stem3_conv_bnact_fwd(const void* x, const void* wp, const float* ab, void* y, int64_t B, int64_t H, int64_t W,
                             int relu, void* stream) {
  if (!x || !wp || !ab || !y) return TSG_E_NULL;
  DsGeom g;
  if (!ds_geom(B, H, W, &g)) return TSG_E_SHAPE;
  if (!aligned16(y) || !aligned16(wp) || !aligned16(ab) || (((uintptr_t)x) & 1u)) return TSG_E_ALIGN;
  hipLaunchKernelGGL(ds_bnact_fwd_k, dim3(g.ntiles), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (const bf16_t*)wp, ab, (bf16_t*)y, g, relu ? 1 : 0);
  TSG_CHECK_LAUNCH();
  return 0;
}

int tsg_stem3_conv_wrw(const void* x, const void* dy, float* dw, int64_t B, int64_t H, int64_t W, void* ws,
                       size_t ws_bytes, void* stream) {
  if (!x || !dy || !dw || !ws) return TSG_E_NULL;
  DsGeom g;
  if (!ds_geom(B, H, W, &g)) return TSG_E_SHAPE;
  if (ws_bytes < tsg_stem3_conv_ws_bytes()) return TSG_E_WS;
  if (!aligned16(dy) || !aligned16(ws) || (((uintptr_t)x) & 1u)) return TSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)((char*)ws + ds_align(DS_WP_BYTES));
  const int grid = g.ntiles < DS_NPART ? g.ntiles : DS_NPART;
  hipLaunchKernelGGL(ds_wrw_k, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)dy, part, g);
  TSG_CHECK_LAUNCH();
  hipLaunchKernelGGL(ds_wrw_fold, dim3(DS_OC * DS_KP / DS_FOLD_E), dim3(256), 0, st, (const float*)part, grid, dw);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
