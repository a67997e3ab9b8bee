// 3x3 / stride 1 / padding 1 convolution + BatchNorm (running statistics) (+ residual) (+ ReLU) of inference, one launch:
//
//   y = bf16( relu?( fma(a[oc], u, b[oc]) + float(residual) ) ),   u = the fp32 MFMA accumulation of the convolution
//
// In eval mode a BatchNorm is the affine map a = gamma / sqrt(var + eps), b = beta - a mean of its running statistics, so
// the chain conv3x3 -> BatchNorm -> (+ shortcut) -> ReLU of ResNet's BasicBlock (furnace/base_model/resnet.py:36-53),
// Bottleneck.conv2 (:80-101) and the 3x3 ConvBnRelu layers (seg_oprs.py:24-46: BiSeNet's attention refinement, refines and
// head) needs no pass of its own: tsg_conv3x3_gen_fwd rounds its accumulators to bf16 and writes them, tsg_bn_apply_fwd
// reads them back with the residual and writes again -- two launches, two roundings and three to four passes over the
// map.  Here the accumulators go through the affine map, the residual and the ReLU in fp32 and are rounded ONCE, at the
// store: x (and the residual) are read once, y is written once.  The result is therefore not bit-equal to the chain's.
//
// x [B,H,W,Cin], residual (may be NULL) and y [B,H,W,Cout]: NHWC bf16.  C_in a multiple of 16, C_out a multiple of 64.
//
// K loop: conv3g_fwd_k<64, 4, ..., GLDS>'s (csrc/conv3g.hip), re-instantiated here as dil3_fwd_k (csrc/dilconv.hip) did
// it: implicit GEMM D[oc][pixel] += W[oc][tap, ci] X[tap, ci][pixel] on 32x32x16 MFMAs; a 4-wave block owns 64 output
// channels x 8 x 32 pixels, two blocks per CU; per chunk of 16 input channels the 9 x 64 x 16 filter slab (MFMA fragment
// order, tsg_mfma.h) arrives by LDS-DMA and the (8+2) x (32+2) x 16 patch through registers with predicated loads (zero
// padding) at a 48-byte pixel stride; both LDS images are double-buffered, one barrier per chunk; a wave computes 64 oc x 2
// rows x 32 pixels (4 accumulators), its 12 pixel fragments of a chunk are read once.  69,504 B of LDS.
//
// Epilogue from the accumulators, no staging image: the filter's output channels are permuted inside each group of 32
// (cbn_row_cout, csrc/cbn_geom.h: the host does it with an index_select on the weight before the filter preparation), so
// a lane's 16 accumulator registers are 16 consecutive output channels of one pixel.  The lane reads a, b (fp32 [2][C_out])
// and 32 contiguous bytes of residual, computes fmaf(a, u, b) + float(residual), ReLU, rounds once and stores 32
// contiguous bytes.
//
// The block plan (cbn_geom.h) is a function of the shape alone.  No atomics, no sum split across blocks, no device query,
// no environment switch: results are bit-identical from launch to launch.  No host synchronisation and no allocation: the
// launch can be captured in a graph.
#include "cbn_geom.h"
#include "tsg_mfma.h"

namespace tsg {

constexpr int CBN_PH = CBN_TH + 2, CBN_PW = CBN_TW + 2;  // input patch
constexpr int CBN_PS = 24;                               // LDS pixel stride in bf16: 32 B of data + 16 B of padding
constexpr int CBN_NPX = CBN_PH * CBN_PW;                 // 340 patch pixels
constexpr int CBN_PATCH = CBN_NPX * CBN_PS;              // bf16 elements of one patch buffer (16,320 B)
constexpr int CBN_NPV = CBN_NPX * 2;                     // 16-byte vectors of a patch chunk: 680
constexpr int CBN_NPU = (CBN_NPV + 255) / 256;           // per thread: 3
constexpr int CBN_FELEMS = 9 * CBN_BN * CBN_KC;          // bf16 elements of one filter slab (18,432 B)
constexpr int CBN_NFV = CBN_FELEMS / 8;                  // 1152 16-byte vectors = 18 pieces of 1 KB
constexpr int CBN_NFW = (CBN_NFV / 64 + 3) / 4;          // pieces per wave: 5 (the last one partly)
constexpr size_t CBN_LDS = (size_t)(2 * CBN_FELEMS + 2 * CBN_PATCH) * 2;
static_assert(CBN_LDS <= 80 * 1024, "two blocks per CU");
static_assert(CBN_TH == 8 && CBN_TW == 32 && CBN_BN == 64, "4 waves x 2 rows x 32 pixels x 2 channel blocks of 32");

__global__ __launch_bounds__(256, 2) void cbn_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wf,
                                                     const float* __restrict__ ab, const bf16_t* __restrict__ res,
                                                     bf16_t* __restrict__ y, CbnGeom g, int relu) {
  constexpr int NPU = CBN_NPU, PW = CBN_PW, PS = CBN_PS;
  extern __shared__ __attribute__((aligned(16))) unsigned char cbn_smem[];
  bf16_t* fbuf = reinterpret_cast<bf16_t*>(cbn_smem);                      // [2][CBN_FELEMS]
  bf16_t* pbuf = fbuf + 2 * CBN_FELEMS;                                    // [2][CBN_PATCH]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, p = lane & 31;
  int oct, slot;
  cbn_block(g, (int)blockIdx.x, &oct, &slot);

  int prc[NPU];                                          // patch vector u: pr | pc << 8 | part << 16, or -1
#pragma unroll
  for (int u = 0; u < NPU; ++u) {
    const int v = tid + 256 * u, pp = v >> 1;
    prc[u] = v < CBN_NPV ? ((pp / PW) | ((pp % PW) << 8) | ((v & 1) << 16)) : -1;
  }
  uint4 rp[NPU];
  const bf16_t* wslab = wf + (int64_t)oct * g.nchunks * CBN_FELEMS;
  const float* ap = ab + oct * CBN_BN + half * 16;       // this lane's a: channels oct 64 + j 32 + half 16 + r
  const float* bp = ap + g.Cout;

  for (int tile = slot; tile < g.ntiles; tile += g.nslots) {
    int bimg, oh0, ow0;
    cbn_tile(g, tile, &bimg, &oh0, &ow0);
    const bf16_t* ximg = x + (int64_t)bimg * g.H * g.W * g.Cin;

    auto fetch = [&](int chunk, int buf) {
      const bf16_t* ws = wslab + (int64_t)chunk * CBN_FELEMS;
      unsigned char* fb = reinterpret_cast<unsigned char*>(fbuf + buf * CBN_FELEMS);
#pragma unroll
      for (int u = 0; u < CBN_NFW; ++u) {
        const int q = wave + 4 * u;                      // wave-uniform piece index
        if (u < CBN_NFW - 1 || q < CBN_NFV / 64)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ws + ((int64_t)q * 64 + lane) * 8),
                                           (__attribute__((address_space(3))) void*)(fb + q * 1024), 16, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < NPU; ++u) {
        const int ih = oh0 - 1 + (prc[u] & 0xff), iw = ow0 - 1 + ((prc[u] >> 8) & 0xff);
        rp[u] = make_uint4(0u, 0u, 0u, 0u);
        if (prc[u] >= 0 && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
          rp[u] = *reinterpret_cast<const uint4*>(ximg + ((int64_t)ih * g.W + iw) * g.Cin + chunk * CBN_KC +
                                                  ((prc[u] >> 16) & 1) * 8);
      }
    };
    auto stage = [&](int buf) {
      bf16_t* pbw = pbuf + buf * CBN_PATCH;
#pragma unroll
      for (int u = 0; u < NPU; ++u)
        if (prc[u] >= 0) {
          const int pp = (prc[u] & 0xff) * PW + ((prc[u] >> 8) & 0xff);
          *reinterpret_cast<uint4*>(pbw + pp * PS + ((prc[u] >> 16) & 1) * 8) = rp[u];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;

    // the previous tile's last chunk ended with a barrier and its epilogue does not touch LDS: the buffers are free
    fetch(0, 0);
    stage(0);
    __syncthreads();

    for (int c = 0; c < g.nchunks; ++c) {
      const int buf = c & 1;
      if (c + 1 < g.nchunks) fetch(c + 1, buf ^ 1);      // in flight during the MFMAs of this chunk
      const bf16_t* pb = pbuf + buf * CBN_PATCH + ((2 * wave) * PW + p) * PS + half * 8;
      const bf16_t* fa = fbuf + buf * CBN_FELEMS + lane * 8;
      bf16x8 bq[4][3];                                   // [patch row of the wave][kw]
#pragma unroll
      for (int pr = 0; pr < 4; ++pr)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
          bq[pr][kw] = *reinterpret_cast<const bf16x8*>(pb + (pr * PW + kw) * PS);
      // the filter fragments of tap t + 1 are read while the MFMAs of tap t run: two register sets
      bf16x8 af[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) af[0][j] = *reinterpret_cast<const bf16x8*>(fa + (j * 64) * 8);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int kh = t / 3, kw = t % 3;
        if (t + 1 < 9) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
            af[(t + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(fa + (((t + 1) * 2 + j) * 64) * 8);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t & 1][j], bq[i + kh][kw], acc[j][i], 0, 0, 0);
      }
      if (c + 1 < g.nchunks) stage(buf ^ 1);
      __syncthreads();
    }

    // ---- epilogue: with the permuted filter acc[j][i][r] is oc = oct 64 + j 32 + half 16 + r, pixel (row 2 wave + i, column p)
    const int ow = ow0 + p;
    const int64_t img_off = (int64_t)bimg * g.H * g.W * g.Cout + oct * CBN_BN + half * 16;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float av[16], bv[16];
      ldc<16>(ap, j * 32, av);
      ldc<16>(bp, j * 32, bv);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int oh = oh0 + 2 * wave + i;
        if (oh >= g.H || ow >= g.W) continue;
        const int64_t off = img_off + ((int64_t)oh * g.W + ow) * g.Cout + j * 32;
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = fmaf(av[r], acc[j][i][r], bv[r]);
        if (res) {
          const uint4 r0 = *reinterpret_cast<const uint4*>(res + off), r1 = *reinterpret_cast<const uint4*>(res + off + 8);
          const uint32_t w[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            v[2 * e] += __uint_as_float(w[e] << 16);
            v[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u);
          }
        }
        if (relu) {
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
        }
        uint4 o0, o1;
        o0.x = pack2_bf16(v[0], v[1]);   o0.y = pack2_bf16(v[2], v[3]);   o0.z = pack2_bf16(v[4], v[5]);   o0.w = pack2_bf16(v[6], v[7]);
        o1.x = pack2_bf16(v[8], v[9]);   o1.y = pack2_bf16(v[10], v[11]); o1.z = pack2_bf16(v[12], v[13]); o1.w = pack2_bf16(v[14], v[15]);
        *reinterpret_cast<uint4*>(y + off) = o0;
        *reinterpret_cast<uint4*>(y + off + 8) = o1;
      }
    }
  }
}

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_conv3x3_bnact_supported(int dtype, int64_t B, int64_t H, int64_t W, int Cin, int Cout) {
  CbnGeom g;
  return dtype == TSG_BF16 && cbn_geom(&g, B, H, W, Cin, Cout);
}

int tsg_conv3x3_bnact_row_perm(int* out64) {
  if (!out64) return TSG_E_NULL;
  for (int q = 0; q < CBN_BN; ++q) out64[q] = (q & ~31) + cbn_row_cout(q & 31);
  return 0;
}

int tsg_conv3x3_bnact_plan(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int* out5) {
  if (!out5) return TSG_E_NULL;
  CbnGeom g;
  if (!cbn_geom(&g, B, H, W, Cin, Cout)) return TSG_E_SHAPE;
  out5[0] = g.ntiles; out5[1] = g.nslots; out5[2] = g.noct; out5[3] = g.grid; out5[4] = (int)CBN_LDS;
  return 0;
}

int tsg_conv3x3_bnact_fwd(const void* x, const void* wf, const float* ab, const void* residual, void* y, int64_t B,
                          int64_t H, int64_t W, int Cin, int Cout, int relu, void* stream) {
  if (!x || !wf || !ab || !y) return TSG_E_NULL;
  CbnGeom g;
  if (!cbn_geom(&g, B, H, W, Cin, Cout)) return TSG_E_SHAPE;
  if (!aligned16(x) || !aligned16(wf) || !aligned16(ab) || !aligned16(y) || (residual && !aligned16(residual)))
    return TSG_E_ALIGN;
  TSG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cbn_fwd_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)CBN_LDS));
  hipLaunchKernelGGL(cbn_fwd_k, dim3((unsigned)g.grid), dim3(256), CBN_LDS, (hipStream_t)stream, (const bf16_t*)x,
                     (const bf16_t*)wf, ab, (const bf16_t*)residual, (bf16_t*)y, g, relu ? 1 : 0);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
