// Dilated 3x3 / stride 1 / padding d / dilation d convolution (d = 2, 4) + BatchNorm (running statistics) (+ residual)
// (+ ReLU) of inference, one launch:
//
//   y[b][oh][ow][oc] = bf16( relu?( fma(a[oc], u, b[oc]) + float(residual[b][oh][ow][oc]) ) )
//   u = sum over (kh, kw, ci) of w[oc][kh][kw][ci] * x[b][oh + d (kh - 1)][ow + d (kw - 1)][ci]   (fp32 MFMA accumulation)
//
// These are the middle layers of every Bottleneck in layer3 (d = 2) and layer4 (d = 4) of the PSPNet / PSANet backbones
// (workloads/pspnet.py::_nostride_dilate), which csrc/convbn.hip (dilation 1 only) leaves to tsg_conv3x3_dil_fwd or the
// vendor convolution + tsg_bn_apply_fwd: two launches, two roundings, three passes over the 1/8 map.  Here the
// accumulators go through the affine map, the residual and the ReLU in fp32 and are rounded ONCE, at the store.  The
// result is therefore not bit-equal to the chain's.
//
// x [B,H,W,Cin], residual (may be NULL) and y [B,H,W,Cout]: NHWC bf16.  C_in a multiple of 16, C_out a multiple of 64.
//
// The kernel is the two merged halves put together, and nothing else:
//   * plan: cbn_geom / cbn_block / cbn_tile of csrc/cbn_geom.h as they are -- 8 x 32 pixels x 64 output channels per
//     4-wave block, persistent slots, XCD-aware block ids; none of it depends on the dilation;
//   * K loop: dil3_fwd_k<D>'s (csrc/dilconv.hip).  Per chunk of 16 input channels the 9 x 64 x 16 filter slab (MFMA
//     fragment order, tsg_mfma.h) arrives by LDS-DMA and the (8 + 2D) x (32 + 2D) x 16 patch through registers with
//     predicated loads (zero padding: the load is skipped) at a pixel stride of 48 B (D = 2: conflict-free 16-byte
//     fragment reads) or 32 B (D = 4: 2-way conflicted; padded, 640 pixels would not leave room for two blocks per CU).
//     Both images are double-buffered, one barrier per chunk.  Tap (kh, kw) of tile row r reads the fragment at patch row
//     r + D kh, column shift D kw; only the fragments of the current tap row and of the next are live.
//     LDS: 78,336 B (D = 2) / 77,824 B (D = 4): two blocks per CU;
//   * epilogue: cbn_fwd_k's (csrc/convbn.hip), from the accumulators with no staging image.  The filter's output channels
//     are permuted inside each group of 32 (cbn_row_cout: conv3x3_bnact_pack's filter, which does not depend on the
//     dilation), so a lane's 16 accumulator registers are 16 consecutive output channels of one pixel: the lane reads a, b
//     (fp32 [2][C_out]) and 32 contiguous bytes of residual, rounds once and stores 32 contiguous bytes.
//
// The epilogue does not touch LDS and a tile's last chunk ends with a barrier, so the next tile's first DMA needs no
// barrier of its own (dil3_fwd_k, whose epilogue stages in the filter buffers, needs one).
//
// No atomics, no sum split across blocks, no device query, no environment switch: results are bit-identical from launch
// to launch.  No host synchronisation and no allocation: the launch can be captured in a graph.  Offsets inside one image
// are 32-bit (cbn_geom's limit), the image base is 64-bit.
#include "cbn_geom.h"
#include "tsg_mfma.h"

namespace tsg {

constexpr int DBN_FELEMS = 9 * CBN_BN * CBN_KC;         // bf16 elements of one filter slab (18,432 B)
constexpr int DBN_NFV = DBN_FELEMS / 8;                 // 1152 16-byte vectors = 18 pieces of 1 KB
constexpr int DBN_NFW = (DBN_NFV / 64 + 3) / 4;         // pieces per wave: 5 (the last one partly)
static_assert(CBN_TH == 8 && CBN_TW == 32 && CBN_BN == 64, "4 waves x 2 rows x 32 pixels x 2 channel blocks of 32");

template <int D> struct DbnCfg {
  static constexpr int PH = CBN_TH + 2 * D, PW = CBN_TW + 2 * D, NPX = PH * PW;   // 12 x 36 = 432 / 16 x 40 = 640
  static constexpr int PS = D <= 2 ? 24 : 16;           // LDS pixel stride in bf16 (48 B padded / 32 B)
  static constexpr int PATCH = NPX * PS;                // bf16 elements of one patch buffer
  static constexpr int NPV = NPX * 2;                   // 16-byte vectors of a patch chunk: 864 / 1280
  static constexpr int NPU = (NPV + 255) / 256;         // per thread: 4 / 5
  static constexpr size_t LDS = (size_t)(2 * DBN_FELEMS + 2 * PATCH) * 2;
  static_assert(PH < 256 && PW < 256, "patch coordinates are packed in bytes");
  static_assert(LDS <= 80 * 1024, "two blocks per CU");
};

template <int D>
__global__ __launch_bounds__(256, 2) void dbn_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wf,
                                                     const float* __restrict__ ab, const bf16_t* __restrict__ res,
                                                     bf16_t* __restrict__ y, CbnGeom g, int relu) {
  using Cfg = DbnCfg<D>;
  constexpr int NPU = Cfg::NPU, PW = Cfg::PW, PS = Cfg::PS;
  extern __shared__ __attribute__((aligned(16))) unsigned char dbn_smem[];
  bf16_t* fbuf = reinterpret_cast<bf16_t*>(dbn_smem);                      // [2][DBN_FELEMS]
  bf16_t* pbuf = fbuf + 2 * DBN_FELEMS;                                    // [2][PATCH]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, p = lane & 31;
  int oct, slot;
  cbn_block(g, (int)blockIdx.x, &oct, &slot);

  int prc[NPU];                                          // patch vector u: pr | pc << 8 | part << 16, or -1
#pragma unroll
  for (int u = 0; u < NPU; ++u) {
    const int v = tid + 256 * u, pp = v >> 1;
    prc[u] = v < Cfg::NPV ? ((pp / PW) | ((pp % PW) << 8) | ((v & 1) << 16)) : -1;
  }
  uint4 rp[NPU];
  const bf16_t* wslab = wf + (int64_t)oct * g.nchunks * DBN_FELEMS;
  const float* ap = ab + oct * CBN_BN + half * 16;       // this lane's a: channels oct 64 + j 32 + half 16 + r; b: + C_out

  for (int tile = slot; tile < g.ntiles; tile += g.nslots) {
    int bimg, oh0, ow0;
    cbn_tile(g, tile, &bimg, &oh0, &ow0);
    const bf16_t* ximg = x + (int64_t)bimg * g.H * g.W * g.Cin;

    auto fetch = [&](int chunk, int buf) {
      const bf16_t* ws = wslab + (int64_t)chunk * DBN_FELEMS;
      unsigned char* fb = reinterpret_cast<unsigned char*>(fbuf + buf * DBN_FELEMS);
#pragma unroll
      for (int u = 0; u < DBN_NFW; ++u) {
        const int q = wave + 4 * u;                      // wave-uniform piece index
        if (u < DBN_NFW - 1 || q < DBN_NFV / 64)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ws + ((int64_t)q * 64 + lane) * 8),
                                           (__attribute__((address_space(3))) void*)(fb + q * 1024), 16, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < NPU; ++u) {
        const int ih = oh0 - D + (prc[u] & 0xff), iw = ow0 - D + ((prc[u] >> 8) & 0xff);
        rp[u] = make_uint4(0u, 0u, 0u, 0u);
        if (prc[u] >= 0 && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
          rp[u] = *reinterpret_cast<const uint4*>(ximg + ((int64_t)ih * g.W + iw) * g.Cin + chunk * CBN_KC +
                                                  ((prc[u] >> 16) & 1) * 8);
      }
    };
    auto stage = [&](int buf) {
      bf16_t* pbw = pbuf + buf * Cfg::PATCH;
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
      const bf16_t* pb = pbuf + buf * Cfg::PATCH + ((2 * wave) * PW + p) * PS + half * 8;
      const bf16_t* fa = fbuf + buf * DBN_FELEMS + lane * 8;
      // the six pixel fragments of kernel row kh + 1 (2 tile rows x 3 column shifts) are read while the MFMAs of row kh
      // run, the filter fragments of tap t + 1 during tap t: two register sets each
      bf16x8 bq[2][2][3];                                // [kh & 1][row of the wave][kw]
      auto read_row = [&](int kh) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw)
            bq[kh & 1][i][kw] = *reinterpret_cast<const bf16x8*>(pb + ((i + D * kh) * PW + D * kw) * PS);
      };
      read_row(0);
      bf16x8 af[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) af[0][j] = *reinterpret_cast<const bf16x8*>(fa + (j * 64) * 8);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int kh = t / 3, kw = t % 3;
        if (kw == 0 && kh + 1 < 3) read_row(kh + 1);
        if (t + 1 < 9) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
            af[(t + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(fa + (((t + 1) * 2 + j) * 64) * 8);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t & 1][j], bq[kh & 1][i][kw], acc[j][i], 0, 0, 0);
      }
      if (c + 1 < g.nchunks) stage(buf ^ 1);
      __syncthreads();
    }

    // ---- epilogue: with the permuted filter acc[j][i][r] is oc = oct 64 + j 32 + half 16 + r, pixel (row 2 wave + i, column p)
    const int ow = ow0 + p;
    const int64_t img_off = (int64_t)bimg * g.H * g.W * g.Cout + oct * CBN_BN + half * 16;
    // a and b do not depend on the tile, and loads of them hoisted out of the tile loop are 64 registers live across the
    // K loop (which then spills): the address is made opaque per tile, the loads stay here (L1 / L2 hits)
    const float* apt = ap;
    asm volatile("" : "+v"(apt));
    const float* bpt = apt + g.Cout;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float av[16], bv[16];
      ldc<16>(apt, j * 32, av);
      ldc<16>(bpt, j * 32, bv);
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

static bool dbn_geom(CbnGeom* g, int64_t B, int64_t H, int64_t W, int Cin, int Cout, int dilation) {
  return (dilation == 2 || dilation == 4) && cbn_geom(g, B, H, W, Cin, Cout);
}

template <int D>
static int dbn_launch(const void* x, const void* wf, const float* ab, const void* residual, void* y, const CbnGeom& g,
                      int relu, hipStream_t st) {
  TSG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dbn_fwd_k<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)DbnCfg<D>::LDS));
  hipLaunchKernelGGL((dbn_fwd_k<D>), dim3((unsigned)g.grid), dim3(256), DbnCfg<D>::LDS, st, (const bf16_t*)x,
                     (const bf16_t*)wf, ab, (const bf16_t*)residual, (bf16_t*)y, g, relu ? 1 : 0);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_conv3x3_dil_bnact_supported(int dtype, int64_t B, int64_t H, int64_t W, int Cin, int Cout, int dilation) {
  CbnGeom g;
  return dtype == TSG_BF16 && dbn_geom(&g, B, H, W, Cin, Cout, dilation);
}

int tsg_conv3x3_dil_bnact_plan(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int dilation, int* out5) {
  if (!out5) return TSG_E_NULL;
  CbnGeom g;
  if (!dbn_geom(&g, B, H, W, Cin, Cout, dilation)) return TSG_E_SHAPE;
  out5[0] = g.ntiles; out5[1] = g.nslots; out5[2] = g.noct; out5[3] = g.grid;
  out5[4] = (int)(dilation == 2 ? DbnCfg<2>::LDS : DbnCfg<4>::LDS);
  return 0;
}

int tsg_conv3x3_dil_bnact_fwd(const void* x, const void* wf, const float* ab, const void* residual, void* y, int64_t B,
                              int64_t H, int64_t W, int Cin, int Cout, int dilation, int relu, void* stream) {
  if (!x || !wf || !ab || !y) return TSG_E_NULL;
  CbnGeom g;
  if (!dbn_geom(&g, B, H, W, Cin, Cout, dilation)) return TSG_E_SHAPE;
  if (!aligned16(x) || !aligned16(wf) || !aligned16(ab) || !aligned16(y) || (residual && !aligned16(residual)))
    return TSG_E_ALIGN;
  return dilation == 2 ? dbn_launch<2>(x, wf, ab, residual, y, g, relu, (hipStream_t)stream)
                       : dbn_launch<4>(x, wf, ab, residual, y, g, relu, (hipStream_t)stream);
}

}  // extern "C"
