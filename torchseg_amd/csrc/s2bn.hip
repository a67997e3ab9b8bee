// 3x3 / stride 2 / padding 1 convolution + BatchNorm (running statistics) (+ residual) (+ ReLU) of inference, one launch:
//
//   y[b][oh][ow][oc] = bf16( relu?( fma(a[oc], u, b[oc]) + float(residual[b][oh][ow][oc]) ) )
//   u = sum over (kh, kw, ci) of w[oc][kh][kw][ci] * x[b][2 oh + kh - 1][2 ow + kw - 1][ci]   (fp32 MFMA accumulation)
//   OH = (H + 1) / 2, OW = (W + 1) / 2
//
// These are BasicBlock.conv1 of layer2 / 3 / 4 and the detail branch's conv_3x3_1 / conv_3x3_2 in BiSeNet-R18, and
// Bottleneck.conv2 of layer2 / 3 / 4 in ResNet-50 / 101, which csrc/convbn.hip (stride 1 only) leaves to the vendor
// convolution + tsg_bn_apply_fwd: two launches, two roundings, an extra pass over the output map.  Here the accumulators go
// through the affine map, the residual and the ReLU in fp32 and are rounded ONCE, at the store.  The result is therefore
// not bit-equal to the chain's.
//
// x [B,H,W,Cin], residual (may be NULL) and y [B,OH,OW,Cout]: NHWC bf16.  C_in a multiple of 16, C_out a multiple of 64.
//
// Plan (csrc/s2b_geom.h): a 4-wave block owns 64 output channels x 4 x 32 OUTPUT pixels, persistent slots, XCD-aware block
// ids.  Wave w computes output row w of the tile: 64 oc x 32 pixels, two accumulators of 32 x 32.
//
// K loop: cbn_fwd_k's structure (csrc/convbn.hip).  Per chunk of 16 input channels the 9 x 64 x 16 filter slab (MFMA
// fragment order, tsg_mfma.h: conv3x3_bnact_pack's filter as it is, the fragment order does not depend on the stride)
// arrives by LDS-DMA and the 9 x 65 x 16 input patch through registers with predicated loads (zero padding: the load is
// skipped); both LDS images are double-buffered, one barrier per chunk.  The stride is in the patch: it is staged as two
// planes, the even patch columns (9 x 33 pixels) and the odd ones (9 x 32), as conv64_fwd_s2_k does, so the 32 lanes of a B
// fragment read consecutive pixels of one plane for every kw (kw = 0: even plane at p, kw = 1: odd plane at p, kw = 2: even
// plane at p + 1) and tap row kh of output row w is patch row 2 w + kh.  A wave reads its 9 pixel fragments of a chunk
// once; the filter fragments of tap t + 1 are read while the MFMAs of tap t run.
//
// What was chosen and why:
//   * 4 x 32 tile, one row per wave: 2 x 18,432 B of filter + 2 x 18,720 B of patch = 74,304 B, two blocks per CU
//     (148,608 B of 160 KB).  An 8 x 32 tile (two rows per wave, 17 x 65 patch) needs about 108 KB: one block per CU and
//     nothing to overlap a block's barrier and prologue with; and the deep layers are short of blocks at batch 1 either
//     way (24 x 48 outputs are 12 tiles of 4 x 32), where the smaller tile gives twice the blocks.
//   * the price: a wave issues 27 16-byte LDS fragment reads (18 filter, 9 pixel) for 18 MFMAs per chunk where cbn_fwd_k
//     issues 30 for 36, so by instruction counts this kernel is nearer the LDS rate than the MFMA rate (eight waves x 27 x
//     8 clocks against two waves per SIMD x 18 x 32 clocks of MFMA per chunk).  Not measured separately.
//   * the patch pixels are 32 B apart, unpadded: a 16-byte fragment read by 32 consecutive pixels is 2-way bank-conflicted,
//     as dbn_fwd_k<4> accepts.  Padding to 48 B would make the two patch buffers 56,160 B and the block 93,024 B: one block
//     per CU.  Only the 9 pixel fragments of the 27 reads are affected.
//
// Epilogue: cbn_fwd_k's, from the accumulators with no staging image and no LDS.  The filter's output channels are permuted
// inside each group of 32 (cbn_row_cout), so a lane's 16 accumulator registers are 16 consecutive output channels of one
// pixel: the lane reads a, b (fp32 [2][C_out]) and 32 contiguous bytes of residual, rounds once and stores 32 contiguous
// bytes.  The epilogue does not touch LDS and a tile's last chunk ends with a barrier, so the next tile's first DMA needs
// no barrier of its own.
//
// No atomics, no sum split across blocks, no device query, no environment switch: results are bit-identical from launch
// to launch.  No host synchronisation and no allocation: the launch can be captured in a graph.  Offsets inside one image
// are below 2^31 (s2b_geom's limits), the image base is 64-bit.
#include "s2b_geom.h"
#include "tsg_mfma.h"

namespace tsg {

constexpr int S2B_PS = 16;                               // LDS pixel stride in bf16: 32 B, unpadded
constexpr int S2B_PATCH = S2B_NPX * S2B_PS;              // bf16 elements of one patch buffer (18,720 B)
constexpr int S2B_NPV = S2B_NPX * 2;                     // 16-byte vectors of a patch chunk: 1170
constexpr int S2B_NPU = (S2B_NPV + 255) / 256;           // per thread: 5
constexpr int S2B_FELEMS = 9 * CBN_BN * CBN_KC;          // bf16 elements of one filter slab (18,432 B)
constexpr int S2B_NFV = S2B_FELEMS / 8;                  // 1152 16-byte vectors = 18 pieces of 1 KB
constexpr int S2B_NFW = (S2B_NFV / 64 + 3) / 4;          // pieces per wave: 5 (the last one partly)
constexpr size_t S2B_LDS = (size_t)(2 * S2B_FELEMS + 2 * S2B_PATCH) * 2;
static_assert(S2B_LDS <= 80 * 1024, "two blocks per CU");
static_assert(S2B_TH == 4 && S2B_TW == 32 && CBN_BN == 64, "4 waves x 1 row x 32 pixels x 2 channel blocks of 32");
static_assert(S2B_PH < 256 && S2B_PW < 256, "patch coordinates are packed in bytes");

__global__ __launch_bounds__(256, 2) void s2b_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wf,
                                                     const float* __restrict__ ab, const bf16_t* __restrict__ res,
                                                     bf16_t* __restrict__ y, S2bGeom g, int relu) {
  constexpr int NPU = S2B_NPU, PS = S2B_PS;
  extern __shared__ __attribute__((aligned(16))) unsigned char s2b_smem[];
  bf16_t* fbuf = reinterpret_cast<bf16_t*>(s2b_smem);                      // [2][S2B_FELEMS]
  bf16_t* pbuf = fbuf + 2 * S2B_FELEMS;                                    // [2][S2B_PATCH]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, p = lane & 31;
  int oct, slot;
  s2b_block(g, (int)blockIdx.x, &oct, &slot);

  int prc[NPU];                                          // patch vector u: pr | pc << 8 | part << 16, or -1
#pragma unroll
  for (int u = 0; u < NPU; ++u) {
    const int v = tid + 256 * u, pp = v >> 1;
    prc[u] = v < S2B_NPV ? ((pp / S2B_PW) | ((pp % S2B_PW) << 8) | ((v & 1) << 16)) : -1;
  }
  uint4 rp[NPU];
  const bf16_t* wslab = wf + (int64_t)oct * g.nchunks * S2B_FELEMS;
  const float* ap = ab + oct * CBN_BN + half * 16;       // this lane's a: channels oct 64 + j 32 + half 16 + r; b: + C_out

  for (int tile = slot; tile < g.ntiles; tile += g.nslots) {
    int bimg, oh0, ow0;
    s2b_tile(g, tile, &bimg, &oh0, &ow0);
    const bf16_t* ximg = x + (int64_t)bimg * g.H * g.W * g.Cin;

    auto fetch = [&](int chunk, int buf) {
      const bf16_t* ws = wslab + (int64_t)chunk * S2B_FELEMS;
      unsigned char* fb = reinterpret_cast<unsigned char*>(fbuf + buf * S2B_FELEMS);
#pragma unroll
      for (int u = 0; u < S2B_NFW; ++u) {
        const int q = wave + 4 * u;                      // wave-uniform piece index
        if (u < S2B_NFW - 1 || q < S2B_NFV / 64)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ws + ((int64_t)q * 64 + lane) * 8),
                                           (__attribute__((address_space(3))) void*)(fb + q * 1024), 16, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < NPU; ++u) {
        const int ih = s2b_patch_ih(oh0, prc[u] & 0xff), iw = s2b_patch_iw(ow0, (prc[u] >> 8) & 0xff);
        rp[u] = make_uint4(0u, 0u, 0u, 0u);
        if (prc[u] >= 0 && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
          rp[u] = *reinterpret_cast<const uint4*>(ximg + ((int64_t)ih * g.W + iw) * g.Cin + chunk * CBN_KC +
                                                  ((prc[u] >> 16) & 1) * 8);
      }
    };
    auto stage = [&](int buf) {
      bf16_t* pbw = pbuf + buf * S2B_PATCH;
#pragma unroll
      for (int u = 0; u < NPU; ++u)
        if (prc[u] >= 0) {
          const int pp = s2b_patch_lds(prc[u] & 0xff, (prc[u] >> 8) & 0xff);
          *reinterpret_cast<uint4*>(pbw + pp * PS + ((prc[u] >> 16) & 1) * 8) = rp[u];
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // the previous tile's last chunk ended with a barrier and its epilogue does not touch LDS: the buffers are free
    fetch(0, 0);
    stage(0);
    __syncthreads();

    for (int c = 0; c < g.nchunks; ++c) {
      const int buf = c & 1;
      if (c + 1 < g.nchunks) fetch(c + 1, buf ^ 1);      // in flight during the MFMAs of this chunk
      const bf16_t* pb = pbuf + buf * S2B_PATCH + half * 8;
      const bf16_t* fa = fbuf + buf * S2B_FELEMS + lane * 8;
      bf16x8 bq[3][3];                                   // [kh][kw]: patch pixel (2 wave + kh, 2 p + kw)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
          bq[kh][kw] = *reinterpret_cast<const bf16x8*>(pb + s2b_tap_lds(wave, p, kh, kw) * PS);
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
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t & 1][j], bq[kh][kw], acc[j], 0, 0, 0);
      }
      if (c + 1 < g.nchunks) stage(buf ^ 1);
      __syncthreads();
    }

    // ---- epilogue: with the permuted filter acc[j][r] is oc = oct 64 + j 32 + half 16 + r, pixel (row wave, column p)
    const int oh = oh0 + wave, ow = ow0 + p;
    if (oh >= g.OH || ow >= g.OW) continue;              // no barrier follows in this iteration
    const int64_t off0 = (int64_t)bimg * g.OH * g.OW * g.Cout + ((int64_t)oh * g.OW + ow) * g.Cout + oct * CBN_BN + half * 16;
    // a and b do not depend on the tile; loads of them hoisted out of the tile loop would be live across the K loop: the
    // address is made opaque per tile, the loads stay here (L1 / L2 hits)
    const float* apt = ap;
    asm volatile("" : "+v"(apt));
    const float* bpt = apt + g.Cout;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float av[16], bv[16];
      ldc<16>(apt, j * 32, av);
      ldc<16>(bpt, j * 32, bv);
      const int64_t off = off0 + j * 32;
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = fmaf(av[r], acc[j][r], bv[r]);
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

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_conv3x3_s2_bnact_supported(int dtype, int64_t B, int64_t H, int64_t W, int Cin, int Cout) {
  S2bGeom g;
  return dtype == TSG_BF16 && s2b_geom(&g, B, H, W, Cin, Cout);
}

int tsg_conv3x3_s2_bnact_plan(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int* out7) {
  if (!out7) return TSG_E_NULL;
  S2bGeom g;
  if (!s2b_geom(&g, B, H, W, Cin, Cout)) return TSG_E_SHAPE;
  out7[0] = g.OH; out7[1] = g.OW; out7[2] = g.ntiles; out7[3] = g.nslots; out7[4] = g.noct; out7[5] = g.grid;
  out7[6] = (int)S2B_LDS;
  return 0;
}

int tsg_conv3x3_s2_bnact_fwd(const void* x, const void* wf, const float* ab, const void* residual, void* y, int64_t B,
                             int64_t H, int64_t W, int Cin, int Cout, int relu, void* stream) {
  if (!x || !wf || !ab || !y) return TSG_E_NULL;
  S2bGeom g;
  if (!s2b_geom(&g, B, H, W, Cin, Cout)) return TSG_E_SHAPE;
  if (!aligned16(x) || !aligned16(wf) || !aligned16(ab) || !aligned16(y) || (residual && !aligned16(residual)))
    return TSG_E_ALIGN;
  TSG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&s2b_fwd_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)S2B_LDS));
  hipLaunchKernelGGL(s2b_fwd_k, dim3((unsigned)g.grid), dim3(256), S2B_LDS, (hipStream_t)stream, (const bf16_t*)x,
                     (const bf16_t*)wf, ab, (const bf16_t*)residual, (bf16_t*)y, g, relu ? 1 : 0);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
