// 1x1 / padding 0 convolution, stride 1 or 2, + BatchNorm (running statistics) (+ residual) (+ ReLU) of inference, one launch:
//
//   y = bf16( relu?( fma(a[oc], u, b[oc]) + float(residual) ) ),   u = the fp32 MFMA accumulation of the convolution
//
// The point-wise layers of ResNet's Bottleneck (conv1, and conv3 with the block's shortcut and final ReLU:
// furnace/base_model/resnet.py:80-101), the 1x1 `downsample` shortcuts (:21-31) and the 1x1 ConvBnRelu layers
// (seg_oprs.py:24-46: FeatureFusion.conv_1x1, the PSP / PSA reductions).  Unfused, these are a 1x1 convolution that rounds
// its sums to bf16 and writes them, and tsg_bn_apply_fwd that reads them back with the residual and writes again: two
// launches, two roundings.  Here the accumulators go through the affine map, the residual and the ReLU in fp32 and are
// rounded ONCE, at the store.  The result is therefore not bit-equal to the two-launch chain's.
//
// x [B,H,W,Cin], residual (may be NULL) and y [B,OH,OW,Cout]: NHWC bf16.  Cin and Cout multiples of 64 in [64, 2048].
//
// The GEMM D[oc][pixel] += W[oc][ci] X[ci][pixel] on v_mfma_f32_32x32x16_bf16 (types of tsg_mfma.h, plan of pwb_geom.h).  A
// 4-wave block owns 64 output channels x 256 output pixels per step; a wave 64 x 64 (four accumulators), two blocks per CU.
// * B operand (x): global memory -> registers, never through LDS.  For a 1x1 convolution the channels of an NHWC pixel are
//   already the k-run of the B operand.  Lane (p = lane & 31, half = lane >> 5) owns pixel p of a 32-pixel group, and for a
//   chunk of 64 input channels loads the 64 contiguous bytes half 64 .. of that pixel's chunk (four 16-byte loads; the two
//   halves cover the 128-byte line): MFMA step ks multiplies channels half 32 + ks 8 .. (pwb_lane_ci), the packed filter is
//   laid out to match.  The stride-2 sub-sampling is the row address (pwb_row), computed once per tile; the host gathers
//   nothing.  A lane whose pixel lies past the end of the last tile reads pixel 0's row instead (in bounds) and stores
//   nothing: a column of B reaches only its own column of D, so what such a lane multiplies is never seen.  (Zeros under a
//   predicate, the first form, compiled to one exec-masked branch per 16-byte load, eight per chunk.)  The next chunk's
//   loads are issued before the MFMAs of the current one (two register sets, the chunk loop is unrolled twice).
// * A operand (filter): packed once per layer in fragment order (pwb_filter_decode); the 8 KB slab of an (oc tile, chunk)
//   arrives in LDS by __builtin_amdgcn_global_load_lds (8 pieces of 1 KB, two per wave), double-buffered, one barrier per
//   chunk, shared by the block's waves.  16,384 B of LDS.
// * Epilogue: cbn_fwd_k's (csrc/convbn.hip).  The filter's rows are permuted inside each group of 32 (cbn_row_cout), so a
//   lane's 16 accumulator registers are 16 consecutive output channels of one pixel: a, b, 32 contiguous bytes of residual,
//   fmaf, add, ReLU, one rounding, 32 contiguous bytes stored.  No staging image.
//
// The block plan is a function of the shape alone.  No atomics, no sum split across blocks, no device query, no environment
// switch: results are bit-identical from launch to launch.  No host synchronisation and no allocation: the launch can be
// captured in a graph.
#include "pwb_geom.h"
#include "tsg_mfma.h"

namespace tsg {

static_assert(PWB_BN == 64 && PWB_KC == 64 && PWB_TP == 256, "4 waves x 2 groups of 32 pixels x 2 channel blocks of 32");
static_assert(2 * PWB_LDS <= 160 * 1024, "two blocks per CU");
constexpr int PWB_NKS = PWB_KC / 16;                     // MFMA steps per chunk: 4

__global__ __launch_bounds__(256, 2) void pwb_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wf,
                                                     const float* __restrict__ ab, const bf16_t* __restrict__ res,
                                                     bf16_t* __restrict__ y, PwbGeom g, int relu) {
  __shared__ __attribute__((aligned(16))) bf16_t fbuf[2 * PWB_FELEMS];     // [2][ks][ocb][lane][8]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, p = lane & 31;
  int oct, slot;
  pwb_block(g, (int)blockIdx.x, &oct, &slot);
  const bf16_t* wslab = wf + (int64_t)oct * g.nchunks * PWB_FELEMS;
  const float* ap = ab + oct * PWB_BN + half * 16;       // this lane's a: channels oct 64 + j 32 + half 16 + r
  const float* bp = ap + g.Cout;

  for (int tile = slot; tile < g.ntiles; tile += g.nslots) {
    int pix[2];
    bool ok[2];
    const bf16_t* xp[2];                                 // this lane's 32 channels of chunk 0 of its two pixels (past P: of pixel 0)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      pix[i] = tile * PWB_TP + wave * 64 + i * 32 + p;
      ok[i] = pix[i] < g.P;
      xp[i] = x + (int64_t)pwb_row(g, ok[i] ? pix[i] : 0) * g.Cin + pwb_lane_ci(half, 0);
    }

    auto fetch = [&](int chunk, int buf, uint4 (&xr)[2][PWB_NKS]) {
      const bf16_t* ws = wslab + (int64_t)chunk * PWB_FELEMS;
      unsigned char* fb = reinterpret_cast<unsigned char*>(fbuf + buf * PWB_FELEMS);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = wave + 4 * u;                      // wave-uniform piece index, 0..7
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ws + (q * 64 + lane) * 8),
                                         (__attribute__((address_space(3))) void*)(fb + q * 1024), 16, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int ks = 0; ks < PWB_NKS; ++ks)
          xr[i][ks] = *reinterpret_cast<const uint4*>(xp[i] + chunk * PWB_KC + (pwb_lane_ci(half, ks) - pwb_lane_ci(half, 0)));
    };

    f32x16 acc[2][2];                                    // [oc block j][pixel group i]
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;

    auto compute = [&](int buf, const uint4 (&xr)[2][PWB_NKS]) {
      const bf16_t* fa = fbuf + buf * PWB_FELEMS + lane * 8;
#pragma unroll
      for (int ks = 0; ks < PWB_NKS; ++ks) {
        bf16x8 af[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) af[j] = *reinterpret_cast<const lds_bf16x8*>(fa + ((ks * 2 + j) * 64) * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[j], __builtin_bit_cast(bf16x8, xr[i][ks]), acc[j][i], 0, 0, 0);
      }
    };

    uint4 xa[2][PWB_NKS], xb[2][PWB_NKS];
    __syncthreads();                                     // every wave is done with the previous tile's last slab
    fetch(0, 0, xa);
    for (int c = 0; c < g.nchunks; c += 2) {
      __syncthreads();                                   // slab c has landed (the fence drains the LDS-DMA), slab c - 1 is free
      if (c + 1 < g.nchunks) fetch(c + 1, 1, xb);        // in flight during the MFMAs of this chunk
      compute(0, xa);
      if (c + 1 < g.nchunks) {
        __syncthreads();
        if (c + 2 < g.nchunks) fetch(c + 2, 0, xa);
        compute(1, xb);
      }
    }

    // ---- epilogue: with the permuted filter acc[j][i][r] is oc = oct 64 + j 32 + half 16 + r of pixel pix[i]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float av[16], bv[16];
      ldc<16>(ap, j * 32, av);
      ldc<16>(bp, j * 32, bv);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (!ok[i]) continue;
        const int64_t off = (int64_t)pix[i] * g.Cout + oct * PWB_BN + j * 32 + half * 16;
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

// fp32 weight [Cout][Cin] -> the packed bf16 filter (round to nearest even); one 16-byte vector per thread
__global__ __launch_bounds__(256) void pwb_prep_filter_k(const float* __restrict__ w, bf16_t* __restrict__ wf, int Cin,
                                                         int nvec) {
  const int vec = blockIdx.x * 256 + threadIdx.x;
  if (vec >= nvec) return;
  int oc, ci0;
  pwb_filter_decode(vec, Cin / PWB_KC, &oc, &ci0);
  float v[8];
  ldc<8>(w, (int64_t)oc * Cin + ci0, v);
  *reinterpret_cast<uint4*>(wf + (int64_t)vec * 8) =
      make_uint4(pack2_bf16(v[0], v[1]), pack2_bf16(v[2], v[3]), pack2_bf16(v[4], v[5]), pack2_bf16(v[6], v[7]));
}

static inline bool pwb_channels_ok(int Cin, int Cout) {
  return Cin >= PWB_CMIN && Cin <= PWB_CMAX && Cin % PWB_KC == 0 && Cout >= PWB_CMIN && Cout <= PWB_CMAX && Cout % PWB_BN == 0;
}

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_conv1x1_bnact_supported(int dtype, int64_t B, int64_t H, int64_t W, int Cin, int Cout, int stride) {
  PwbGeom g;
  return dtype == TSG_BF16 && pwb_geom(&g, B, H, W, Cin, Cout, stride);
}

int tsg_conv1x1_bnact_plan(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int stride, int* out5) {
  if (!out5) return TSG_E_NULL;
  PwbGeom g;
  if (!pwb_geom(&g, B, H, W, Cin, Cout, stride)) return TSG_E_SHAPE;
  out5[0] = g.ntiles; out5[1] = g.nslots; out5[2] = g.noct; out5[3] = g.grid; out5[4] = PWB_LDS;
  return 0;
}

size_t tsg_conv1x1_bnact_filter_bytes(int Cin, int Cout) {
  return pwb_channels_ok(Cin, Cout) ? (size_t)Cin * Cout * sizeof(bf16_t) : 0;
}

int tsg_conv1x1_bnact_prep_filter(const float* w, void* wf, int Cin, int Cout, void* stream) {
  if (!w || !wf) return TSG_E_NULL;
  if (!pwb_channels_ok(Cin, Cout)) return TSG_E_SHAPE;
  if (!aligned16(w) || !aligned16(wf)) return TSG_E_ALIGN;
  const int nvec = Cin * Cout / 8;
  hipLaunchKernelGGL(pwb_prep_filter_k, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     (bf16_t*)wf, Cin, nvec);
  TSG_CHECK_LAUNCH();
  return 0;
}

int tsg_conv1x1_bnact_fwd(const void* x, const void* wf, const float* ab, const void* residual, void* y, int64_t B,
                          int64_t H, int64_t W, int Cin, int Cout, int stride, int relu, void* stream) {
  if (!x || !wf || !ab || !y) return TSG_E_NULL;
  PwbGeom g;
  if (!pwb_geom(&g, B, H, W, Cin, Cout, stride)) return TSG_E_SHAPE;
  if (!aligned16(x) || !aligned16(wf) || !aligned16(ab) || !aligned16(y) || (residual && !aligned16(residual)))
    return TSG_E_ALIGN;
  hipLaunchKernelGGL(pwb_fwd_k, dim3((unsigned)g.grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (const bf16_t*)wf, ab, (const bf16_t*)residual, (bf16_t*)y, g, relu ? 1 : 0);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
