// PSPNet's pyramid pooling head of inference without the concatenation (furnace side: workloads/pspnet.py
// PyramidPooling.forward), three launches:
//
//   stock:  y = relu(bn(conv3x3(cat([x, up(p_0), ..., up(p_{n-1})]), W6)))          up = bilinear, align_corners=True
//   here:   y = bf16( relu?( fma(a, conv3x3(x, W6[:, :C]) + E, b) ) )
//
// Interpolation and convolution are both linear, so the share of the pooled channels (n Cb of the C + n Cb input channels
// of W6) is contracted on the pooled maps p_s [B, Cb, sh_s, sw_s] -- at most 64 cells per branch -- before it is spread over
// the full map (the arithmetic and the plan: csrc/ppm_geom.h):
//
//   1. ppm_taps_k     T[b][cell][tap][oc] = sum_cb W6[oc][C + s Cb + cb][tap] p_s[b][cell][cb]             fp32
//      One wave per (image, branch, tap, 32 output channels) on v_mfma_f32_32x32x16_bf16: M = oc, N = the cells of the branch
//      padded to 32 or 64, K = Cb.  Both operands come straight from global memory as 16-byte fragments (the branch slices
//      of the weight are packed [s][tap][oc][cb] bf16 once per layer); bf16 products, fp32 accumulation, no LDS.
//   2. ppm_addend_k   E[b][oh][ow][oc], fp32 NHWC: the bilinear interpolation of T, per tap, summed over the taps whose
//      pixel lies inside the map (the concatenated tensor is zero-padded as a whole: the pooled channels are NOT extended
//      past the border).  The interpolation is separable.  A block owns one output row and 64 output channels: it first
//      forms R[kw][col][oc] = sum_{kh valid} sum_cy ly[oh + kh - 1][cy] T[kh][kw][cy][col][oc] in LDS (3 x ncols x 64
//      floats, at most 24 KB), then every pixel of the row sums lx[ow + kw - 1][cx] R[kw][cx] over its valid kw, the branches
//      and the two columns of each: at most 24 LDS reads of 16 bytes per 16 bytes stored.  Taps and weights are src_index's
//      (csrc/tsg_resample.h), the ones tsg_upsample_bilinear_ac_fwd uses.
//   3. pab_fwd_k      tsg_conv3x3_bnact_add_fwd: cbn_fwd_k's K loop, tiles, plan (csrc/cbn_geom.h) and permuted-filter
//      epilogue (csrc/convbn.hip), re-instantiated here as csrc/dilbn.hip re-instantiated dil3_fwd_k's loop.  In the
//      epilogue each lane reads its 16 consecutive fp32 addend values (64 bytes) and adds them to its accumulators before
//      the affine map; ONE rounding, at the store.  It reads the plain layer's filter pack (conv3x3_bnact_pack of
//      W6[:, :C]).  69,504 B of LDS, two blocks per CU.
//
// T and E live in a workspace of the caller's (tsg_ppm_ws_bytes).  No allocation, no host synchronisation, no atomics, no
// sum split across blocks, no device query, no environment switch: the launches can be captured in a graph and their
// results are bit-identical from launch to launch.
#include "cbn_geom.h"
#include "ppm_geom.h"
#include "tsg_mfma.h"
#include "tsg_resample.h"

namespace tsg {

// g.arr[s] by selects: a per-thread index into a kernel argument would send the struct to scratch
__device__ __forceinline__ int ppm_pick(const int (&a)[PPM_MAXN], int s) {
  return s == 0 ? a[0] : s == 1 ? a[1] : s == 2 ? a[2] : a[3];
}

struct PpmScale {
  float sy[PPM_MAXN], sx[PPM_MAXN];                      // ac_scale(sh_s, H), ac_scale(sw_s, W)
};
__device__ __forceinline__ float ppm_pickf(const float (&a)[PPM_MAXN], int s) {
  return s == 0 ? a[0] : s == 1 ? a[1] : s == 2 ? a[2] : a[3];
}

// ---- stage 1: the tap tables ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ppm_taps_k(const bf16_t* __restrict__ p0, const bf16_t* __restrict__ p1,
                                                  const bf16_t* __restrict__ p2, const bf16_t* __restrict__ p3,
                                                  const bf16_t* __restrict__ wb, float* __restrict__ T, PpmGeom g) {
  const int lane = threadIdx.x, row = lane & 31, half = lane >> 5;
  int b, s, tap, oct;
  ppm_tap_block(g, (int)blockIdx.x, &b, &s, &tap, &oct);                   // wave-uniform
  const bf16_t* p = s == 0 ? p0 : s == 1 ? p1 : s == 2 ? p2 : p3;
  const int ncell = ppm_pick(g.sh, s) * ppm_pick(g.sw, s), cell0 = ppm_pick(g.cell0, s);
  // A: row = output channel, 8 consecutive cb per lane half; B: column = cell, the same 8 cb
  const bf16_t* wrow = wb + ((((int64_t)s * 9 + tap) * g.Cout + oct * PPM_OCT + row) * g.Cb + half * 8);
  const bf16_t* pimg = p + ((int64_t)b * ncell * g.Cb + half * 8);
  const bool two = ncell > 32;
  const bool in0 = row < ncell, in1 = row + 32 < ncell;
  const bf16_t* pc0 = pimg + (int64_t)(in0 ? row : 0) * g.Cb;              // a lane without a cell reads nothing
  const bf16_t* pc1 = pimg + (int64_t)(in1 ? row + 32 : 0) * g.Cb;
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
  bf16x8 zero;
#pragma unroll
  for (int e = 0; e < 8; ++e) zero[e] = (__bf16)0.f;
  for (int k0 = 0; k0 < g.Cb; k0 += 16) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(wrow + k0);
    bf16x8 b0 = zero, b1 = zero;
    if (in0) b0 = *reinterpret_cast<const bf16x8*>(pc0 + k0);
    if (in1) b1 = *reinterpret_cast<const bf16x8*>(pc1 + k0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0, acc0, 0, 0, 0);
    if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b1, acc1, 0, 0, 0);
  }
  // acc[4 q + i] of this lane: output channel oct 32 + 8 q + 4 half + i, cell row (+ 32)
  float* tb = T + (((int64_t)b * g.ncells + cell0) * 9 + tap) * g.Cout + oct * PPM_OCT + 4 * half;
  if (in0) {
    float* t = tb + (int64_t)row * 9 * g.Cout;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(t + 8 * q) = make_float4(acc0[4 * q], acc0[4 * q + 1], acc0[4 * q + 2], acc0[4 * q + 3]);
  }
  if (in1) {
    float* t = tb + (int64_t)(row + 32) * 9 * g.Cout;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(t + 8 * q) = make_float4(acc1[4 * q], acc1[4 * q + 1], acc1[4 * q + 2], acc1[4 * q + 3]);
  }
}

// ---- stage 2: the addend -------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 ppm_lerp_acc(float4 acc, float l1, float4 v0, float4 v1) {
  const float l0 = 1.f - l1;                                                // aten::upsample_bilinear2d's pair of weights
  acc.x += l0 * v0.x + l1 * v1.x;
  acc.y += l0 * v0.y + l1 * v1.y;
  acc.z += l0 * v0.z + l1 * v1.z;
  acc.w += l0 * v0.w + l1 * v1.w;
  return acc;
}

constexpr int PPM_Q = PPM_OCB / 4;                                          // float4 per pixel of a block: 16

__global__ __launch_bounds__(256) void ppm_addend_k(const float* __restrict__ T, float* __restrict__ E, PpmGeom g,
                                                     PpmScale sc) {
  __shared__ float4 R[3 * PPM_MAXCOLS * PPM_Q];                             // [kw][col][oc / 4]: 24,576 B
  const int tid = threadIdx.x, q = tid & (PPM_Q - 1), grp = tid >> 4;       // 16 groups of 16 lanes
  int b, oh, oct;
  ppm_add_block(g, (int)blockIdx.x, &b, &oh, &oct);
  const float* Tb = T + (int64_t)b * g.ncells * 9 * g.Cout + oct * PPM_OCB + q * 4;

  // the row stage: R[kw][col] = sum over the valid kh and the two rows cy of ih = oh + kh - 1
  for (int item = grp; item < 3 * g.ncols; item += 16) {
    const int kw = item / g.ncols, col = item - kw * g.ncols;
    const int s = ppm_col_branch(g, col);
    const int sh = ppm_pick(g.sh, s), sw = ppm_pick(g.sw, s);
    const int cell = ppm_pick(g.cell0, s) + (col - ppm_pick(g.col0, s));    // of row cy = 0
    const float scale = ppm_pickf(sc.sy, s);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = oh + kh - 1;
      if (ih < 0 || ih >= g.H) continue;                                    // zero padding of the concatenated tensor
      int i0, i1;
      float l1;
      src_index(scale, ih, sh, i0, i1, l1);
      const float4 v0 = *reinterpret_cast<const float4*>(Tb + ((int64_t)(cell + i0 * sw) * 9 + kh * 3 + kw) * g.Cout);
      const float4 v1 = *reinterpret_cast<const float4*>(Tb + ((int64_t)(cell + i1 * sw) * 9 + kh * 3 + kw) * g.Cout);
      acc = ppm_lerp_acc(acc, l1, v0, v1);
    }
    R[item * PPM_Q + q] = acc;
  }
  __syncthreads();

  // the pixel stage
  float* Erow = E + (((int64_t)b * g.H + oh) * g.W) * g.Cout + oct * PPM_OCB + q * 4;
  for (int ow = grp; ow < g.W; ow += 16) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int iw = ow + kw - 1;
      if (iw < 0 || iw >= g.W) continue;
      const float4* Rk = R + kw * g.ncols * PPM_Q + q;
#pragma unroll
      for (int s = 0; s < PPM_MAXN; ++s) {
        if (s >= g.n) break;
        int i0, i1;
        float l1;
        src_index(sc.sx[s], iw, g.sw[s], i0, i1, l1);
        acc = ppm_lerp_acc(acc, l1, Rk[(g.col0[s] + i0) * PPM_Q], Rk[(g.col0[s] + i1) * PPM_Q]);
      }
    }
    *reinterpret_cast<float4*>(Erow + (int64_t)ow * g.Cout) = acc;
  }
}

// ---- stage 3: the convolution over x with the addend in its epilogue --------------------------------------------------
constexpr int PAB_PH = CBN_TH + 2, PAB_PW = CBN_TW + 2;  // input patch
constexpr int PAB_PS = 24;                               // LDS pixel stride in bf16: 32 B of data + 16 B of padding
constexpr int PAB_NPX = PAB_PH * PAB_PW;                 // 340 patch pixels
constexpr int PAB_PATCH = PAB_NPX * PAB_PS;              // bf16 elements of one patch buffer (16,320 B)
constexpr int PAB_NPV = PAB_NPX * 2;                     // 16-byte vectors of a patch chunk: 680
constexpr int PAB_NPU = (PAB_NPV + 255) / 256;           // per thread: 3
constexpr int PAB_FELEMS = 9 * CBN_BN * CBN_KC;          // bf16 elements of one filter slab (18,432 B)
constexpr int PAB_NFV = PAB_FELEMS / 8;                  // 1152 16-byte vectors = 18 pieces of 1 KB
constexpr int PAB_NFW = (PAB_NFV / 64 + 3) / 4;          // pieces per wave: 5 (the last one partly)
constexpr size_t PAB_LDS = (size_t)(2 * PAB_FELEMS + 2 * PAB_PATCH) * 2;
static_assert(PAB_LDS <= 80 * 1024, "two blocks per CU");
static_assert(CBN_TH == 8 && CBN_TW == 32 && CBN_BN == 64, "4 waves x 2 rows x 32 pixels x 2 channel blocks of 32");

__global__ __launch_bounds__(256, 2) void pab_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wf,
                                                     const float* __restrict__ ab, const float* __restrict__ add,
                                                     bf16_t* __restrict__ y, CbnGeom g, int relu) {
  constexpr int NPU = PAB_NPU, PW = PAB_PW, PS = PAB_PS;
  extern __shared__ __attribute__((aligned(16))) unsigned char pab_smem[];
  bf16_t* fbuf = reinterpret_cast<bf16_t*>(pab_smem);                      // [2][PAB_FELEMS]
  bf16_t* pbuf = fbuf + 2 * PAB_FELEMS;                                    // [2][PAB_PATCH]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, p = lane & 31;
  int oct, slot;
  cbn_block(g, (int)blockIdx.x, &oct, &slot);

  int prc[NPU];                                          // patch vector u: pr | pc << 8 | part << 16, or -1
#pragma unroll
  for (int u = 0; u < NPU; ++u) {
    const int v = tid + 256 * u, pp = v >> 1;
    prc[u] = v < PAB_NPV ? ((pp / PW) | ((pp % PW) << 8) | ((v & 1) << 16)) : -1;
  }
  uint4 rp[NPU];
  const bf16_t* wslab = wf + (int64_t)oct * g.nchunks * PAB_FELEMS;
  const float* ap = ab + oct * CBN_BN + half * 16;       // this lane's a: channels oct 64 + j 32 + half 16 + r
  const float* bp = ap + g.Cout;

  for (int tile = slot; tile < g.ntiles; tile += g.nslots) {
    int bimg, oh0, ow0;
    cbn_tile(g, tile, &bimg, &oh0, &ow0);
    const bf16_t* ximg = x + (int64_t)bimg * g.H * g.W * g.Cin;

    auto fetch = [&](int chunk, int buf) {
      const bf16_t* ws = wslab + (int64_t)chunk * PAB_FELEMS;
      unsigned char* fb = reinterpret_cast<unsigned char*>(fbuf + buf * PAB_FELEMS);
#pragma unroll
      for (int u = 0; u < PAB_NFW; ++u) {
        const int q = wave + 4 * u;                      // wave-uniform piece index
        if (u < PAB_NFW - 1 || q < PAB_NFV / 64)
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
      bf16_t* pbw = pbuf + buf * PAB_PATCH;
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
      const bf16_t* pb = pbuf + buf * PAB_PATCH + ((2 * wave) * PW + p) * PS + half * 8;
      const bf16_t* fa = fbuf + buf * PAB_FELEMS + lane * 8;
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
        float ev[16];                                    // the lane's 64 bytes of the addend
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4 t = *reinterpret_cast<const float4*>(add + off + 4 * e);
          ev[4 * e] = t.x; ev[4 * e + 1] = t.y; ev[4 * e + 2] = t.z; ev[4 * e + 3] = t.w;
        }
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = fmaf(av[r], acc[j][i][r] + ev[r], bv[r]);
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

static void ppm_scales(const PpmGeom& g, PpmScale* sc) {
  for (int s = 0; s < PPM_MAXN; ++s) {
    sc->sy[s] = ac_scale(g.sh[s], g.H);
    sc->sx[s] = ac_scale(g.sw[s], g.W);
  }
}

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_ppm_supported(int dtype, int64_t B, int64_t H, int64_t W, int n, const int* sh, const int* sw, int C, int Cb,
                      int Cout) {
  PpmGeom g;
  CbnGeom c;
  return dtype == TSG_BF16 && ppm_geom(&g, B, H, W, n, sh, sw, Cb, Cout) && cbn_geom(&c, B, H, W, C, Cout);
}

size_t tsg_ppm_ws_bytes(int64_t B, int64_t H, int64_t W, int n, const int* sh, const int* sw, int Cb, int Cout) {
  PpmGeom g;
  return ppm_geom(&g, B, H, W, n, sh, sw, Cb, Cout) ? ppm_ws_bytes(g) : 0;
}

int tsg_ppm_plan(int64_t B, int64_t H, int64_t W, int n, const int* sh, const int* sw, int Cb, int Cout, int64_t* out6) {
  if (!sh || !sw || !out6) return TSG_E_NULL;
  PpmGeom g;
  if (!ppm_geom(&g, B, H, W, n, sh, sw, Cb, Cout)) return TSG_E_SHAPE;
  out6[0] = g.ncells; out6[1] = g.ncols; out6[2] = g.tap_grid; out6[3] = g.add_grid;
  out6[4] = (int64_t)ppm_e_offset(g); out6[5] = (int64_t)ppm_ws_bytes(g);
  return 0;
}

int tsg_ppm_taps_supported(int dtype, int64_t B, int n, const int* sh, const int* sw, int Cb, int Cout) {
  PpmGeom g;
  return dtype == TSG_BF16 && ppm_geom(&g, B, 1, 1, n, sh, sw, Cb, Cout);
}

int tsg_ppm_taps_fwd(const void* p0, const void* p1, const void* p2, const void* p3, const void* wb, float* T, int64_t B,
                     int n, const int* sh, const int* sw, int Cb, int Cout, void* stream) {
  const void* ps[PPM_MAXN] = {p0, p1, p2, p3};
  if (!wb || !T || !sh || !sw) return TSG_E_NULL;
  for (int s = 0; s < (n < 1 ? 1 : n > PPM_MAXN ? PPM_MAXN : n); ++s)
    if (!ps[s]) return TSG_E_NULL;
  PpmGeom g;
  if (!ppm_geom(&g, B, 1, 1, n, sh, sw, Cb, Cout)) return TSG_E_SHAPE;
  if (!aligned16(wb) || !aligned16(T)) return TSG_E_ALIGN;
  for (int s = 0; s < n; ++s)
    if (!aligned16(ps[s])) return TSG_E_ALIGN;
  for (int s = n; s < PPM_MAXN; ++s) ps[s] = ps[0];
  hipLaunchKernelGGL(ppm_taps_k, dim3((unsigned)g.tap_grid), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)ps[0],
                     (const bf16_t*)ps[1], (const bf16_t*)ps[2], (const bf16_t*)ps[3], (const bf16_t*)wb, T, g);
  TSG_CHECK_LAUNCH();
  return 0;
}

int tsg_ppm_addend_supported(int64_t B, int64_t H, int64_t W, int n, const int* sh, const int* sw, int Cout) {
  PpmGeom g;
  return ppm_geom(&g, B, H, W, n, sh, sw, 16, Cout);
}

int tsg_ppm_addend_fwd(const float* T, float* E, int64_t B, int64_t H, int64_t W, int n, const int* sh, const int* sw,
                       int Cout, void* stream) {
  if (!T || !E || !sh || !sw) return TSG_E_NULL;
  PpmGeom g;
  if (!ppm_geom(&g, B, H, W, n, sh, sw, 16, Cout)) return TSG_E_SHAPE;
  if (!aligned16(T) || !aligned16(E)) return TSG_E_ALIGN;
  PpmScale sc;
  ppm_scales(g, &sc);
  hipLaunchKernelGGL(ppm_addend_k, dim3((unsigned)g.add_grid), dim3(256), 0, (hipStream_t)stream, T, E, g, sc);
  TSG_CHECK_LAUNCH();
  return 0;
}

int tsg_conv3x3_bnact_add_supported(int dtype, int64_t B, int64_t H, int64_t W, int Cin, int Cout) {
  CbnGeom g;
  return dtype == TSG_BF16 && cbn_geom(&g, B, H, W, Cin, Cout);
}

int tsg_conv3x3_bnact_add_plan(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int* out5) {
  if (!out5) return TSG_E_NULL;
  CbnGeom g;
  if (!cbn_geom(&g, B, H, W, Cin, Cout)) return TSG_E_SHAPE;
  out5[0] = g.ntiles; out5[1] = g.nslots; out5[2] = g.noct; out5[3] = g.grid; out5[4] = (int)PAB_LDS;
  return 0;
}

int tsg_conv3x3_bnact_add_fwd(const void* x, const void* wf, const float* ab, const float* addend, void* y, int64_t B,
                              int64_t H, int64_t W, int Cin, int Cout, int relu, void* stream) {
  if (!x || !wf || !ab || !addend || !y) return TSG_E_NULL;
  CbnGeom g;
  if (!cbn_geom(&g, B, H, W, Cin, Cout)) return TSG_E_SHAPE;
  if (!aligned16(x) || !aligned16(wf) || !aligned16(ab) || !aligned16(addend) || !aligned16(y)) return TSG_E_ALIGN;
  TSG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pab_fwd_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)PAB_LDS));
  hipLaunchKernelGGL(pab_fwd_k, dim3((unsigned)g.grid), dim3(256), PAB_LDS, (hipStream_t)stream, (const bf16_t*)x,
                     (const bf16_t*)wf, ab, addend, (bf16_t*)y, g, relu ? 1 : 0);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
