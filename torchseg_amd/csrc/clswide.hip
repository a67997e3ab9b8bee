// The wide classifier convolutions: nn.Conv2d(C_in, n_classes, kernel_size=1) with bias for up to 256 classes and C_in up
// to 1024 on a channels_last bf16 feature map — pspnet / psanet network.py (`Conv2d(512, 150, 1)` behind Dropout2d, the
// `Conv2d(1024, 150, 1)` auxiliary head) and fcn network.py (`Conv2d(512, 21, 1)`).  The layouts and the arithmetic are the
// ones of csrc/clshead.hip (x / dx channels_last [B, HW, C], z / dz PLANAR [B, N, HW], fp32 master weight rounded to bf16
// inside, fp32 accumulation on v_mfma_f32_32x32x16_bf16), but the weight (150 x 1024 bf16 = 300 KB) no longer fits in
// registers and H*W is only a multiple of 4 (90^2 = 8100), so a plane starts 8-byte aligned and a group of pixels may lie
// in two images:
//   forward   z[b, n, hw]  = bf16(bias[n] + sum_c W[n, c] x[b, hw, c])   block = 128 pixels (32 per wave) x <= 4 class tiles;
//                                                                      A = W, staged 64 channels at a time through LDS in
//                                                                      fragment order (converted once per block), B = the
//                                                                      pixels straight from global memory in fragment shape;
//                                                                      D rows are classes: planar logits, 64-byte segments
//   dgrad     dx[b, hw, c] = bf16(sum_n dz[b, n, hw] W[n, c])           block = 128 pixels x <= 4 channel tiles; K = classes
//                                                                      padded to 16: A = dz gathered from its planes (2-byte
//                                                                      loads, 64-byte segments), B = the block's W columns,
//                                                                      transposed to fragment order in LDS once
//   wgrad     dW[n, c]     = sum_{b, hw} dz[b, n, hw] x[b, hw, c]       block = <= 3 class tiles x 2 channel tiles x one of S
//                                                                      pixel ranges, its 4 waves interleave the 16-pixel k
//                                                                      steps; A = two 8-byte runs of a dz plane (a run of 4
//                                                                      pixels never leaves an image), B = x gathered; block
//                                                                      sum through LDS in wave order, S <= 8 partials per
//                                                                      element folded in fp64 in split order; dbias[n] by a
//                                                                      plane-sum kernel.  No atomics.
// 1 <= n_classes <= 256, C_in % 64 == 0, 64 <= C_in <= 1024, H*W % 4 == 0.
#include "tsg_mfma.h"

namespace tsg {

constexpr int CW_MAXN = 256;
constexpr int CW_MINC = 64, CW_MAXC = 1024;
constexpr int CW_FNT = 4;            // forward: class tiles per block
constexpr int CW_KC = 64;            // forward: channels per staged weight chunk (4 k steps)
constexpr int CW_DCT = 4;            // dgrad: channel tiles per block
constexpr int CW_WNT = 3;            // wgrad: class tiles per block
constexpr int CW_WCT = 2;            // wgrad: channel tiles per block
constexpr int CW_WSPLIT = 8;         // wgrad: at most this many pixel ranges (= partials per element)
constexpr int CW_WSTEPS = 128;       // wgrad: a pixel range has at least this many k steps (32 per wave)

struct CwGeom { int64_t B, HW, P; int C, N; };

// row of accumulator register r in a 32 x 32 tile
__device__ __forceinline__ int cw_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ uint4 cw_pack8(const float* f) {
  return make_uint4(pack2_bf16(f[0], f[1]), pack2_bf16(f[2], f[3]), pack2_bf16(f[4], f[5]), pack2_bf16(f[6], f[7]));
}

// ---------------------------------------------------------------- forward
// grid (pixel groups of 128, class-tile groups).  wl[t][ks][lane]: the A fragment of class tile t and k step ks of the
// current 64-channel chunk; lane (half, l31) holds W[tile row l31][16 ks + 8 half .. + 7]
__global__ __launch_bounds__(256, 3) void clw_fwd_k(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                 const float* __restrict__ bias, bf16_t* __restrict__ z, CwGeom g, int ntb) {
  __shared__ uint4 wl[CW_FNT * 4 * 64];
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31, wave = tid >> 6;
  const int ntiles = (g.N + 31) >> 5, tile0 = blockIdx.y * ntb;
  const int nt = ntiles - tile0 < ntb ? ntiles - tile0 : ntb;
  const int64_t p = ((int64_t)blockIdx.x * 4 + wave) * 32 + l31;
  const bool ok = p < g.P;
  const bf16_t* xr = x + (ok ? p : g.P - 1) * g.C + half * 8;
  // staging: 8 consecutive threads take 8 consecutive rows of a tile (consecutive 16-byte LDS slots), the next 8 the next
  // 8 channels of the same rows
  const int srow = (tid & 7) | ((tid >> 6) << 3), scg = (tid >> 3) & 7;
  f32x16 acc[CW_FNT];
#pragma unroll
  for (int t = 0; t < CW_FNT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  for (int c0 = 0; c0 < g.C; c0 += CW_KC) {
    uint4 bv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) bv[ks] = *reinterpret_cast<const uint4*>(xr + c0 + ks * 16);
    __syncthreads();                                                       // the previous chunk has been read
#pragma unroll
    for (int t = 0; t < CW_FNT; ++t) {
      if (t < nt) {
        const int n = (tile0 + t) * 32 + srow;
        uint4 pk = make_uint4(0u, 0u, 0u, 0u);
        if (n < g.N) {
          const float* wr = w + (int64_t)n * g.C + c0 + scg * 8;
          const float4 a = *reinterpret_cast<const float4*>(wr), b = *reinterpret_cast<const float4*>(wr + 4);
          pk = make_uint4(pack2_bf16(a.x, a.y), pack2_bf16(a.z, a.w), pack2_bf16(b.x, b.y), pack2_bf16(b.z, b.w));
        }
        wl[(t * 4 + (scg >> 1)) * 64 + (scg & 1) * 32 + srow] = pk;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int t = 0; t < CW_FNT; ++t)
        if (t < nt)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wl[(t * 4 + ks) * 64 + lane]),
                                                           __builtin_bit_cast(bf16x8, bv[ks]), acc[t], 0, 0, 0);
  }
  if (ok) {
    const int64_t b = p / g.HW, hw = p - b * g.HW;
    bf16_t* zb = z + b * g.N * g.HW + hw;
#pragma unroll
    for (int t = 0; t < CW_FNT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = (tile0 + t) * 32 + cw_row(r, half);
          if (n < g.N) zb[(int64_t)n * g.HW] = f32_to_bf16(acc[t][r] + (bias ? bias[n] : 0.f));
        }
      }
  }
}

// ---------------------------------------------------------------- dgrad
// grid (pixel groups of 128, channel groups of 128).  wl[ct][ks][lane] (dynamic, KS KB per channel tile): the B fragment of
// channel tile ct and k step ks; lane (half, l31) holds W[16 ks + 8 half .. + 7][column l31 of the tile], classes >= N zero
__global__ __launch_bounds__(256, 3) void clw_dgrad_k(const bf16_t* __restrict__ dz, const float* __restrict__ w,
                                                   bf16_t* __restrict__ dx, CwGeom g) {
  extern __shared__ uint4 cw_dyn[];
  uint4* wl = cw_dyn;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31, wave = tid >> 6;
  const int KS = (g.N + 15) >> 4, cbase = blockIdx.y * (32 * CW_DCT);
  const int nct = (g.C - cbase) / 32 < CW_DCT ? (g.C - cbase) / 32 : CW_DCT;
  for (int i = tid; i < 2 * KS * 32 * CW_DCT; i += 256) {
    const int c = i & (32 * CW_DCT - 1), g8 = i / (32 * CW_DCT);
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int n = g8 * 8 + e;
      f[e] = (n < g.N && cbase + c < g.C) ? w[(int64_t)n * g.C + cbase + c] : 0.f;
    }
    wl[((c >> 5) * KS + (g8 >> 1)) * 64 + (g8 & 1) * 32 + (c & 31)] = cw_pack8(f);
  }
  __syncthreads();
  const int64_t grp = (int64_t)blockIdx.x * 4 + wave, p = grp * 32 + l31;
  const bool ok = p < g.P;
  const int64_t pc = ok ? p : g.P - 1, b = pc / g.HW, hw = pc - b * g.HW;
  const bf16_t* zb = dz + b * g.N * g.HW + hw;
  f32x16 acc[CW_DCT];
#pragma unroll
  for (int ct = 0; ct < CW_DCT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  for (int ks = 0; ks < KS; ++ks) {
    // A fragment: row = pixel l31 of the group, k = class 16 ks + 8 half + e
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int n = 16 * ks + 8 * half + e;
      h[e] = (ok && n < g.N) ? (uint32_t)zb[(int64_t)n * g.HW] : 0u;
    }
    const uint4 av = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
#pragma unroll
    for (int ct = 0; ct < CW_DCT; ++ct)
      if (ct < nct)
        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av),
                                                          __builtin_bit_cast(bf16x8, wl[(ct * KS + ks) * 64 + lane]), acc[ct], 0, 0, 0);
  }
  // acc[ct][r]: pixel row cw_row(r, half), channel l31.  Lane pairs trade one register so that every lane stores two
  // adjacent channels (4 bytes) of one row: the even lane row ra, the odd lane row rb (csrc/clshead.hip)
  const bool even = (lane & 1) == 0;
#pragma unroll
  for (int ct = 0; ct < CW_DCT; ++ct)
    if (ct < nct) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int ra = 2 * q, rb = 2 * q + 1;
        const float got = __shfl_xor(even ? acc[ct][rb] : acc[ct][ra], 1, 64);
        const int64_t pr = grp * 32 + cw_row(even ? ra : rb, half);
        const uint32_t word = even ? pack2_bf16(acc[ct][ra], got) : pack2_bf16(got, acc[ct][rb]);
        if (pr < g.P) *reinterpret_cast<uint32_t*>(dx + pr * g.C + cbase + ct * 32 + (l31 & ~1)) = word;
      }
    }
}

// ---------------------------------------------------------------- wgrad
// grid (channel pairs of tiles, class-tile groups, splits).  part[split][n][c]
__global__ __launch_bounds__(256, 2) void clw_wgrad_k(const bf16_t* __restrict__ dz, const bf16_t* __restrict__ x,
                                                   float* __restrict__ part, CwGeom g, int64_t steps_per_split) {
  __shared__ float img[CW_WNT * CW_WCT * 32 * 32];                       // the block's sum, wave by wave (fixed order)
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31, wave = tid >> 6;
  const int cbase = blockIdx.x * (32 * CW_WCT), tile0 = blockIdx.y * CW_WNT, ntiles = (g.N + 31) >> 5;
  const int nt = ntiles - tile0 < CW_WNT ? ntiles - tile0 : CW_WNT;
  f32x16 acc[CW_WNT][CW_WCT];
#pragma unroll
  for (int t = 0; t < CW_WNT; ++t)
#pragma unroll
    for (int ct = 0; ct < CW_WCT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][ct][r] = 0.f;
  const int64_t nsteps = (g.P + 15) / 16, s0 = (int64_t)blockIdx.z * steps_per_split;
  const int64_t s1 = s0 + steps_per_split < nsteps ? s0 + steps_per_split : nsteps;
  for (int64_t st = s0 + wave; st < s1; st += 4) {
    const int64_t p0 = st * 16 + 8 * half;
    // A: row = class l31 of tile t, k = the pixels p0 .. p0 + 7 as two runs of 4 (HW % 4 == 0: a run stays in one plane and
    // is 8-byte aligned); runs at or past P and rows >= N are zero
    uint2 run[CW_WNT][2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t pq = p0 + 4 * q, b = pq / g.HW, hw = pq - b * g.HW;
#pragma unroll
      for (int t = 0; t < CW_WNT; ++t) {
        const int n = (tile0 + t) * 32 + l31;
        run[t][q] = make_uint2(0u, 0u);
        if (t < nt && n < g.N && pq < g.P) run[t][q] = *reinterpret_cast<const uint2*>(dz + (b * g.N + n) * g.HW + hw);
      }
    }
    // B: column = channel l31 of tile ct, k = the same 8 pixels, gathered (64-byte segments across the lanes)
    uint4 bv[CW_WCT];
#pragma unroll
    for (int ct = 0; ct < CW_WCT; ++ct) {
      uint32_t h[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = p0 + e < g.P ? (uint32_t)x[(p0 + e) * g.C + cbase + ct * 32 + l31] : 0u;
      bv[ct] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    }
#pragma unroll
    for (int t = 0; t < CW_WNT; ++t)
      if (t < nt) {
        const uint4 av = make_uint4(run[t][0].x, run[t][0].y, run[t][1].x, run[t][1].y);
#pragma unroll
        for (int ct = 0; ct < CW_WCT; ++ct)
          acc[t][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv[ct]),
                                                               acc[t][ct], 0, 0, 0);
      }
  }
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int t = 0; t < CW_WNT; ++t)
#pragma unroll
        for (int ct = 0; ct < CW_WCT; ++ct)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float* q = img + ((t * CW_WCT + ct) * 32 + cw_row(r, half)) * 32 + l31;
            *q = (wv == 0 ? 0.f : *q) + acc[t][ct][r];
          }
    }
    __syncthreads();
  }
  float* dst = part + (int64_t)blockIdx.z * g.N * g.C;
  for (int i = tid; i < CW_WNT * CW_WCT * 32 * 32; i += 256) {
    const int c = i & 31, row = (i >> 5) & 31, ct = (i >> 10) % CW_WCT, t = i / (1024 * CW_WCT);
    const int n = (tile0 + t) * 32 + row;
    if (t < nt && n < g.N) dst[(int64_t)n * g.C + cbase + ct * 32 + c] = img[i];
  }
}

// bias gradient: block (n, b) sums one plane of dz in 8-byte runs; part_b[b][n]
__global__ __launch_bounds__(256) void clw_dbias_k(const bf16_t* __restrict__ dz, float* __restrict__ part_b, CwGeom g) {
  __shared__ float smr[2 * 4];
  const int n = blockIdx.x;
  const int64_t b = blockIdx.y;
  const bf16_t* zp = dz + (b * g.N + n) * g.HW;
  float a = 0.f, dummy = 0.f;
  for (int64_t i = (int64_t)threadIdx.x * 4; i < g.HW; i += 256 * 4) {
    const uint2 v = *reinterpret_cast<const uint2*>(zp + i);
    a += (__uint_as_float(v.x << 16) + __uint_as_float(v.x & 0xffff0000u)) +
         (__uint_as_float(v.y << 16) + __uint_as_float(v.y & 0xffff0000u));
  }
  block_sum2(a, dummy, smr);
  if (threadIdx.x == 0) part_b[b * g.N + n] = a;
}

// dw[i] = sum over the splits, db[n] = sum over the images: fp64, in index order
__global__ __launch_bounds__(256) void clw_fold_k(const float* __restrict__ part, const float* __restrict__ part_b, int nsplit,
                                                  int64_t nimg, int64_t nw, int N, float* __restrict__ dw, float* __restrict__ db) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nw) {
    double t = 0.0;
    for (int s = 0; s < nsplit; ++s) t += (double)part[(int64_t)s * nw + i];
    dw[i] = (float)t;
  } else if (db && i < nw + N) {
    const int64_t n = i - nw;
    double t = 0.0;
    for (int64_t b = 0; b < nimg; ++b) t += (double)part_b[b * N + n];
    db[n] = (float)t;
  }
}

static int cw_geom(CwGeom* g, int64_t B, int64_t HW, int C, int N) {
  if (B <= 0 || HW <= 0 || N <= 0 || N > CW_MAXN || C < CW_MINC || C > CW_MAXC || C % 64 || HW % 4) return TSG_E_SHAPE;
  if (B * HW > 0x3fffffffffLL / C) return TSG_E_SHAPE;                    // the narrow path's limit
  g->B = B; g->HW = HW; g->P = B * HW; g->C = C; g->N = N;
  return 0;
}

// pixel ranges of the weight gradient: a function of the shape only
static int cw_splits(int64_t P, int64_t* steps_per_split) {
  const int64_t nsteps = (P + 15) / 16;
  int64_t s = nsteps / CW_WSTEPS;
  s = s < 1 ? 1 : (s > CW_WSPLIT ? CW_WSPLIT : s);
  const int64_t per = (nsteps + s - 1) / s;
  *steps_per_split = per;
  return (int)((nsteps + per - 1) / per);
}

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_cls_head_wide_supported(int dtype, int Cin, int n_classes, int64_t HW) {
  CwGeom g;
  return dtype == TSG_BF16 && cw_geom(&g, 1, HW, Cin, n_classes) == 0;
}

int tsg_cls_head_wide_fwd(const void* x, const float* w, const float* bias, void* z, int64_t B, int64_t HW, int Cin,
                          int n_classes, void* stream) {
  if (!x || !w || !z) return TSG_E_NULL;
  CwGeom g;
  int e = cw_geom(&g, B, HW, Cin, n_classes);
  if (e) return e;
  if (!aligned16(x) || !aligned16(w)) return TSG_E_ALIGN;
  const int ntiles = (g.N + 31) / 32, ngrp = (ntiles + CW_FNT - 1) / CW_FNT, ntb = (ntiles + ngrp - 1) / ngrp;
  const int64_t blocks = (g.P + 127) / 128;
  if (blocks > 0x7fffffff) return TSG_E_SHAPE;
  hipLaunchKernelGGL(clw_fwd_k, dim3((unsigned)blocks, (unsigned)((ntiles + ntb - 1) / ntb)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, w, bias, (bf16_t*)z, g, ntb);
  TSG_CHECK_LAUNCH();
  return 0;
}

int tsg_cls_head_wide_dgrad(const void* dz, const float* w, void* dx, int64_t B, int64_t HW, int Cin, int n_classes,
                            void* stream) {
  if (!dz || !w || !dx) return TSG_E_NULL;
  CwGeom g;
  int e = cw_geom(&g, B, HW, Cin, n_classes);
  if (e) return e;
  if (!aligned16(dz) || !aligned16(dx)) return TSG_E_ALIGN;
  const int64_t blocks = (g.P + 127) / 128;
  if (blocks > 0x7fffffff) return TSG_E_SHAPE;
  const int KS = (g.N + 15) / 16;
  hipLaunchKernelGGL(clw_dgrad_k, dim3((unsigned)blocks, (unsigned)((g.C + 32 * CW_DCT - 1) / (32 * CW_DCT))), dim3(256),
                     (size_t)KS * CW_DCT * 64 * sizeof(uint4), (hipStream_t)stream, (const bf16_t*)dz, w, (bf16_t*)dx, g);
  TSG_CHECK_LAUNCH();
  return 0;
}

size_t tsg_cls_head_wide_wgrad_ws_bytes(int64_t B, int64_t HW, int Cin, int n_classes) {
  CwGeom g;
  if (cw_geom(&g, B, HW, Cin, n_classes)) return 0;
  int64_t per;
  return ((size_t)cw_splits(g.P, &per) * n_classes * Cin + (size_t)B * n_classes) * sizeof(float);
}

int tsg_cls_head_wide_wgrad(const void* dz, const void* x, float* dw, float* dbias, int64_t B, int64_t HW, int Cin,
                            int n_classes, void* ws, size_t ws_bytes, void* stream) {
  if (!dz || !x || !dw || !ws) return TSG_E_NULL;
  CwGeom g;
  int e = cw_geom(&g, B, HW, Cin, n_classes);
  if (e) return e;
  if (B > 65535) return TSG_E_SHAPE;
  if (ws_bytes < tsg_cls_head_wide_wgrad_ws_bytes(B, HW, Cin, n_classes)) return TSG_E_WS;
  if (!aligned16(dz) || !aligned16(x) || !aligned16(ws)) return TSG_E_ALIGN;
  int64_t per;
  const int nsplit = cw_splits(g.P, &per);
  const int ntiles = (g.N + 31) / 32;
  const int64_t nw = (int64_t)n_classes * Cin;
  float* part = (float*)ws;
  float* part_b = part + (size_t)nsplit * nw;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(clw_wgrad_k, dim3((unsigned)(g.C / (32 * CW_WCT)), (unsigned)((ntiles + CW_WNT - 1) / CW_WNT), (unsigned)nsplit),
                     dim3(256), 0, st, (const bf16_t*)dz, (const bf16_t*)x, part, g, per);
  TSG_CHECK_LAUNCH();
  if (dbias) {
    hipLaunchKernelGGL(clw_dbias_k, dim3((unsigned)n_classes, (unsigned)B), dim3(256), 0, st, (const bf16_t*)dz, part_b, g);
    TSG_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(clw_fold_k, dim3((unsigned)((nw + n_classes + 255) / 256)), dim3(256), 0, st, part, part_b, nsplit, B, nw,
                     n_classes, dw, dbias);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
