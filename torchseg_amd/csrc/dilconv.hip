// Dilated 3x3 / stride 1 / padding d / dilation d convolutions (d = 2, 4), bf16 channels_last, on the bf16 MFMA: forward,
// data gradient and weight gradient of the 3x3 layers that workloads/pspnet.py::_nostride_dilate makes of ResNet-v1c's
// layer3 (dilation 2) and layer4 (dilation 4) — the backbone of PSPNet and PSANet.  C_in a multiple of 16, C_out a multiple
// of 64, as in csrc/conv3g.hip.
//
// Structure: the WIDER HALO, not the phase lattices.  A dilation-d layer is d^2 plain convolutions on the sub-lattices
// x[:, i::d, j::d], and the plain kernels' tile loops would carry over with a pixel pitch of d — but the shipped maps are
// 90^2 and 60^2: a phase of a 90^2 map at d = 4 is 23 x 23 (or 22 x 22) pixels and fills 3 tiles of 8 x 32 to 69 %, at
// d = 2 it is 45 x 45 in 12 tiles: 66 %.  The dense map fills its 12 x 3 tiles to 88 %, so a third more of the MFMA work
// is useful, and the price is staging: the patch of an 8 x 32 tile grows from 10 x 34 to (8 + 2d) x (32 + 2d) pixels,
// 1.27x (d = 2) / 1.88x (d = 4) the bytes per MFMA, read from L2 (XCD-aware mapping, as conv3g_fwd_k) while the MFMAs of
// the previous chunk run.  The kernel stays on the MFMA side of that trade as long as two blocks share a CU, which
// decides the LDS layout below.
//
// dil3_fwd_k<D, STATS> (forward; data gradient with the mode-1 filter):
//   * conv3g_fwd_k's loop: implicit GEMM D[oc][pixel] += W[oc][tap, ci] X[tap, ci][pixel], 32x32x16 MFMAs, a 4-wave block
//     owns 64 output channels x 8 x 32 pixels and walks C_in in chunks of 16, both LDS images double-buffered, the filter
//     slab (fragment order of tsg_mfma.h, written by tsg_conv3x3_gen_prep_filter at tile width 64: independent of the
//     dilation) by LDS-DMA, the patch through registers with predicated loads (zero padding), one barrier per chunk;
//   * a wave computes 64 oc x 2 rows x 32 pixels; tap (kh, kw) of tile row r reads the pixel fragment at patch row
//     r + d kh, column shift d kw: 18 fragment reads per chunk for the 36 MFMAs, one kernel row ahead of their use;
//   * LDS: 2 x 18,432 B of filter + 2 patches.  d = 2: 432 pixels at 48 B (conflict-free fragment reads) = 78,336 B in
//     all; d = 4: 640 pixels, stored unpadded at 32 B (2-way conflicted reads, which conv3h_fwd_k showed the LDS pipe has
//     to spare) = 77,824 B.  Either way two blocks per CU (160 KB), inside 256 VGPRs;
//   * epilogue as conv3g_fwd_k: through LDS, 16-byte NHWC stores, optional addend, optional per-channel sums / square sums
//     of the bf16-rounded outputs folded in a fixed order into partial[slot][2][C_out].
//   The output may have a channel count that is a multiple of 16 only (the data gradient of a layer with such a C_in):
//   the filter is then prepared for the count rounded up to 64 (zero rows) and the surplus channels are not stored.
//
// dil3_wrw_k<D> (weight gradient): conv3_wrw_gen_k's scheme (csrc/conv3wrw.hip) — GEMM M = oc, N = (tap, ci), K = pixels; a
// block owns one (64 oc, 64 ci) pair and every bpp-th 4 x 32 pixel tile, keeps the [64 x 576] accumulator in MFMA registers
// over all its tiles, both operands stay pixel-major in LDS and the K = pixel fragments come from transposing reads, so a
// tap is a pixel offset: (d kh, d kw) in a (4 + 2d) x (32 + 2d) patch.  The x fragment of patch row pr serves every (tile
// row, kh) with row + d kh = pr.  Next tile's operands are prefetched into registers by raw buffer loads (out-of-image
// positions and channels beyond C_in carry an offset past num_records: zeros).  One block per CU (116,736 B of LDS at
// d = 4).  Partials [pair][slot][64][9][64] are folded in fp64 in slot order by dil3_wrw_fold_k: no atomics, bit-equal runs.
#include "tsg_mfma.h"

namespace tsg {

constexpr int DL_TH = 8, DL_TW = 32;                     // output tile of the forward kernel
constexpr int DL_KC = 16;                                // input channels per chunk
constexpr int DL_BN = 64;                                // output channels per block
constexpr int DL_FELEMS = 9 * DL_BN * DL_KC;             // bf16 elements of one filter slab (18,432 B)
constexpr int DL_NFV = DL_FELEMS / 8;                    // 1152 16-byte vectors = 18 pieces of 1 KB
constexpr int DL_OS = DL_BN + 8;                         // epilogue staging: bf16 per pixel
static_assert(256 * DL_OS <= 2 * DL_FELEMS, "the output tile is staged in the two filter buffers");

template <int D> struct DlCfg {
  static constexpr int PH = DL_TH + 2 * D, PW = DL_TW + 2 * D, NPX = PH * PW;
  static constexpr int PS = D <= 2 ? 24 : 16;            // LDS pixel stride in bf16 (48 B padded / 32 B)
  static constexpr int PATCH = NPX * PS;
  static constexpr int NPV = NPX * 2;                    // 16-byte vectors of a patch chunk: 864 / 1280
  static constexpr int NPU = (NPV + 255) / 256;          // per thread: 4 / 5
  static constexpr size_t LDS = (size_t)(2 * DL_FELEMS + 2 * PATCH) * 2;
  static_assert(LDS <= 80 * 1024, "two blocks per CU");
};

struct DlGeom {
  int B, H, W, Cin, Cout, Cst;                           // Cout: padded to 64 (the filter's), Cst: channels of y (its pitch)
  int tiles_h, tiles_w, ntiles, nchunks, noct, nslots;
};

template <int D, bool STATS>
__global__ __launch_bounds__(256, 2) void dil3_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wf,
                                                      bf16_t* __restrict__ y, DlGeom g, float* __restrict__ partial,
                                                      const bf16_t* __restrict__ addend) {
  using Cfg = DlCfg<D>;
  constexpr int NPU = Cfg::NPU, PW = Cfg::PW, PS = Cfg::PS, OS = DL_OS;
  extern __shared__ __attribute__((aligned(16))) unsigned char dl_smem[];
  bf16_t* fbuf = reinterpret_cast<bf16_t*>(dl_smem);                       // [2][DL_FELEMS]
  bf16_t* pbuf = fbuf + 2 * DL_FELEMS;                                     // [2][PATCH]
  bf16_t* outs = fbuf;                                                     // epilogue: [256 pixels][OS]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, p = lane & 31;
  // XCD-aware persistent mapping: the blocks of one slot (same pixel tiles, all oc tiles) sit on one XCD
  const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
  const int oct = jb % g.noct, slot = (jb / g.noct) * 8 + xcd;

  int prc[NPU];                                          // patch vector u: pr | pc << 8 | part << 16, or -1
#pragma unroll
  for (int u = 0; u < NPU; ++u) {
    const int v = tid + 256 * u, pp = v >> 1;
    prc[u] = v < Cfg::NPV ? ((pp / PW) | ((pp % PW) << 8) | ((v & 1) << 16)) : -1;
  }
  uint4 rp[NPU];
  constexpr int NFW = (DL_NFV / 64 + 3) / 4;             // 1 KB pieces of a slab per wave: 5 (the last one partly)
  const bf16_t* wslab = wf + (int64_t)oct * g.nchunks * DL_FELEMS;

  float st1[8], st2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { st1[e] = 0.f; st2[e] = 0.f; }

  for (int tile = slot; tile < g.ntiles; tile += g.nslots) {
    const int ow0 = (tile % g.tiles_w) * DL_TW, oh0 = ((tile / g.tiles_w) % g.tiles_h) * DL_TH;
    const int bimg = tile / (g.tiles_w * g.tiles_h);
    const bf16_t* ximg = x + (int64_t)bimg * g.H * g.W * g.Cin;

    auto fetch = [&](int chunk, int buf) {
      const bf16_t* ws = wslab + (int64_t)chunk * DL_FELEMS;
      unsigned char* fb = reinterpret_cast<unsigned char*>(fbuf + buf * DL_FELEMS);
#pragma unroll
      for (int u = 0; u < NFW; ++u) {
        const int q = wave + 4 * u;                      // wave-uniform piece index
        if (u < NFW - 1 || q < DL_NFV / 64)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ws + ((int64_t)q * 64 + lane) * 8),
                                           (__attribute__((address_space(3))) void*)(fb + q * 1024), 16, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < NPU; ++u) {
        const int ih = oh0 - D + (prc[u] & 0xff), iw = ow0 - D + ((prc[u] >> 8) & 0xff);
        rp[u] = make_uint4(0u, 0u, 0u, 0u);
        if (prc[u] >= 0 && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
          rp[u] = *reinterpret_cast<const uint4*>(ximg + ((int64_t)ih * g.W + iw) * g.Cin + chunk * DL_KC +
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

    __syncthreads();                                     // the DMA writes LDS at once: the previous tile's epilogue must be done
    fetch(0, 0);
    stage(0);
    __syncthreads();

    for (int c = 0; c < g.nchunks; ++c) {
      const int buf = c & 1;
      if (c + 1 < g.nchunks) fetch(c + 1, buf ^ 1);      // in flight during the MFMAs of this chunk
      const bf16_t* pb = pbuf + buf * Cfg::PATCH + ((2 * wave) * PW + p) * PS + half * 8;
      const bf16_t* fa = fbuf + buf * DL_FELEMS + lane * 8;
      // the six pixel fragments of kernel row kh + 1 (2 tile rows x 3 column shifts) are read while the MFMAs of row kh
      // run, the filter fragments of tap t + 1 during tap t: two register sets each
      bf16x8 bq[2][2][3];                             // [kh & 1][row of the wave][kw]
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

    // ---- epilogue: acc[j][i][r] is oc = j 32 + (r & 3) + 8 (r >> 2) + 4 half, pixel (row 2 wave + i, column p)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          uint2 v;
          v.x = pack2_bf16(acc[j][i][4 * gq + 0], acc[j][i][4 * gq + 1]);
          v.y = pack2_bf16(acc[j][i][4 * gq + 2], acc[j][i][4 * gq + 3]);
          *reinterpret_cast<uint2*>(outs + ((2 * wave + i) * DL_TW + p) * OS + j * 32 + 8 * gq + 4 * half) = v;
        }
    __syncthreads();
    const int64_t img_off = (int64_t)bimg * g.H * g.W * g.Cst + oct * DL_BN;
    bf16_t* yimg = y + img_off;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                        // 256 pixels x 8 vectors over 256 threads
      const int v = tid + 256 * k, px = v >> 3, part = v & 7;
      const int oh = oh0 + (px >> 5), ow = ow0 + (px & 31);
      if (oh < g.H && ow < g.W && oct * DL_BN + part * 8 < g.Cst) {
        uint4 o = *reinterpret_cast<const uint4*>(outs + px * OS + part * 8);
        const int64_t off = ((int64_t)oh * g.W + ow) * g.Cst + part * 8;
        if (addend) o = add_bf16x8(o, *reinterpret_cast<const uint4*>(addend + img_off + off));
        *reinterpret_cast<uint4*>(yimg + off) = o;
        if (STATS) {                                     // the values just stored: no second pass over the tile
          const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(w[e] << 16), hi = __uint_as_float(w[e] & 0xffff0000u);
            st1[2 * e] += lo; st2[2 * e] = fmaf(lo, lo, st2[2 * e]);
            st1[2 * e + 1] += hi; st2[2 * e + 1] = fmaf(hi, hi, st2[2 * e + 1]);
          }
        }
      }
    }
    // the next tile's first __syncthreads() orders these reads before the buffers are rewritten
  }

  if (STATS) {                                           // fold the 32 pixel groups in a fixed order
    __syncthreads();
    float* red = reinterpret_cast<float*>(fbuf);         // [32][2][64] floats = 16 KB: the filter buffers are free now
    const int part = tid & 7, q = tid >> 3;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(q * 2 + 0) * DL_BN + part * 8 + e] = st1[e];
      red[(q * 2 + 1) * DL_BN + part * 8 + e] = st2[e];
    }
    __syncthreads();
    if (tid < 2 * DL_BN) {
      const int c = tid % DL_BN, which = tid / DL_BN;
      float sacc = 0.f;
      for (int qq = 0; qq < 32; ++qq) sacc += red[(qq * 2 + which) * DL_BN + c];
      partial[((int64_t)slot * 2 + which) * g.Cst + oct * DL_BN + c] = sacc;
    }
  }
}

// ---------------------------------------------------------------- weight gradient
constexpr int DW_C = 64;                                 // channels of a pair, both ways
constexpr int DW_N = 9 * DW_C;                           // 576 = (tap, ci)
constexpr int DW_TH = 4, DW_TW = 32;                     // dy tile: 128 pixels = 8 K steps of 16
constexpr int DW_RBE = 96;                               // bf16 per pixel row in LDS: 64 channels + 32 pad (conv3wrw.hip)
constexpr int DW_DY = DW_TH * DW_TW * DW_RBE;

template <int D> struct DwCfg {
  static constexpr int PR = DW_TH + 2 * D, PC = DW_TW + 2 * D, NPX = PR * PC;       // 8 x 36 / 12 x 40
  static constexpr int XU = (NPX * 8 + 255) / 256;                                 // 16-byte x chunks per thread: 9 / 15
  static constexpr size_t LDS = (size_t)(DW_DY + NPX * DW_RBE) * 2;                // 79,872 B / 116,736 B
};

struct DwGeom {
  int B, H, W, tiles_h, tiles_w, ntiles;
  int Cin, Cout, nci, npairs, bpp, xs;                   // ci tiles (the last may be partial), pairs, slots per pair, XCDs per slot
};

template <int D>
__global__ __launch_bounds__(256, 1) void dil3_wrw_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                      float* __restrict__ part, DwGeom g) {
  typedef DwCfg<D> P;
  extern __shared__ __attribute__((aligned(16))) unsigned char dw_smem[];
  bf16_t* dyL = reinterpret_cast<bf16_t*>(dw_smem);    // [128 pixels][DW_RBE]
  bf16_t* xL = dyL + DW_DY;                            // [NPX pixels][DW_RBE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wh = wave & 1;             // oc half, ci half of the pair
  const int half = lane >> 5, sub = (lane >> 4) & 1, i16 = lane & 15;
  // the pairs of a slot (same pixel tiles) are consecutive block ids on one XCD (two with xs == 2): conv3_wrw_gen_k
  const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
  const int pps = g.npairs / g.xs;
  const int pair = (g.xs == 2 ? (xcd & 1) * pps : 0) + jb % pps;
  const int slot = (jb / pps) * (8 / g.xs) + (g.xs == 2 ? xcd >> 1 : xcd);
  const int oc0 = (pair / g.nci) * DW_C, ci0 = (pair % g.nci) * DW_C;

  const int spart = tid & 7, spix = tid >> 3;
  const bool cok = ci0 + spart * 8 < g.Cin;            // a partial last ci tile: its missing channels are zeros
  int xr[P::XU], xc[P::XU];
  uint32_t dyo[DW_TH], xo32[P::XU];                    // tile-independent byte offsets of this thread's chunks
#pragma unroll
  for (int u = 0; u < P::XU; ++u) {
    const int pp = spix + 32 * u;
    xr[u] = pp < P::NPX ? pp / P::PC : -1;
    xc[u] = pp % P::PC;
    xo32[u] = (uint32_t)((((int64_t)(xr[u] < 0 ? 0 : xr[u]) * g.W + xc[u]) * g.Cin + spart * 8) * 2);
  }
#pragma unroll
  for (int u = 0; u < DW_TH; ++u) dyo[u] = (uint32_t)((((int64_t)u * g.W + spix) * g.Cout + spart * 8) * 2);
  const int chan = 16 * sub + 4 * (i16 & 3);
  const lds_v4i16* afr = (const lds_v4i16*)(dyL + (8 * half + (i16 >> 2)) * DW_RBE + chan + 32 * wm);
  const lds_v4i16* bfr = (const lds_v4i16*)(xL + (8 * half + (i16 >> 2)) * DW_RBE + chan + 32 * wh);

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  uint4 rd[DW_TH], rx[P::XU];
  auto fetch = [&](int tile) {
    constexpr uint32_t kOob = 0x80000000u;             // >= num_records: the buffer unit returns zeros
    const bool live = tile < g.ntiles;                 // beyond the block's last tile: no access at all
    const int tl = live ? tile : 0;
    const int ow0 = (tl % g.tiles_w) * DW_TW, oh0 = ((tl / g.tiles_w) % g.tiles_h) * DW_TH;
    const int b = tl / (g.tiles_w * g.tiles_h);
    const int ih0 = oh0 - D, iw0 = ow0 - D;            // input pixel of patch (0, 0)
    const bf16_t* dbase = dy + (((int64_t)b * g.H + oh0) * g.W + ow0) * g.Cout + oc0;
    const bf16_t* xbase = x + (((int64_t)b * g.H + ih0) * g.W + iw0) * g.Cin + ci0;
    const __amdgpu_buffer_rsrc_t rd_ = __builtin_amdgcn_make_buffer_rsrc((void*)dbase, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc((void*)xbase, 0, 0x7fffffff, 0x00020000);
    const bool colok = live && ow0 + spix < g.W;
#pragma unroll
    for (int u = 0; u < DW_TH; ++u) {
      const uint32_t off = (colok && oh0 + u < g.H) ? dyo[u] : kOob;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rd_, (int)off, 0, 0);
      rd[u] = make_uint4(v.x, v.y, v.z, v.w);
    }
#pragma unroll
    for (int u = 0; u < P::XU; ++u) {
      const bool ok = live && cok && xr[u] >= 0 && (uint32_t)(ih0 + xr[u]) < (uint32_t)g.H &&
                      (uint32_t)(iw0 + xc[u]) < (uint32_t)g.W;
      const uint32_t off = ok ? xo32[u] : kOob;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rx_, (int)off, 0, 0);
      rx[u] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  union Frag { v4i16 q[2]; bf16x8 v; };

  int tile = slot;
  if (tile < g.ntiles) fetch(tile);
  for (; tile < g.ntiles; tile += g.bpp) {
    __syncthreads();                                   // the previous tile's fragment reads are done
#pragma unroll
    for (int u = 0; u < DW_TH; ++u) *reinterpret_cast<uint4*>(dyL + (spix + 32 * u) * DW_RBE + spart * 8) = rd[u];
#pragma unroll
    for (int u = 0; u < P::XU; ++u)
      if (xr[u] >= 0) *reinterpret_cast<uint4*>(xL + (spix + 32 * u) * DW_RBE + spart * 8) = rx[u];
    __syncthreads();
    fetch(tile + g.bpp);                               // in flight during the MFMAs (all lanes out of range past the end)
    // dy fragments of the 8 K steps (tile row ks >> 1, columns 16 (ks & 1) + 8 half ..) stay in registers; the x fragment
    // at patch (row pr, column 16 c + D kw) serves every kernel row kh with pr - D kh a tile row
    Frag fa[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      fa[ks].q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(afr + (ks * 16 + 0) * (DW_RBE / 4)));
      fa[ks].q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(afr + (ks * 16 + 4) * (DW_RBE / 4)));
    }
#pragma unroll
    for (int pr = 0; pr < P::PR; ++pr)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int px = pr * P::PC + c * 16 + D * kw;   // patch pixel of the fragment's first K
          Frag fb;
          fb.q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(bfr + (px + 0) * (DW_RBE / 4)));
          fb.q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(bfr + (px + 4) * (DW_RBE / 4)));
#pragma unroll
          for (int kh = 0; kh < 3; ++kh) {
            const int rr = pr - D * kh;
            if (rr >= 0 && rr < DW_TH)
              acc[kh * 3 + kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2 * rr + c].v, fb.v, acc[kh * 3 + kw], 0, 0, 0);
          }
        }
  }
  // partial of this (pair, slot): [pair][slot][64 oc][9 taps][64 ci]
  float* out = part + ((int64_t)pair * g.bpp + slot) * DW_C * DW_N;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = 32 * wm + (r & 3) + 8 * (r >> 2) + 4 * half;
      out[oc * DW_N + t * DW_C + 32 * wh + (lane & 31)] = acc[t][r];
    }
}

// dw[oc][tap][ci] = the pair's bpp partials summed in slot order in fp64; one thread per float4 of dw
__global__ __launch_bounds__(256) void dil3_wrw_fold_k(const float* __restrict__ part, DwGeom g, float* __restrict__ dw,
                                                       int64_t nvec) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvec) return;
  const int cv = g.Cin / 4;
  const int ci = (int)(v % cv) * 4;
  const int64_t row = v / cv;                          // oc * 9 + tap
  const int tap = (int)(row % 9), oc = (int)(row / 9);
  const int pair = (oc / DW_C) * g.nci + ci / DW_C;
  const float* src = part + (int64_t)pair * g.bpp * DW_C * DW_N + (oc % DW_C) * DW_N + tap * DW_C + ci % DW_C;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int s = 0; s < g.bpp; ++s) {
    const float4 t = *reinterpret_cast<const float4*>(src + (int64_t)s * DW_C * DW_N);
    a0 += (double)t.x; a1 += (double)t.y; a2 += (double)t.z; a3 += (double)t.w;
  }
  *reinterpret_cast<float4*>(dw + row * g.Cin + ci) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
}

static int dl_geom(DlGeom* g, int64_t B, int64_t H, int64_t W, int Cin, int Cout, int dilation) {
  if (dilation != 2 && dilation != 4) return TSG_E_SHAPE;
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % DL_KC || Cout % 16) return TSG_E_SHAPE;
  const int Cp = (Cout + DL_BN - 1) / DL_BN * DL_BN;
  const int64_t th = (H + DL_TH - 1) / DL_TH, tw = (W + DL_TW - 1) / DL_TW;
  if (B * th * tw > 0x7fffffffLL || H * W * (int64_t)(Cin > Cp ? Cin : Cp) > 0x7fffffffLL) return TSG_E_SHAPE;
  g->B = (int)B; g->H = (int)H; g->W = (int)W; g->Cin = Cin; g->Cout = Cp; g->Cst = Cout;
  g->tiles_h = (int)th; g->tiles_w = (int)tw; g->ntiles = (int)(B * th * tw);
  g->nchunks = Cin / DL_KC; g->noct = Cp / DL_BN;
  int64_t ns = 512 / g->noct;                            // two blocks per CU, a multiple of 8 slots per oc tile
  if (ns > g->ntiles) ns = g->ntiles;
  ns = (ns + 7) / 8 * 8;
  if (ns < 8) ns = 8;
  g->nslots = (int)ns;
  return 0;
}

static int dw_geom(DwGeom* g, int64_t B, int64_t H, int64_t W, int Cin, int Cout, int dilation) {
  if (dilation != 2 && dilation != 4) return TSG_E_SHAPE;
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % 16 || Cout % DW_C) return TSG_E_SHAPE;
  const int64_t th = (H + DW_TH - 1) / DW_TH, tw = (W + DW_TW - 1) / DW_TW;
  if (B * th * tw > 0x7fffffffLL || B * H * W * (int64_t)(Cin > Cout ? Cin : Cout) > 0x7fffffff00LL) return TSG_E_SHAPE;
  // a thread's byte offsets inside one tile's patch are 32-bit buffer offsets below the out-of-range marker
  if ((int64_t)(DW_TH + 2 * dilation + 1) * W * (Cin > Cout ? Cin : Cout) * 2 >= 0x40000000LL) return TSG_E_SHAPE;
  g->B = (int)B; g->H = (int)H; g->W = (int)W;
  g->tiles_h = (int)th; g->tiles_w = (int)tw; g->ntiles = (int)(B * th * tw);
  g->Cin = Cin; g->Cout = Cout; g->nci = (Cin + DW_C - 1) / DW_C; g->npairs = (Cout / DW_C) * g->nci;
  int bpp = (256 + g->npairs - 1) / g->npairs;           // one block per CU
  if (bpp > g->ntiles) bpp = g->ntiles;
  if (bpp < 1) bpp = 1;
  g->xs = (bpp <= 4 && g->npairs % 2 == 0 && g->npairs * 8 > 256) ? 2 : 1;
  g->bpp = g->xs == 2 ? (bpp + 3) / 4 * 4 : (bpp + 7) / 8 * 8;
  return 0;
}

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_conv3x3_dil_supported(int dtype, int Cin, int Cout, int kh, int kw, int stride, int pad, int dilation, int groups) {
  return dtype == TSG_BF16 && Cin > 0 && Cout > 0 && Cin % DL_KC == 0 && Cout % 64 == 0 && kh == 3 && kw == 3 &&
         stride == 1 && (dilation == 2 || dilation == 4) && pad == dilation && groups == 1;
}

int tsg_conv3x3_dil_stats_partials(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int dilation) {
  DlGeom g;
  int e = dl_geom(&g, B, H, W, Cin, Cout, dilation);
  if (e) return e;
  return Cout % DL_BN ? TSG_E_SHAPE : g.nslots;
}

int tsg_conv3x3_dil_fwd(const void* x, const void* wf, void* y, float* partial, const void* addend, int64_t B, int64_t H,
                        int64_t W, int Cin, int Cout, int dilation, void* stream) {
  if (!x || !wf || !y) return TSG_E_NULL;
  if (addend && partial) return TSG_E_SHAPE;             // statistics are of the convolution
  DlGeom g;
  int e = dl_geom(&g, B, H, W, Cin, Cout, dilation);
  if (e) return e;
  if (partial && Cout % DL_BN) return TSG_E_SHAPE;
  if (!aligned16(x) || !aligned16(wf) || !aligned16(y) || (addend && !aligned16(addend))) return TSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int grid = g.nslots * g.noct;
#define DL_GO(DD, STT)                                                                                            \
  do {                                                                                                            \
    TSG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dil3_fwd_k<DD, STT>),                              \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)DlCfg<DD>::LDS));                \
    hipLaunchKernelGGL((dil3_fwd_k<DD, STT>), dim3(grid), dim3(256), DlCfg<DD>::LDS, st, (const bf16_t*)x,        \
                       (const bf16_t*)wf, (bf16_t*)y, g, partial, (const bf16_t*)addend);                         \
  } while (0)
  if (dilation == 2) { if (partial) DL_GO(2, true); else DL_GO(2, false); }
  else { if (partial) DL_GO(4, true); else DL_GO(4, false); }
#undef DL_GO
  TSG_CHECK_LAUNCH();
  return 0;
}

size_t tsg_conv3x3_dil_wrw_ws_bytes(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int dilation) {
  DwGeom g;
  if (dw_geom(&g, B, H, W, Cin, Cout, dilation)) return 0;
  return (size_t)g.npairs * g.bpp * DW_C * DW_N * sizeof(float);
}

int tsg_conv3x3_dil_wrw(const void* x, const void* dy, float* dw, int64_t B, int64_t H, int64_t W, int Cin, int Cout,
                        int dilation, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !dw || !ws) return TSG_E_NULL;
  DwGeom g;
  int e = dw_geom(&g, B, H, W, Cin, Cout, dilation);
  if (e) return e;
  if (ws_bytes < tsg_conv3x3_dil_wrw_ws_bytes(B, H, W, Cin, Cout, dilation)) return TSG_E_WS;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(dw) || !aligned16(ws)) return TSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
#define DW_GO(DD)                                                                                                 \
  do {                                                                                                            \
    TSG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dil3_wrw_k<DD>),                                   \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)DwCfg<DD>::LDS));                \
    hipLaunchKernelGGL((dil3_wrw_k<DD>), dim3(g.npairs * g.bpp), dim3(256), DwCfg<DD>::LDS, st, (const bf16_t*)x, \
                       (const bf16_t*)dy, (float*)ws, g);                                                         \
  } while (0)
  if (dilation == 2) DW_GO(2); else DW_GO(4);
#undef DW_GO
  TSG_CHECK_LAUNCH();
  const int64_t nvec = (int64_t)Cout * 9 * Cin / 4;
  hipLaunchKernelGGL(dil3_wrw_fold_k, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, st, (const float*)ws, g, dw, nvec);
  TSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
