// Host plan of the fused 3x3 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/convbn.hip): the accepted
// shapes, the pixel tiles, the persistent blocks and which tiles each of them walks, the row permutation of the prepared
// filter, and the offset limits.  Plain C++ with no HIP include, so that the launcher, the `supported` and plan queries,
// the kernel and a host-only test program (tests/cbn_geom_check.cpp) share this one definition.
//
//   y[b][oh][ow][oc] = bf16( relu?( fma(a[oc], u, b[oc]) + float(residual[b][oh][ow][oc]) ) ),
//   u = sum over (kh, kw, ci) of w[oc][kh][kw][ci] * x[b][oh + kh - 1][ow + kw - 1][ci]   (fp32 MFMA accumulation)
//
// The tiling is conv3g_fwd_k's at 64 output channels per block: an oc tile is CBN_BN = 64 output channels, a pixel tile
// CBN_TH x CBN_TW = 8 x 32 output pixels of one image, tile index = (b tiles_h + th) tiles_w + tw.  A 4-wave block owns one
// oc tile and the pixel tiles slot, slot + nslots, ...; no sum is split across blocks.  Block ids map XCD-aware: the
// blocks of one slot (same pixels, every oc tile) have the same id modulo 8.  Everything here is a function of the shape
// alone; nothing is asked of the device and nothing is read from the environment.
//
// The filter: tsg_conv3x3_gen_prep_filter(w', TSG_F32, ..., mode 0, BN 64) of the weight whose output channels were
// permuted inside each group of 32:  w'[32 t + m] = w[32 t + cbn_row_cout(m)].  Row m of a 32-row MFMA A tile then holds
// output channel cbn_row_cout(m), and the 16 accumulator registers of a lane of v_mfma_f32_32x32x16_bf16 (rows
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) are 16 CONSECUTIVE output channels: register r of lane half h is channel
// 32 t + 16 h + r, so the epilogue reads and writes 32 contiguous bytes per lane without a staging image.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CBN_HD __host__ __device__
#else
#define CBN_HD
#endif

namespace tsg {

constexpr int CBN_TH = 8, CBN_TW = 32;                  // output pixels of a tile
constexpr int CBN_KC = 16;                              // input channels per chunk
constexpr int CBN_BN = 64;                              // output channels per block
constexpr int CBN_BLOCKS = 512;                         // two 4-wave blocks on each of 256 compute units
constexpr int64_t CBN_MAX_OFF = 0x7fffffffLL;           // element offsets inside one image of x, y and the residual

struct CbnGeom {
  int B, H, W, Cin, Cout;
  int tiles_h, tiles_w, ntiles;                         // pixel tiles (per oc tile)
  int nchunks, noct, nslots;                            // Cin / 16, Cout / 64, persistent blocks per oc tile
  int grid;                                             // nslots * noct
};

// row of a 32-row A tile -> output channel within the tile (a bijection of [0, 32))
CBN_HD inline int cbn_row_cout(int row) { return 16 * ((row >> 2) & 1) + 4 * (row >> 3) + (row & 3); }

// the single statement of the accepted shapes and of the plan (dtype and pointer alignment are the launcher's)
inline bool cbn_geom(CbnGeom* g, int64_t B, int64_t H, int64_t W, int Cin, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % CBN_KC || Cout % CBN_BN) return false;
  if (B > CBN_MAX_OFF || H > CBN_MAX_OFF || W > CBN_MAX_OFF) return false;
  const int64_t cmax = Cin > Cout ? Cin : Cout;
  if (H > CBN_MAX_OFF / W || H * W > CBN_MAX_OFF / cmax) return false;      // one image of either operand: 32-bit offsets
  const int64_t th = (H + CBN_TH - 1) / CBN_TH, tw = (W + CBN_TW - 1) / CBN_TW;
  if (B > CBN_MAX_OFF / (th * tw)) return false;                            // th tw <= H W < 2^31
  g->B = (int)B; g->H = (int)H; g->W = (int)W; g->Cin = Cin; g->Cout = Cout;
  g->tiles_h = (int)th; g->tiles_w = (int)tw; g->ntiles = (int)(B * th * tw);
  g->nchunks = Cin / CBN_KC; g->noct = Cout / CBN_BN;
  int64_t ns = CBN_BLOCKS / g->noct;                    // a multiple of 8 slots per oc tile (XCD mapping), at least 8
  if (ns > g->ntiles) ns = g->ntiles;
  ns = (ns + 7) / 8 * 8;
  if (ns < 8) ns = 8;
  g->nslots = (int)ns;
  const int64_t grid = ns * g->noct;
  if (grid > CBN_MAX_OFF) return false;
  g->grid = (int)grid;
  return true;
}

// block id -> (oc tile, slot)
CBN_HD inline void cbn_block(const CbnGeom& g, int block, int* oct, int* slot) {
  const int xcd = block & 7, jb = block >> 3;
  *oct = jb % g.noct;
  *slot = (jb / g.noct) * 8 + xcd;
}

// tile index -> image and the tile's first output pixel
CBN_HD inline void cbn_tile(const CbnGeom& g, int tile, int* b, int* oh0, int* ow0) {
  *ow0 = (tile % g.tiles_w) * CBN_TW;
  *oh0 = ((tile / g.tiles_w) % g.tiles_h) * CBN_TH;
  *b = tile / (g.tiles_w * g.tiles_h);
}

}  // namespace tsg
