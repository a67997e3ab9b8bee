// Host plan of the fused stride-2 3x3 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/s2bn.hip): the
// accepted shapes, the output size, the pixel tiles over the OUTPUT, the persistent blocks and which tiles each of them
// walks, the input patch of a tile with its two LDS planes, and the offset limits.  Plain C++ with no HIP include, so that
// the launcher, the `supported` and plan queries, the kernel and a host-only test program (tests/s2b_geom_check.cpp) share
// this one definition.  cbn_geom.h (chunk size, oc tile, row permutation of the prepared filter) is used as it is.
//
//   y[b][oh][ow][oc] = bf16( relu?( fma(a[oc], u, b[oc]) + float(residual[b][oh][ow][oc]) ) ),
//   u = sum over (kh, kw, ci) of w[oc][kh][kw][ci] * x[b][2 oh + kh - 1][2 ow + kw - 1][ci]   (fp32 MFMA accumulation)
//   OH = (H + 1) / 2, OW = (W + 1) / 2   (kernel 3, stride 2, padding 1; H, W are the input's)
//
// An oc tile is CBN_BN = 64 output channels, a pixel tile S2B_TH x S2B_TW = 4 x 32 OUTPUT pixels of one image, tile index
// = (b tiles_h + th) tiles_w + tw.  A 4-wave block owns one oc tile and the pixel tiles slot, slot + nslots, ...; no sum is
// split across blocks.  Block ids map XCD-aware: the blocks of one slot (same pixels, every oc tile) have the same id
// modulo 8.  Everything here is a function of the shape alone.
//
// The patch of a tile at (oh0, ow0) is S2B_PH x S2B_PW = 9 x 65 input pixels: patch row pr is input row 2 oh0 - 1 + pr,
// patch column pc is input column 2 ow0 - 1 + pc, so tap (kh, kw) of tile pixel (r, p) is patch pixel (2 r + kh, 2 p + kw).
// LDS holds the patch as two planes: the even patch columns (33 per row) and the odd ones (32 per row); the 32 pixels p of
// a B fragment are then consecutive pixels of one plane for every kw (kw = 0: even plane at p, kw = 1: odd plane at p,
// kw = 2: even plane at p + 1).
#pragma once
#include "cbn_geom.h"

namespace tsg {

constexpr int S2B_TH = 4, S2B_TW = 32;                  // output pixels of a tile
constexpr int S2B_PH = 2 * S2B_TH + 1;                  // 9 patch rows
constexpr int S2B_PW = 2 * S2B_TW + 1;                  // 65 patch columns
constexpr int S2B_EW = S2B_TW + 1, S2B_DW = S2B_TW;     // columns of a row of the even / odd plane
constexpr int S2B_ODD0 = S2B_PH * S2B_EW;               // first pixel of the odd plane: 297
constexpr int S2B_NPX = S2B_PH * S2B_PW;                // 585 patch pixels
constexpr int S2B_BLOCKS = 512;                         // two 4-wave blocks on each of 256 compute units

struct S2bGeom {
  int B, H, W, Cin, Cout;
  int OH, OW;
  int tiles_h, tiles_w, ntiles;                         // pixel tiles over the output (per oc tile)
  int nchunks, noct, nslots;                            // Cin / 16, Cout / 64, persistent blocks per oc tile
  int grid;                                             // nslots * noct
};

// the single statement of the accepted shapes and of the plan (dtype and pointer alignment are the launcher's)
inline bool s2b_geom(S2bGeom* g, int64_t B, int64_t H, int64_t W, int Cin, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % CBN_KC || Cout % CBN_BN) return false;
  if (B > CBN_MAX_OFF || H > CBN_MAX_OFF || W > CBN_MAX_OFF) return false;
  if (H > CBN_MAX_OFF / W || H * W > CBN_MAX_OFF / Cin) return false;       // one image of x: 32-bit element offsets
  const int64_t OH = (H + 1) / 2, OW = (W + 1) / 2;
  if (OH * OW > CBN_MAX_OFF / Cout) return false;                           // one image of y / the residual (OH OW <= H W)
  const int64_t th = (OH + S2B_TH - 1) / S2B_TH, tw = (OW + S2B_TW - 1) / S2B_TW;
  if (B > CBN_MAX_OFF / (th * tw)) return false;                            // th tw <= H W < 2^31
  g->B = (int)B; g->H = (int)H; g->W = (int)W; g->Cin = Cin; g->Cout = Cout;
  g->OH = (int)OH; g->OW = (int)OW;
  g->tiles_h = (int)th; g->tiles_w = (int)tw; g->ntiles = (int)(B * th * tw);
  g->nchunks = Cin / CBN_KC; g->noct = Cout / CBN_BN;
  int64_t ns = S2B_BLOCKS / g->noct;                    // a multiple of 8 slots per oc tile (XCD mapping), at least 8
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
CBN_HD inline void s2b_block(const S2bGeom& g, int block, int* oct, int* slot) {
  const int xcd = block & 7, jb = block >> 3;
  *oct = jb % g.noct;
  *slot = (jb / g.noct) * 8 + xcd;
}

// tile index -> image and the tile's first output pixel
CBN_HD inline void s2b_tile(const S2bGeom& g, int tile, int* b, int* oh0, int* ow0) {
  *ow0 = (tile % g.tiles_w) * S2B_TW;
  *oh0 = ((tile / g.tiles_w) % g.tiles_h) * S2B_TH;
  *b = tile / (g.tiles_w * g.tiles_h);
}

// patch pixel (pr, pc) of the tile at (oh0, ow0) -> input row and column (may lie outside the image: zero padding)
CBN_HD inline int s2b_patch_ih(int oh0, int pr) { return 2 * oh0 - 1 + pr; }
CBN_HD inline int s2b_patch_iw(int ow0, int pc) { return 2 * ow0 - 1 + pc; }

// patch pixel (pr, pc) -> pixel index in the LDS image of a chunk (even plane first)
CBN_HD inline int s2b_patch_lds(int pr, int pc) {
  return (pc & 1) ? S2B_ODD0 + pr * S2B_DW + (pc >> 1) : pr * S2B_EW + (pc >> 1);
}

// tap (kh, kw) of tile pixel (r, p) -> pixel index in the LDS image: what a lane of the B fragment reads
CBN_HD inline int s2b_tap_lds(int r, int p, int kh, int kw) {
  const int pr = 2 * r + kh;
  return kw == 1 ? S2B_ODD0 + pr * S2B_DW + p : pr * S2B_EW + p + (kw >> 1);
}

}  // namespace tsg
