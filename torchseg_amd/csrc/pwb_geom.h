// Host plan of the fused 1x1 convolution + BatchNorm (+ residual) (+ ReLU) of inference (csrc/pwbn.hip): the accepted
// shapes, the pixel tiles, the persistent blocks and which (oc tile, pixel tile) pairs each of them walks, the row of x an
// output pixel reads, and the ONE definition of the packed filter's layout.  Plain C++ with no HIP include, so that the
// launcher, the `supported` and plan queries, the filter preparation, the kernel and a host-only test program
// (tests/pwb_geom_check.cpp) share it.
//
//   y[b][oh][ow][oc] = bf16( relu?( fma(a[oc], u, b[oc]) + float(residual[b][oh][ow][oc]) ) ),
//   u = sum over ci of w[oc][ci] * x[b][s oh][s ow][ci]   (fp32 MFMA accumulation),  OH = (H - 1) / s + 1, OW likewise
//
// is the GEMM D[oc][pixel] += W[oc][ci] X[ci][pixel] with the output pixels numbered flat, p = (b OH + oh) OW + ow.  An oc
// tile is PWB_BN = 64 output channels, a pixel tile PWB_TP = 256 consecutive p (64 per wave: two MFMA column groups of 32),
// the reduction runs in chunks of PWB_KC = 64 input channels.  A 4-wave block owns one oc tile and the pixel tiles slot,
// slot + nslots, ...; no sum is split across blocks.  Block ids map XCD-aware as in cbn_geom.h: the blocks of one slot
// (same pixels, every oc tile) have the same id modulo 8 and are adjacent in launch order, so the Cout / 64 reads of a
// pixel tile's x meet in one L2.  Everything here is a function of the shape alone.
//
// The packed filter (Cout * Cin bf16) in the order the kernel's LDS-DMA copies it and its A fragments read it:
//   wf[oc tile][chunk][ks 0..3][ocb 0..1][lane 0..63][e 0..7]
//     = W[oc tile 64 + ocb 32 + cbn_row_cout(lane & 31)][chunk 64 + pwb_lane_ci(lane >> 5, ks) + e]
// * rows: cbn_row_cout (cbn_geom.h, the one definition of that permutation) puts the 16 accumulator registers of a lane on
//   16 consecutive output channels, so the epilogue reads and writes 32 contiguous bytes per lane;
// * k order: the order of the k sum is free, and MFMA step ks of lane half h takes the 8 channels h 32 + ks 8 .. of the
//   chunk (NOT the natural ks 16 + h 8): the B operand of a lane for a whole chunk is then 64 contiguous bytes of its pixel,
//   and the two halves of a wave cover the pixel's 128-byte line.
#pragma once
#include <stdint.h>
#include "cbn_geom.h"

#define PWB_HD CBN_HD

namespace tsg {

constexpr int PWB_BN = 64;                              // output channels per block
constexpr int PWB_KC = 64;                              // input channels per chunk: four K steps of the 32x32x16 MFMA
constexpr int PWB_TP = 256;                             // output pixels per tile: 4 waves x 2 groups of 32
constexpr int PWB_BLOCKS = 512;                         // two 4-wave blocks on each of 256 compute units
constexpr int PWB_CMIN = 64, PWB_CMAX = 2048;           // channel counts: multiples of 64 in [64, 2048]
constexpr int64_t PWB_ELEMS = 0x7fffffffLL;             // an operand has at most this many elements
constexpr int PWB_FELEMS = PWB_BN * PWB_KC;             // bf16 elements of one (oc tile, chunk) slab: 8 KB
constexpr int PWB_LDS = 2 * PWB_FELEMS * 2;             // the double-buffered slab: 16,384 B

struct PwbGeom {
  int B, H, W, OH, OW, Cin, Cout, stride;
  int P;                                                // output pixels B OH OW (< 2^25: Cout >= 64)
  int ntiles, nchunks, noct, nslots;                    // pixel tiles, Cin / 64, Cout / 64, persistent blocks per oc tile
  int grid;                                             // nslots * noct
};

// the single statement of the accepted shapes and of the plan (dtype and pointer alignment are the launcher's)
inline bool pwb_geom(PwbGeom* g, int64_t B, int64_t H, int64_t W, int Cin, int Cout, int stride) {
  if (stride != 1 && stride != 2) return false;
  if (Cin < PWB_CMIN || Cin > PWB_CMAX || Cin % PWB_KC || Cout < PWB_CMIN || Cout > PWB_CMAX || Cout % PWB_BN) return false;
  if (B < 1 || H < 1 || W < 1 || B > PWB_ELEMS || H > PWB_ELEMS || W > PWB_ELEMS) return false;
  if (H > PWB_ELEMS / W || H * W > PWB_ELEMS / Cin) return false;
  if (B > PWB_ELEMS / (H * W * Cin)) return false;                          // x: B H W Cin <= 2^31 - 1
  const int64_t OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  if (B > PWB_ELEMS / (OH * OW * Cout)) return false;                       // y, residual: B OH OW Cout <= 2^31 - 1
  g->B = (int)B; g->H = (int)H; g->W = (int)W; g->OH = (int)OH; g->OW = (int)OW;
  g->Cin = Cin; g->Cout = Cout; g->stride = stride;
  g->P = (int)(B * OH * OW);
  g->ntiles = (g->P + PWB_TP - 1) / PWB_TP;
  g->nchunks = Cin / PWB_KC; g->noct = Cout / PWB_BN;
  int ns = PWB_BLOCKS / g->noct;                        // a multiple of 8 slots per oc tile (XCD mapping), at least 8
  if (ns > g->ntiles) ns = g->ntiles;
  ns = (ns + 7) / 8 * 8;
  if (ns < 8) ns = 8;
  g->nslots = ns;
  g->grid = ns * g->noct;                               // <= 512 + 7 * 32
  return true;
}

// block id -> (oc tile, slot); the block walks the pixel tiles slot, slot + nslots, ... < ntiles
PWB_HD inline void pwb_block(const PwbGeom& g, int block, int* oct, int* slot) {
  const int xcd = block & 7, jb = block >> 3;
  *oct = jb % g.noct;
  *slot = (jb / g.noct) * 8 + xcd;
}

// output pixel p (0 <= p < P) -> the row of x ([B H W] flat) it reads; row * Cin < 2^31
PWB_HD inline int pwb_row(const PwbGeom& g, int p) {
  if (g.stride == 1) return p;
  const int ohw = g.OH * g.OW, b = p / ohw, r = p - b * ohw, oh = r / g.OW, ow = r - oh * g.OW;
  return (b * g.H + g.stride * oh) * g.W + g.stride * ow;
}

// first of the 8 chunk channels that MFMA step ks (0..3) of lane half h (0..1) multiplies
PWB_HD inline int pwb_lane_ci(int half, int ks) { return half * 32 + ks * 8; }

// 16-byte vector `vec` (element offset 8 vec, 0 <= vec < Cout Cin / 8) of the packed filter holds W[*oc][*ci0 .. *ci0 + 7]
PWB_HD inline void pwb_filter_decode(int vec, int nchunks, int* oc, int* ci0) {
  const int lane = vec & 63, ocb = (vec >> 6) & 1, ks = (vec >> 7) & 3, r = vec >> 9;
  const int chunk = r % nchunks, oct = r / nchunks;
  *oc = oct * PWB_BN + ocb * 32 + cbn_row_cout(lane & 31);
  *ci0 = chunk * PWB_KC + pwb_lane_ci(lane >> 5, ks);
}

}  // namespace tsg
