// Host plan of the fused separable unit (csrc/sepconv.hip): the accepted shapes, the layout of the packed constants, the
// pixel strip a block owns and the grid.  Plain C++ with no HIP include, so that the launcher, the pack-size query, the
// kernels and a host-only test program (tests/sep_geom_check.cpp) share this one definition.
//
//   y[p][co] = relu?( a[co] * sum_ci W_p[co][ci] * t[p][ci] + b[co] (+ residual[p][co]) ),   t = dw3x3(x, W_d)
//
// A block owns SEP strip of consecutive output pixels p = (b OH + oh) OW + ow and every output channel of them: no sum is
// split across blocks.  Everything here is a function of the shape alone; nothing is asked of the device.
//
// The pack (one device buffer, every section 16-byte aligned, written by one launch of sep_pack_k):
//   [0, wd_bytes)            W_d  fp32 [C_in / 8][9 taps][8]            element (cv, tap, e) = W_d[cv 8 + e][tap]
//   [ab_off, + 8 C_out)      a, b fp32 [2][C_out]                       rows 0 and 1 of tsg_bn_affine's fwd_pack
//   [wp_off, pack_bytes)     W_p, by dtype:
//     TSG_BF16: bf16 (round to nearest even) in MFMA A-fragment order [MT][NKS][64 lanes][8]:
//         element (mt, ks, lane, e) = W_p[co = mt 32 + sep_row_cout(lane & 31)][ci = ks 16 + (lane >> 5) 8 + e],
//         zero where co >= C_out or ci >= C_in (C_out = 16 and C_in % 16 == 8 are padded here, never in a tensor).
//         sep_row_cout permutes the 32 rows of a tile so that the 16 accumulator registers of a lane of
//         v_mfma_f32_32x32x16_bf16 (rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) are 16 CONSECUTIVE output channels:
//         register r of lane half h is channel mt 32 + 16 h + r, and the epilogue stores 32 contiguous bytes per lane.
//     TSG_F32:  fp32, transposed [C_in][C_out] (lanes across output channels read it coalesced), not rounded.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SEP_HD __host__ __device__
#else
#define SEP_HD
#endif

namespace tsg {

constexpr int SEP_THREADS = 256;
constexpr int SEP_CIN_MIN = 8, SEP_CIN_MAX = 256;       // multiples of 8
constexpr int SEP_COUT_MIN = 16, SEP_COUT_MAX = 256;    // multiples of 16
constexpr int SEP_TP_BIG = 64, SEP_TP_SMALL = 32;       // bf16: output pixels per block (two / one MFMA column tiles)
constexpr int SEP_TP_F32 = 16;                          // fp32 parity kernel: output pixels per block
constexpr int SEP_LDS_PAD = 8;                          // bf16 elements between the t rows of two pixels (one 16-byte slot)
constexpr int SEP_BIG_FROM = 2 * 256 * SEP_TP_BIG;      // pixel count from which 64-pixel strips still give 2 blocks per CU
constexpr int64_t SEP_ELEMS = (int64_t)1 << 40;         // an operand has at most this many elements

struct SepGeom {
  int Cin, Cout, H, W, OH, OW, stride;
  int64_t B, npix;                  // images; output pixels
  int nvec;                         // C_in / 8: 16-byte groups of a t row
  int KP, NKS;                      // C_in rounded up to the MFMA's K step of 16; K steps
  int MT;                           // 32-row tiles of output channels (C_out rounded up)
  int TP;                           // output pixels per block
  int64_t grid;                     // blocks
  size_t ab_off, wp_off, pack_bytes;
};

// rows of a 32-row A tile -> output channel within the tile (a bijection of [0, 32), see above)
SEP_HD inline int sep_row_cout(int row) { return 16 * ((row >> 2) & 1) + 4 * (row >> 3) + (row & 3); }

inline bool sep_channels_ok(int Cin, int Cout) {
  return Cin >= SEP_CIN_MIN && Cin <= SEP_CIN_MAX && Cin % 8 == 0 && Cout >= SEP_COUT_MIN && Cout <= SEP_COUT_MAX &&
         Cout % 16 == 0;
}

// the single statement of the accepted shapes (dtype and pointer alignment are the launcher's)
inline bool sep_shape_ok(int Cin, int Cout, int stride, int64_t B, int H, int W) {
  if (!sep_channels_ok(Cin, Cout) || (stride != 1 && stride != 2) || B < 1 || H < 1 || W < 1) return false;
  const int64_t hw = (int64_t)H * W;                    // < 2^62
  if (hw > SEP_ELEMS / SEP_CIN_MAX) return false;
  if (B > SEP_ELEMS / (hw * SEP_CIN_MAX)) return false; // x and y: at most 2^40 elements, so every offset fits int64
  return true;
}

// the pack's sections; bf16 = the W_p section is the fragment-order bf16 image, else the transposed fp32 matrix
inline bool sep_pack_layout(SepGeom* g, int Cin, int Cout, bool bf16) {
  if (!sep_channels_ok(Cin, Cout)) return false;
  g->Cin = Cin; g->Cout = Cout;
  g->nvec = Cin / 8;
  g->KP = (Cin + 15) / 16 * 16; g->NKS = g->KP / 16;
  g->MT = (Cout + 31) / 32;
  g->ab_off = (size_t)Cin * 9 * sizeof(float);                          // 288 bytes per 8 channels
  g->wp_off = g->ab_off + (size_t)2 * Cout * sizeof(float);             // 128 bytes per 16 channels
  g->pack_bytes = g->wp_off + (bf16 ? (size_t)g->MT * g->NKS * 64 * 8 * 2 : (size_t)Cin * Cout * sizeof(float));
  return true;
}

inline bool sep_geom(SepGeom* g, int Cin, int Cout, int stride, int64_t B, int H, int W, bool bf16) {
  if (!sep_shape_ok(Cin, Cout, stride, B, H, W) || !sep_pack_layout(g, Cin, Cout, bf16)) return false;
  g->H = H; g->W = W; g->stride = stride; g->B = B;
  g->OH = (H - 1) / stride + 1; g->OW = (W - 1) / stride + 1;
  g->npix = B * g->OH * g->OW;
  g->TP = !bf16 ? SEP_TP_F32 : (g->npix >= SEP_BIG_FROM ? SEP_TP_BIG : SEP_TP_SMALL);
  g->grid = (g->npix + g->TP - 1) / g->TP;
  return g->grid <= 0x7fffffffLL;
}

// element offset, in the bf16 W_p section, of W_p[co][ci] (co < MT 32, ci < KP)
SEP_HD inline int sep_wp_frag_index(int co, int ci, int NKS) {
  const int mt = co >> 5, c = co & 31;
  const int row = 8 * ((c & 15) >> 2) + 4 * (c >> 4) + (c & 3);          // the inverse of sep_row_cout
  const int ks = ci >> 4, lane = ((ci >> 3) & 1) * 32 + row;
  return ((mt * NKS + ks) * 64 + lane) * 8 + (ci & 7);
}

}  // namespace tsg
