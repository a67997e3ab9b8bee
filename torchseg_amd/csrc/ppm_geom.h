// Host plan of the concat-free pyramid pooling head of inference (csrc/ppmbn.hip): the accepted shapes, the cell and
// column tables of the pooled branches, the grids of the tap-table and addend launches, and the workspace.  Plain C++ with
// no HIP include, so that the launchers, the `supported` and workspace queries, the kernels and a host-only test program
// (tests/ppm_geom_check.cpp) share this one definition.
//
// The head is relu(a u + b) with u = conv3x3(cat([x, up(p_0), ..., up(p_{n-1})]), W6), up = bilinear, align_corners.  Both
// the interpolation and the convolution are linear, so the pooled half of u is formed on the pooled maps:
//
//   T[b][cell][tap][oc]  = sum over cb of W6[oc][C + s Cb + cb][tap] p_s[b][cy][cx][cb]          (stage 1, fp32)
//   E[b][oh][ow][oc]     = sum over taps (kh, kw) whose pixel (ih, iw) = (oh + kh - 1, ow + kw - 1) lies inside the map,
//                          branches s and the two rows cy and two columns cx of ih and iw, of
//                          ly_s[ih][cy] lx_s[iw][cx] T[b][cell(s, cy, cx)][kh 3 + kw][oc]       (stage 2, fp32 NHWC)
//   y                    = bf16(relu?(fma(a, conv3x3(x, W6[:, :C]) + E, b)))                     (stage 3)
//
// A tap outside the map contributes nothing: the concatenated tensor is zero-padded as a whole.
//
// Branch s is a pooled map of sh[s] x sw[s] cells.  `cell` numbers the cells of all branches in order:
// cell(s, cy, cx) = cell0[s] + cy sw[s] + cx; `col` numbers their columns: col(s, cx) = col0[s] + cx.  Stage 2 keeps the row
// stage R[kw][col][oc] of one output row and PPM_OCB output channels in LDS, which bounds the number of columns.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PPM_HD __host__ __device__
#else
#define PPM_HD
#endif

namespace tsg {

constexpr int PPM_MAXN = 4;                             // branches
constexpr int PPM_MAXCELLS = 64;                        // cells of one branch: two N tiles of 32 of the tap-table MFMA
constexpr int PPM_MAXCOLS = 32;                         // columns of all branches together (the row stage in LDS)
constexpr int PPM_OCT = 32;                             // output channels of a tap-table wave (one MFMA M tile)
constexpr int PPM_OCB = 64;                             // output channels of an addend block
constexpr int64_t PPM_MAX_OFF = 0x7fffffffLL;

struct PpmGeom {
  int B, H, W, n, Cb, Cout;
  int sh[PPM_MAXN], sw[PPM_MAXN], cell0[PPM_MAXN], col0[PPM_MAXN];
  int ncells, ncols;                                    // of all branches
  int tap_grid;                                         // B n 9 (Cout / 32) waves of stage 1
  int add_grid;                                         // B H (Cout / 64) blocks of stage 2
};

// the single statement of the accepted shapes (dtype and pointer alignment are the launchers'); H = W = 1 for a query
// that concerns the tap tables alone
inline bool ppm_geom(PpmGeom* g, int64_t B, int64_t H, int64_t W, int n, const int* sh, const int* sw, int Cb, int Cout) {
  if (!sh || !sw || B <= 0 || H <= 0 || W <= 0 || n < 1 || n > PPM_MAXN || Cb <= 0 || Cout <= 0 || Cb % 16 || Cout % 64)
    return false;
  if (B > PPM_MAX_OFF || H > PPM_MAX_OFF || W > PPM_MAX_OFF || Cb > (1 << 20) || Cout > (1 << 20)) return false;
  if (H > PPM_MAX_OFF / W || H * W > PPM_MAX_OFF / Cout) return false;       // one image of E: 32-bit offsets
  int cells = 0, cols = 0;
  for (int s = 0; s < PPM_MAXN; ++s) {
    g->sh[s] = g->sw[s] = 1;
    g->cell0[s] = g->col0[s] = 0;
  }
  for (int s = 0; s < n; ++s) {
    if (sh[s] < 1 || sw[s] < 1 || sh[s] > PPM_MAXCELLS || sw[s] > PPM_MAXCELLS || sh[s] * sw[s] > PPM_MAXCELLS) return false;
    g->sh[s] = sh[s]; g->sw[s] = sw[s];
    g->cell0[s] = cells; g->col0[s] = cols;
    cells += sh[s] * sw[s];
    cols += sw[s];
  }
  if (cols > PPM_MAXCOLS) return false;
  const int64_t tap_grid = B * n * 9 * (Cout / PPM_OCT), add_grid = B * H * (Cout / PPM_OCB);
  if (tap_grid > PPM_MAX_OFF || add_grid > PPM_MAX_OFF) return false;
  if (B * cells * 9 > PPM_MAX_OFF / Cout) return false;                       // T: 32-bit offsets
  g->B = (int)B; g->H = (int)H; g->W = (int)W; g->n = n; g->Cb = Cb; g->Cout = Cout;
  g->ncells = cells; g->ncols = cols;
  g->tap_grid = (int)tap_grid; g->add_grid = (int)add_grid;
  return true;
}

// stage 1's block -> (image, branch, tap, oc tile of 32)
PPM_HD inline void ppm_tap_block(const PpmGeom& g, int block, int* b, int* s, int* tap, int* oct) {
  const int noct = g.Cout / PPM_OCT;
  *oct = block % noct; block /= noct;
  *tap = block % 9; block /= 9;
  *s = block % g.n;
  *b = block / g.n;
}

// stage 2's block -> (image, output row, oc tile of 64)
PPM_HD inline void ppm_add_block(const PpmGeom& g, int block, int* b, int* oh, int* oct) {
  const int noct = g.Cout / PPM_OCB;
  *oct = block % noct; block /= noct;
  *oh = block % g.H;
  *b = block / g.H;
}

// column of all branches -> its branch
PPM_HD inline int ppm_col_branch(const PpmGeom& g, int col) {
  return (g.n > 1 && col >= g.col0[1]) + (g.n > 2 && col >= g.col0[2]) + (g.n > 3 && col >= g.col0[3]);
}

// bytes of T [B][ncells][9][Cout] fp32 and of E [B][H][W][Cout] fp32; E follows T in the workspace, 256-byte aligned
inline size_t ppm_t_bytes(const PpmGeom& g) { return (size_t)g.B * g.ncells * 9 * g.Cout * sizeof(float); }
inline size_t ppm_e_offset(const PpmGeom& g) { return (ppm_t_bytes(g) + 255) / 256 * 256; }
inline size_t ppm_e_bytes(const PpmGeom& g) { return (size_t)g.B * g.H * g.W * g.Cout * sizeof(float); }
inline size_t ppm_ws_bytes(const PpmGeom& g) { return ppm_e_offset(g) + ppm_e_bytes(g); }

}  // namespace tsg
