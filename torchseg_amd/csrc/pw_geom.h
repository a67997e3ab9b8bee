// Host plan of the 1x1 convolutions' weight gradient (csrc/pwwgrad.hip): which shapes are accepted, the channel tiles, the
// number S of pixel slices, the pixel range of each slice and the grid.  Plain C++ with no HIP include, so that the launcher,
// the workspace query, the slice query and a host-only test program (tests/pw_geom_check.cpp) share this one definition.
//
//   dw[co][ci] = sum_p dy[p][co] * x[row(p)][ci],  p = (b OH + oh) OW + ow,  row(p) = (b H + s oh) W + s ow
//
// is a GEMM with M = C_out, N = C_in, K = P = B OH OW.  A block owns one (C_out tile, C_in tile, pixel slice) triple; the
// pixel axis is cut in CHUNKS of PW_KC pixels (what a block stages in LDS at a time) and a slice is `cps` consecutive chunks.
// S depends on (P, C_out, C_in) only: the CU count is the compile-time constant PW_CUS and nothing is asked of the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PW_HD __host__ __device__          // the kernel maps its block id and slice with the functions the host uses
#else
#define PW_HD
#endif

namespace tsg {

constexpr int PW_KC = 64;                     // pixels per chunk: four K steps of v_mfma_f32_32x32x16_bf16
constexpr int PW_CUS = 256;                   // compute units of the MI355X
constexpr int PW_BLOCKS = 2 * PW_CUS;         // blocks wanted: two 4-wave blocks are resident per CU
constexpr int PW_MIN_CHUNKS = 4;              // a slice is at least this long (256 pixels) unless P itself is shorter
constexpr int PW_CMIN = 64, PW_CMAX = 2048;   // channel counts: multiples of 64 in [64, 2048]
constexpr int64_t PW_ELEMS = 0x7fffffffLL;    // an operand has at most this many elements: 32-bit byte offsets hold

struct PwGeom {
  int Cin, Cout, H, W, OH, OW, stride;
  int64_t B, P;                               // images; output pixels = the reduction length
  int bm, bn;                                 // C_out / C_in channels per block tile: 128 where that divides, else 64
  int tiles_m, tiles_n, tiles;                // C_out tiles, C_in tiles, their product
  int64_t nchunks, cps;                       // chunks of PW_KC pixels in P; chunks per slice
  int S;                                      // slices: every one holds at least one pixel, all but the last cps chunks
  int64_t grid;                               // blocks launched: tiles * (S rounded up to the 8 XCDs)
};

// the single statement of the accepted shapes (dtype and pointer alignment are the launcher's)
inline bool pw_shape_ok(int Cin, int Cout, int64_t B, int H, int W, int stride) {
  if (stride != 1 && stride != 2) return false;
  if (Cin < PW_CMIN || Cin > PW_CMAX || Cin % 64 || Cout < PW_CMIN || Cout > PW_CMAX || Cout % 64) return false;
  if (B < 1 || H < 1 || W < 1) return false;
  const int64_t hw = (int64_t)H * W;                          // < 2^62
  if (hw > PW_ELEMS / Cin) return false;
  if (B > PW_ELEMS / (hw * Cin)) return false;                // x: B H W C_in <= 2^31 - 1
  const int64_t ohw = (int64_t)((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  if (B > PW_ELEMS / (ohw * Cout)) return false;              // dy: B OH OW C_out <= 2^31 - 1
  return true;
}

inline bool pw_geom(PwGeom* g, int Cin, int Cout, int64_t B, int H, int W, int stride) {
  if (!pw_shape_ok(Cin, Cout, B, H, W, stride)) return false;
  g->Cin = Cin; g->Cout = Cout; g->H = H; g->W = W; g->stride = stride; g->B = B;
  g->OH = (H - 1) / stride + 1; g->OW = (W - 1) / stride + 1;
  g->P = B * g->OH * g->OW;                                   // < 2^25 (C_out >= 64)
  g->bm = Cout % 128 ? 64 : 128; g->bn = Cin % 128 ? 64 : 128;
  g->tiles_m = Cout / g->bm; g->tiles_n = Cin / g->bn; g->tiles = g->tiles_m * g->tiles_n;      // <= 32 * 32
  g->nchunks = (g->P + PW_KC - 1) / PW_KC;
  int64_t want = (PW_BLOCKS + g->tiles - 1) / g->tiles;       // slices that fill the chip
  const int64_t most = g->nchunks / PW_MIN_CHUNKS;            // slices of at least PW_MIN_CHUNKS chunks
  if (want > most) want = most;
  if (want < 1) want = 1;
  g->cps = (g->nchunks + want - 1) / want;
  g->S = (int)((g->nchunks + g->cps - 1) / g->cps);           // no empty slice
  g->grid = (int64_t)g->tiles * ((g->S + 7) / 8 * 8);         // <= 1024 * 512
  return true;
}

// pixels [*p0, *p1) of slice s, 0 <= s < S
PW_HD inline void pw_slice_range(const PwGeom& g, int s, int64_t* p0, int64_t* p1) {
  *p0 = (int64_t)s * g.cps * PW_KC;
  const int64_t e = *p0 + g.cps * PW_KC;
  *p1 = e < g.P ? e : g.P;
}

// (C_out tile, C_in tile, slice) of block `id` of the grid; slice >= S: the block has nothing to do.  Consecutive ids go
// round-robin over the 8 XCDs, so the tiles of one slice, which read the same pixels, are ids 8 apart: one XCD, one L2.
PW_HD inline void pw_block(const PwGeom& g, int64_t id, int* tm, int* tn, int* slice) {
  const int xcd = (int)(id & 7);
  const int64_t jb = id >> 3;
  const int tile = (int)(jb % g.tiles);
  *slice = (int)(jb / g.tiles) * 8 + xcd;
  *tm = tile / g.tiles_n; *tn = tile % g.tiles_n;
}

// ---- a pixel's byte offsets in x and dy, and the step to the same position of the next chunk.  The offsets are exact for
// every pixel < P (an operand has < 2^32 bytes) and are computed modulo 2^32: unsigned arithmetic, no carry is lost.
// Walking PW_KC pixels on is d_b images + d_oh output rows + d_ow output columns; x moves by a constant plus one
// correction when the column wraps into the next row and one when the row wraps into the next image.
struct PwSteps { int d_ow, d_oh; uint32_t xstep, fix_ow, fix_oh, dstep; };
struct PwPix { int p, ow, oh; uint32_t xo, dyo; };

PW_HD inline PwSteps pw_steps(const PwGeom& g) {
  const uint32_t st = (uint32_t)g.stride, rowb = (uint32_t)g.Cin * 2u, H = (uint32_t)g.H, W = (uint32_t)g.W;
  PwSteps s;
  s.d_ow = PW_KC % g.OW; s.d_oh = (PW_KC / g.OW) % g.OH;
  const uint32_t d_b = (uint32_t)(PW_KC / g.OW / g.OH);
  s.xstep = ((d_b * H + st * (uint32_t)s.d_oh) * W + st * (uint32_t)s.d_ow) * rowb;
  s.fix_ow = st * (uint32_t)(g.W - g.OW) * rowb;                       // ow -= OW, oh += 1
  s.fix_oh = (H - st * (uint32_t)g.OH) * W * rowb;                     // oh -= OH, b += 1
  s.dstep = (uint32_t)PW_KC * (uint32_t)g.Cout * 2u;
  return s;
}

PW_HD inline PwPix pw_pix(const PwGeom& g, int p) {
  const uint32_t st = (uint32_t)g.stride;
  const int b = (int)(p / ((int64_t)g.OH * g.OW)), r = (int)(p - b * ((int64_t)g.OH * g.OW));
  PwPix q;
  q.p = p; q.oh = r / g.OW; q.ow = r - q.oh * g.OW;
  q.xo = (((uint32_t)b * (uint32_t)g.H + st * (uint32_t)q.oh) * (uint32_t)g.W + st * (uint32_t)q.ow) * ((uint32_t)g.Cin * 2u);
  q.dyo = (uint32_t)p * ((uint32_t)g.Cout * 2u);
  return q;
}

PW_HD inline void pw_advance(const PwGeom& g, const PwSteps& s, PwPix* q) {
  q->p += PW_KC; q->dyo += s.dstep; q->xo += s.xstep;
  q->ow += s.d_ow; if (q->ow >= g.OW) { q->ow -= g.OW; ++q->oh; q->xo += s.fix_ow; }
  q->oh += s.d_oh; if (q->oh >= g.OH) { q->oh -= g.OH; q->xo += s.fix_oh; }
}

inline uint64_t pw_ws_bytes(const PwGeom& g) {
  return g.S > 1 ? (uint64_t)g.S * g.Cout * g.Cin * sizeof(float) : 0;     // <= 512 * 2^22 * 4
}

}  // namespace tsg
