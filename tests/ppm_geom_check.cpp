// Host-only check of torchseg_amd/csrc/ppm_geom.h, the plan of the concat-free pyramid pooling head (built and run by
// tests/test_ppmbn_cpu.py with ASan + UBSan; UBSan stops on any signed overflow of an intermediate).  For a sweep of shapes
// and pooled maps: the cell and column tables tile [0, ncells) and [0, ncols) without gap or overlap, every column decodes
// to its branch, every block id of the tap launch decodes to an (image, branch, tap, oc tile) of its own and every T element
// is owned by exactly one lane of one block, every block id of the addend launch decodes to an (image, row, oc tile) of
// its own and every E element is owned by exactly one block, the row stage fits its LDS image, the workspace holds T and E
// without overlap at 16-byte-aligned offsets, and the limits of the accepted set refuse what lies outside.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>
#include "../torchseg_amd/csrc/ppm_geom.h"

using namespace tsg;

static int g_fail = 0;
static long g_checks = 0;
static char g_what[200];
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { if (++g_fail < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_what); } \
  } while (0)

static void check_shape(int64_t B, int64_t H, int64_t W, int n, const int* sh, const int* sw, int Cb, int Cout, bool elements) {
  snprintf(g_what, sizeof g_what, "B %lld H %lld W %lld n %d first map %dx%d Cb %d Cout %d", (long long)B, (long long)H,
           (long long)W, n, sh[0], sw[0], Cb, Cout);
  PpmGeom g;
  if (!ppm_geom(&g, B, H, W, n, sh, sw, Cb, Cout)) { CHECK(false); return; }
  CHECK(g.B == B && g.H == H && g.W == W && g.n == n && g.Cb == Cb && g.Cout == Cout);
  int cells = 0, cols = 0;
  for (int s = 0; s < n; ++s) {
    CHECK(g.sh[s] == sh[s] && g.sw[s] == sw[s] && g.cell0[s] == cells && g.col0[s] == cols);
    CHECK(sh[s] * sw[s] <= PPM_MAXCELLS);
    for (int cx = 0; cx < sw[s]; ++cx) CHECK(ppm_col_branch(g, cols + cx) == s);
    cells += sh[s] * sw[s];
    cols += sw[s];
  }
  for (int s = n; s < PPM_MAXN; ++s) CHECK(g.sh[s] == 1 && g.sw[s] == 1);    // what the kernels' selects may touch
  CHECK(g.ncells == cells && g.ncols == cols && cols <= PPM_MAXCOLS);
  CHECK(3 * g.ncols * (PPM_OCB / 4) <= 3 * PPM_MAXCOLS * (PPM_OCB / 4));      // the row stage's LDS image
  CHECK((int64_t)g.tap_grid == B * n * 9 * (Cout / PPM_OCT) && (int64_t)g.add_grid == B * H * (Cout / PPM_OCB));
  // the workspace: T at 0, E behind it, both 16-byte aligned, no overlap
  CHECK(ppm_t_bytes(g) == (size_t)B * cells * 9 * Cout * 4 && ppm_e_offset(g) >= ppm_t_bytes(g) && ppm_e_offset(g) % 256 == 0);
  CHECK(ppm_e_offset(g) - ppm_t_bytes(g) < 256 && ppm_ws_bytes(g) == ppm_e_offset(g) + (size_t)B * H * W * Cout * 4);
  CHECK((int64_t)B * cells * 9 * Cout <= PPM_MAX_OFF && H * W * Cout <= PPM_MAX_OFF);
  if (!elements) return;
  // stage 1: block -> (b, s, tap, oct) is a bijection, and the lanes' stores cover T exactly once
  std::vector<unsigned char> t((size_t)B * cells * 9 * Cout, 0);
  std::vector<unsigned char> seen((size_t)g.tap_grid, 0);
  for (int blk = 0; blk < g.tap_grid; ++blk) {
    int b, s, tap, oct;
    ppm_tap_block(g, blk, &b, &s, &tap, &oct);
    CHECK(b >= 0 && b < B && s >= 0 && s < n && tap >= 0 && tap < 9 && oct >= 0 && oct < Cout / PPM_OCT);
    if (b < 0 || b >= B || s < 0 || s >= n || tap < 0 || tap >= 9 || oct < 0 || oct >= Cout / PPM_OCT) continue;
    const size_t id = (((size_t)b * n + s) * 9 + tap) * (Cout / PPM_OCT) + oct;
    CHECK(seen[id] == 0);
    seen[id] = 1;
    const int ncell = g.sh[s] * g.sw[s];
    for (int lane = 0; lane < 64; ++lane)
      for (int nt = 0; nt < 2; ++nt) {
        const int cell = (lane & 31) + 32 * nt;
        if (cell >= ncell) continue;                                           // the kernel's store predicate
        for (int r = 0; r < 16; ++r) {
          const int oc = oct * PPM_OCT + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
          unsigned char& e = t[(((size_t)b * cells + g.cell0[s] + cell) * 9 + tap) * Cout + oc];
          CHECK(e == 0);
          e = 1;
        }
      }
  }
  for (unsigned char e : t) CHECK(e == 1);
  // stage 2: block -> (b, oh, oct) is a bijection onto the rows of E
  std::vector<unsigned char> rows((size_t)g.add_grid, 0);
  for (int blk = 0; blk < g.add_grid; ++blk) {
    int b, oh, oct;
    ppm_add_block(g, blk, &b, &oh, &oct);
    CHECK(b >= 0 && b < B && oh >= 0 && oh < H && oct >= 0 && oct < Cout / PPM_OCB);
    if (b < 0 || b >= B || oh < 0 || oh >= H || oct < 0 || oct >= Cout / PPM_OCB) continue;
    unsigned char& e = rows[((size_t)b * H + oh) * (Cout / PPM_OCB) + oct];
    CHECK(e == 0);
    e = 1;
  }
  for (unsigned char e : rows) CHECK(e == 1);
}

static void check_refused(int64_t B, int64_t H, int64_t W, int n, const int* sh, const int* sw, int Cb, int Cout) {
  snprintf(g_what, sizeof g_what, "refuse B %lld H %lld W %lld n %d Cb %d Cout %d", (long long)B, (long long)H, (long long)W, n,
           Cb, Cout);
  PpmGeom g;
  CHECK(!ppm_geom(&g, B, H, W, n, sh, sw, Cb, Cout));
}

int main() {
  const int std4[4] = {1, 2, 3, 6};
  const int rh[2] = {2, 6}, rw[2] = {3, 4}, rw5[2] = {3, 5};
  const int one[1] = {8}, wide_h[1] = {2}, wide_w[1] = {32};
  // the GPU test's shapes, PSPNet's heads at 480 x 480, 768 x 1536 and 1024 x 2048, a batch
  check_shape(1, 6, 7, 4, std4, std4, 16, 64, true);
  check_shape(2, 8, 32, 4, std4, std4, 16, 64, true);
  check_shape(1, 9, 33, 4, std4, std4, 32, 128, true);
  check_shape(1, 17, 40, 2, rh, rw, 16, 192, true);
  check_shape(1, 72, 256, 4, std4, std4, 16, 512, true);
  check_shape(1, 17, 33, 2, rh, rw5, 32, 64, true);
  check_shape(1, 60, 60, 4, std4, std4, 512, 512, true);
  check_shape(1, 96, 192, 4, std4, std4, 512, 512, false);
  check_shape(1, 128, 256, 4, std4, std4, 512, 512, false);
  check_shape(16, 96, 192, 4, std4, std4, 512, 512, false);
  check_shape(3, 5, 5, 1, one, one, 16, 64, true);                 // one branch of 64 cells: both N tiles
  check_shape(1, 4, 40, 1, wide_h, wide_w, 16, 64, true);          // 32 columns: the whole LDS image
  for (int n = 1; n <= 4; ++n)
    for (int H : {1, 2, 7})
      for (int W : {1, 3, 33}) check_shape(2, H, W, n, std4, std4, 48, 192, true);
  check_shape(1, 4096, 4096, 4, std4, std4, 16, 64, false);        // 2^30 elements per image of E
  check_shape(1, 1, 33554431, 4, std4, std4, 16, 64, false);

  check_refused(1, 8, 8, 0, std4, std4, 16, 64);
  check_refused(1, 8, 8, 5, std4, std4, 16, 64);
  check_refused(1, 8, 8, -1, std4, std4, 16, 64);
  check_refused(1, 8, 8, 4, std4, std4, 24, 64);
  check_refused(1, 8, 8, 4, std4, std4, 16, 96);
  check_refused(1, 8, 8, 4, std4, std4, 0, 64);
  check_refused(1, 8, 8, 4, std4, std4, 16, 0);
  check_refused(0, 8, 8, 4, std4, std4, 16, 64);
  check_refused(1, 0, 8, 4, std4, std4, 16, 64);
  check_refused(1, 8, 0, 4, std4, std4, 16, 64);
  check_refused(1, 8, 8, 4, nullptr, std4, 16, 64);
  check_refused(1, 8, 8, 4, std4, nullptr, 16, 64);
  const int nine[1] = {9}, zero[1] = {0}, neg[1] = {-3}, w33[1] = {33}, h1[1] = {1}, huge[1] = {65536};
  check_refused(1, 8, 8, 1, nine, nine, 16, 64);                   // 81 cells
  check_refused(1, 8, 8, 1, zero, one, 16, 64);
  check_refused(1, 8, 8, 1, one, neg, 16, 64);
  check_refused(1, 8, 8, 1, h1, w33, 16, 64);                      // 33 columns
  check_refused(1, 8, 8, 1, huge, huge, 16, 64);                   // the product would overflow an int
  const int w16[3] = {16, 16, 1}, h2[3] = {2, 2, 1};
  check_refused(1, 8, 8, 3, h2, w16, 16, 64);                      // 33 columns together
  check_refused(1, 8192, 8192, 4, std4, std4, 16, 64);             // 2^32 elements per image of E
  check_refused(1, 1, 33554432, 4, std4, std4, 16, 64);
  check_refused(INT64_MAX, 8, 8, 4, std4, std4, 16, 64);
  check_refused(1, INT64_MAX, INT64_MAX, 4, std4, std4, 16, 64);
  check_refused(2147483647, 8, 8, 4, std4, std4, 16, 64);          // the grids
  check_refused(1000000, 1, 1, 4, std4, std4, 16, 512);            // T beyond 2^31 elements
  check_refused(1, 8, 8, 4, std4, std4, 1 << 21, 64);

  if (g_fail) { fprintf(stderr, "%d of %ld checks FAILED\n", g_fail, g_checks); return 1; }
  printf("%ld checks passed\n", g_checks);
  return 0;
}
