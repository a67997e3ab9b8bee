// Host-only check of torchseg_amd/csrc/cbn_geom.h, the plan of the fused 3x3 convolution + BatchNorm kernel (built and
// run by tests/test_convbn_cpu.py with ASan + UBSan; UBSan stops on any signed overflow of an intermediate).
// cbn_row_cout is a bijection whose image puts the 16 accumulator rows of either lane half on 16 consecutive channels.  For
// a sweep of shapes: every block id decodes to an (oc tile, slot) of its own, every output pixel of every oc tile is owned
// by exactly one (block, tile step), the tiles of a block come from the walk slot, slot + nslots, ..., and the largest
// element offset any lane forms inside one image of x, y, the residual, and inside the filter, stays below 2^31.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../torchseg_amd/csrc/cbn_geom.h"

using namespace tsg;

static int g_fail = 0;
static long g_checks = 0;
static char g_what[160];
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { if (++g_fail < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_what); } \
  } while (0)

// pixels: also count every output pixel (small shapes); otherwise the tiles only
static void check_shape(int64_t B, int64_t H, int64_t W, int Cin, int Cout, bool pixels) {
  snprintf(g_what, sizeof g_what, "B %lld H %lld W %lld Cin %d Cout %d", (long long)B, (long long)H, (long long)W, Cin, Cout);
  CbnGeom g;
  if (!cbn_geom(&g, B, H, W, Cin, Cout)) { CHECK(false); return; }
  CHECK(g.B == B && g.H == H && g.W == W && g.Cin == Cin && g.Cout == Cout);
  CHECK(g.tiles_h == (H + 7) / 8 && g.tiles_w == (W + 31) / 32 && (int64_t)g.ntiles == B * g.tiles_h * g.tiles_w);
  CHECK(g.nchunks * CBN_KC == Cin && g.noct * CBN_BN == Cout);
  CHECK(g.nslots >= 8 && g.nslots % 8 == 0 && g.grid == g.nslots * g.noct);
  CHECK(g.nslots <= (g.ntiles + 7) / 8 * 8 || g.nslots == 8);             // no more than 7 idle slots beyond the tiles
  CHECK((int64_t)g.nslots * g.noct <= CBN_BLOCKS + 8 * g.noct || g.nslots == 8);
  // offsets: one image of either operand, and the filter (int64 in the kernel; stated here for the 32-bit claim)
  const int64_t cmax = Cin > Cout ? Cin : Cout;
  CHECK(((H - 1) * W + (W - 1)) * cmax + cmax <= CBN_MAX_OFF);
  CHECK(B * H * W <= INT64_MAX / cmax);                                     // the batch offset fits int64
  // block -> (oc tile, slot) is a bijection of [0, grid) onto [0, noct) x [0, nslots)
  std::vector<unsigned char> seen((size_t)g.grid, 0);
  std::vector<unsigned char> tile_owner((size_t)g.noct * g.ntiles, 0);
  std::vector<unsigned char> px;
  if (pixels) px.assign((size_t)g.noct * B * H * W, 0);
  for (int blk = 0; blk < g.grid; ++blk) {
    int oct, slot;
    cbn_block(g, blk, &oct, &slot);
    CHECK(oct >= 0 && oct < g.noct && slot >= 0 && slot < g.nslots);
    if (oct < 0 || oct >= g.noct || slot < 0 || slot >= g.nslots) continue;
    CHECK((slot & 7) == (blk & 7));                                         // the blocks of a slot share an XCD
    const size_t id = (size_t)oct * g.nslots + slot;
    CHECK(seen[id] == 0);
    seen[id] = 1;
    for (int64_t tile = slot; tile < g.ntiles; tile += g.nslots) {
      CHECK(tile_owner[(size_t)oct * g.ntiles + tile] == 0);
      tile_owner[(size_t)oct * g.ntiles + tile] = 1;
      int b, oh0, ow0;
      cbn_tile(g, (int)tile, &b, &oh0, &ow0);
      CHECK(b >= 0 && b < B && oh0 >= 0 && oh0 < H && ow0 >= 0 && ow0 < W && oh0 % CBN_TH == 0 && ow0 % CBN_TW == 0);
      if (!pixels || b < 0 || b >= B) continue;
      for (int r = 0; r < CBN_TH; ++r)
        for (int c = 0; c < CBN_TW; ++c) {
          const int64_t oh = oh0 + r, ow = ow0 + c;
          if (oh >= H || ow >= W) continue;                                 // the kernel's store predicate
          unsigned char& n = px[((size_t)oct * B + b) * H * W + oh * W + ow];
          CHECK(n == 0);
          n = 1;
        }
    }
  }
  for (unsigned char s : tile_owner) CHECK(s == 1);
  for (unsigned char s : px) CHECK(s == 1);
}

static void check_refused(int64_t B, int64_t H, int64_t W, int Cin, int Cout) {
  snprintf(g_what, sizeof g_what, "refuse B %lld H %lld W %lld Cin %d Cout %d", (long long)B, (long long)H, (long long)W, Cin, Cout);
  CbnGeom g;
  CHECK(!cbn_geom(&g, B, H, W, Cin, Cout));
}

int main() {
  snprintf(g_what, sizeof g_what, "cbn_row_cout");
  unsigned seen = 0;
  for (int row = 0; row < 32; ++row) {
    const int c = cbn_row_cout(row);
    CHECK(c >= 0 && c < 32 && !((seen >> c) & 1u));
    seen |= 1u << c;
  }
  CHECK(seen == 0xffffffffu);
  for (int h = 0; h < 2; ++h)
    for (int r = 0; r < 16; ++r)          // accumulator register r of lane half h: row (r & 3) + 8 (r >> 2) + 4 h
      CHECK(cbn_row_cout((r & 3) + 8 * (r >> 2) + 4 * h) == 16 * h + r);

  const int sizes[] = {1, 7, 8, 9, 31, 32, 33, 72, 256};
  const int couts[] = {64, 192, 512};
  for (int H : sizes)
    for (int W : sizes)
      for (int Cout : couts) {
        check_shape(1, H, W, 16, Cout, true);
        check_shape(3, H, W, 48, Cout, H * W <= 72 * 72);
      }
  // BiSeNet-R18's stage maps at 768 x 1536 and 1024 x 2048, the GPU test's shapes, and the limits
  const int r18[4][2] = {{4, 64}, {8, 128}, {16, 256}, {32, 512}};
  for (const auto& s : r18) {
    check_shape(1, 768 / s[0], 1536 / s[0], s[1], s[1], false);
    check_shape(1, 1024 / s[0], 2048 / s[0], s[1], s[1], false);
    check_shape(16, 768 / s[0], 1536 / s[0], s[1], s[1], false);
  }
  check_shape(1, 5, 7, 16, 64, true);
  check_shape(2, 8, 32, 32, 64, true);
  check_shape(1, 9, 33, 48, 128, true);
  check_shape(1, 17, 40, 64, 192, true);
  check_shape(1, 72, 256, 16, 512, true);
  check_shape(1, 4096, 4096, 16, 64, false);             // 2^30 elements per image of y
  check_shape(1, 1, 33554431, 16, 64, false);            // (2^25 - 1) x 64 < 2^31
  check_shape(1, 2097151, 1, 1024, 64, false);
  check_shape(4096, 8, 32, 2048, 2048, false);
  check_shape(1000003, 1, 1, 16, 64, false);             // a tile per image

  check_refused(1, 8, 8, 24, 64);
  check_refused(1, 8, 8, 16, 96);
  check_refused(1, 8, 8, 16, 32);
  check_refused(1, 8, 8, 0, 64);
  check_refused(1, 8, 8, 16, 0);
  check_refused(1, 8, 8, -16, 64);
  check_refused(0, 8, 8, 16, 64);
  check_refused(1, 0, 8, 16, 64);
  check_refused(1, 8, 0, 16, 64);
  check_refused(-1, 8, 8, 16, 64);
  check_refused(1, 8192, 8192, 16, 64);                  // 2^32 elements per image
  check_refused(1, 1, 33554432, 16, 64);                 // 2^25 x 64 = 2^31
  check_refused(1, 65536, 65536, 16, 64);
  check_refused(2147483648LL, 1, 1, 16, 64);
  check_refused(2147483647, 9, 1, 16, 64);               // 2^32 - 2 tiles
  check_refused(INT64_MAX, 8, 8, 16, 64);
  check_refused(1, INT64_MAX, 8, 16, 64);
  check_refused(1, 8, INT64_MAX, 16, 64);
  check_refused(1, INT64_MAX, INT64_MAX, 16, 64);

  if (g_fail) { fprintf(stderr, "%d of %ld checks FAILED\n", g_fail, g_checks); return 1; }
  printf("%ld checks passed\n", g_checks);
  return 0;
}
