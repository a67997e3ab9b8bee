// Host-only check of torchseg_amd/csrc/pwb_geom.h, the plan of the fused 1x1 convolution + BatchNorm kernel (built and
// run by tests/test_pwbn_cpu.py with ASan + UBSan; UBSan stops on any signed overflow of an intermediate).
// For a sweep of shapes: every block id decodes to an (oc tile, slot) of its own, every (oc tile, pixel tile) is visited
// exactly once by the walk slot, slot + nslots, ..., every output element is owned by exactly one (block, wave, lane,
// register) under the kernel's store predicate, the row of x a stride-2 pixel reads lies inside x, in the pixel's own image
// and at the sub-sampled position, the packed filter's layout is a bijection of [Cout] x [Cin] whose rows put a lane's 16
// accumulator registers on consecutive channels and whose k order is the one the kernel's B operand loads, the largest
// element offset any lane forms stays below 2^31, and pwb_geom refuses everything just outside the limits.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../torchseg_amd/csrc/pwb_geom.h"

using namespace tsg;

static int g_fail = 0;
static long g_checks = 0;
static char g_what[160];
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { if (++g_fail < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_what); } \
  } while (0)

// elements: also count every output element and check every pixel's row (small shapes); otherwise tiles and extremes only
static void check_shape(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int stride, bool elements) {
  snprintf(g_what, sizeof g_what, "B %lld H %lld W %lld Cin %d Cout %d s %d", (long long)B, (long long)H, (long long)W, Cin,
           Cout, stride);
  PwbGeom g;
  if (!pwb_geom(&g, B, H, W, Cin, Cout, stride)) { CHECK(false); return; }
  CHECK(g.B == B && g.H == H && g.W == W && g.Cin == Cin && g.Cout == Cout && g.stride == stride);
  CHECK(g.OH == (H - 1) / stride + 1 && g.OW == (W - 1) / stride + 1 && (int64_t)g.P == B * g.OH * g.OW);
  CHECK((int64_t)g.ntiles == ((int64_t)g.P + PWB_TP - 1) / PWB_TP);
  CHECK(g.nchunks * PWB_KC == Cin && g.noct * PWB_BN == Cout);
  CHECK(g.nslots >= 8 && g.nslots % 8 == 0 && g.grid == g.nslots * g.noct);
  CHECK(g.nslots <= (g.ntiles + 7) / 8 * 8 || g.nslots == 8);              // no more than 7 idle slots beyond the tiles
  CHECK(g.grid <= PWB_BLOCKS + 8 * g.noct || g.nslots == 8);
  // 32 bits: every operand, the last tile's pixel index (also of the lanes past P), the filter
  CHECK(B * H * W * Cin <= PWB_ELEMS && (int64_t)g.P * Cout <= PWB_ELEMS);
  CHECK((int64_t)g.ntiles * PWB_TP <= PWB_ELEMS && (int64_t)Cin * Cout <= PWB_ELEMS);
  // block -> (oc tile, slot) is a bijection of [0, grid) onto [0, noct) x [0, nslots); the walk visits every pair once
  std::vector<unsigned char> seen((size_t)g.grid, 0);
  std::vector<unsigned char> tile_owner((size_t)g.noct * g.ntiles, 0);
  std::vector<unsigned char> el;
  if (elements) el.assign((size_t)g.P * Cout, 0);
  for (int blk = 0; blk < g.grid; ++blk) {
    int oct, slot;
    pwb_block(g, blk, &oct, &slot);
    CHECK(oct >= 0 && oct < g.noct && slot >= 0 && slot < g.nslots);
    if (oct < 0 || oct >= g.noct || slot < 0 || slot >= g.nslots) continue;
    CHECK((slot & 7) == (blk & 7));                                         // the blocks of a slot share an XCD
    const size_t id = (size_t)oct * g.nslots + slot;
    CHECK(seen[id] == 0);
    seen[id] = 1;
    for (int64_t tile = slot; tile < g.ntiles; tile += g.nslots) {
      CHECK(tile_owner[(size_t)oct * g.ntiles + tile] == 0);
      tile_owner[(size_t)oct * g.ntiles + tile] = 1;
      if (!elements) continue;
      for (int wave = 0; wave < 4; ++wave)
        for (int lane = 0; lane < 64; ++lane)
          for (int i = 0; i < 2; ++i) {
            const int64_t pix = tile * PWB_TP + wave * 64 + i * 32 + (lane & 31);
            if (pix >= g.P) continue;                                       // the kernel's load and store predicate
            for (int j = 0; j < 2; ++j)
              for (int r = 0; r < 16; ++r) {
                // the MFMA puts register r of lane half h on row (r & 3) + 8 (r >> 2) + 4 h of the 32-row A tile
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int oc = oct * PWB_BN + j * 32 + cbn_row_cout(row);
                CHECK(oc == oct * PWB_BN + j * 32 + (lane >> 5) * 16 + r);  // what the epilogue's address assumes
                unsigned char& n = el[(size_t)pix * Cout + oc];
                CHECK(n == 0);
                n = 1;
              }
          }
    }
  }
  for (unsigned char s : tile_owner) CHECK(s == 1);
  for (unsigned char s : el) CHECK(s == 1);
  // rows: inside x, inside the pixel's image, at the sub-sampled position; injective
  const int64_t step = elements ? 1 : (g.P > 4096 ? g.P / 4096 : 1);
  int64_t last = -1;
  auto check_row = [&](int64_t p) {
    const int64_t row = pwb_row(g, (int)p);
    const int64_t b = p / ((int64_t)g.OH * g.OW), r = p % ((int64_t)g.OH * g.OW), oh = r / g.OW, ow = r % g.OW;
    CHECK(row >= 0 && row < B * H * W);
    CHECK(row / (H * W) == b);
    CHECK(row == (b * H + stride * oh) * W + stride * ow);
    CHECK(stride * oh < H && stride * ow < W);
    CHECK((row + 1) * Cin <= PWB_ELEMS);
    return row;
  };
  for (int64_t p = 0; p < g.P; p += step) {
    const int64_t row = check_row(p);
    CHECK(row > last);
    last = row;
  }
  CHECK(check_row((int64_t)g.P - 1) >= last);
}

static void check_filter(int Cin, int Cout) {
  snprintf(g_what, sizeof g_what, "filter Cin %d Cout %d", Cin, Cout);
  const int nvec = Cin * Cout / 8, nch = Cin / PWB_KC;
  std::vector<unsigned char> seen((size_t)Cin * Cout, 0);
  for (int vec = 0; vec < nvec; ++vec) {
    int oc, ci0;
    pwb_filter_decode(vec, nch, &oc, &ci0);
    CHECK(oc >= 0 && oc < Cout && ci0 >= 0 && ci0 + 8 <= Cin && ci0 % 8 == 0);
    if (oc < 0 || oc >= Cout || ci0 < 0 || ci0 + 8 > Cin) continue;
    for (int e = 0; e < 8; ++e) {
      CHECK(seen[(size_t)oc * Cin + ci0 + e] == 0);
      seen[(size_t)oc * Cin + ci0 + e] = 1;
    }
    // the kernel: slab (oc tile, chunk) = 512 consecutive vectors, A fragment (ks, ocb) = 64 of them in lane order, and
    // lane (m, h) of step ks holds row m of the tile at the channels the B operand of lane half h holds at step ks
    const int lane = vec & 63, ocb = (vec >> 6) & 1, ks = (vec >> 7) & 3, slab = vec >> 9;
    CHECK(oc / PWB_BN == slab / nch && ci0 / PWB_KC == slab % nch);
    CHECK(oc % PWB_BN == ocb * 32 + cbn_row_cout(lane & 31));
    CHECK(ci0 % PWB_KC == pwb_lane_ci(lane >> 5, ks));
  }
  for (unsigned char s : seen) CHECK(s == 1);
}

static void check_refused(int64_t B, int64_t H, int64_t W, int Cin, int Cout, int stride) {
  snprintf(g_what, sizeof g_what, "refuse B %lld H %lld W %lld Cin %d Cout %d s %d", (long long)B, (long long)H, (long long)W,
           Cin, Cout, stride);
  PwbGeom g;
  CHECK(!pwb_geom(&g, B, H, W, Cin, Cout, stride));
}

int main() {
  // a lane's B operand of a chunk: the four steps are 64 contiguous bytes, the two halves the 128-byte line
  snprintf(g_what, sizeof g_what, "pwb_lane_ci");
  for (int h = 0; h < 2; ++h)
    for (int ks = 0; ks < 4; ++ks) CHECK(pwb_lane_ci(h, ks) == h * 32 + ks * 8);

  // the GPU test's cases
  check_shape(1, 5, 7, 64, 64, 1, true);
  check_shape(2, 8, 32, 128, 64, 1, true);
  check_shape(1, 9, 33, 192, 128, 1, true);
  check_shape(2, 9, 33, 64, 192, 2, true);
  check_shape(1, 18, 40, 256, 64, 2, true);
  check_shape(1, 130, 129, 64, 512, 1, true);
  const int sizes[] = {1, 2, 7, 16, 31, 33};
  for (int H : sizes)
    for (int W : sizes)
      for (int s = 1; s <= 2; ++s) {
        check_shape(1, H, W, 64, 64, s, true);
        check_shape(3, H, W, 128, 192, s, true);
      }
  // ResNet-50 (and the dilated form's) layers and BiSeNet-R18's shortcuts and ffm.conv_1x1 at 768 x 1536
  const int r50[][4] = {{4, 64, 64, 1},     {4, 64, 256, 1},    {4, 256, 64, 1},     {4, 256, 128, 1},  {4, 256, 512, 2},
                        {8, 128, 512, 1},   {8, 512, 128, 1},   {8, 512, 256, 1},    {8, 512, 1024, 2}, {16, 256, 1024, 1},
                        {16, 1024, 256, 1}, {16, 1024, 512, 1}, {16, 1024, 2048, 2}, {32, 512, 2048, 1}, {32, 2048, 512, 1},
                        {8, 1024, 2048, 1}, {8, 2048, 512, 1},  {4, 64, 128, 2},     {8, 128, 256, 2},  {16, 256, 512, 2},
                        {8, 256, 256, 1}};
  for (const auto& l : r50) {
    check_shape(1, 768 / l[0], 1536 / l[0], l[1], l[2], l[3], false);
    check_shape(16, 768 / l[0], 1536 / l[0], l[1], l[2], l[3], false);
  }
  // the edges of the supported set
  check_shape(1, 1, 1, 64, 64, 1, true);
  check_shape(1, 1, 1, 2048, 2048, 2, true);
  check_shape(1, 1, 33554431, 64, 64, 1, false);         // (2^25 - 1) x 64 < 2^31
  check_shape(1, 33554431, 1, 64, 64, 2, false);
  check_shape(1, 1024, 1023, 2048, 64, 1, false);        // x just under 2^31 elements
  check_shape(1, 1024, 1023, 64, 2048, 1, false);        // y just under 2^31 elements
  check_shape(1, 2045, 2047, 64, 2048, 2, false);        // OH OW = 1023 x 1024: y just under 2^31 elements
  check_shape(1048575, 1, 1, 2048, 64, 1, false);        // a pixel per image
  check_shape(4095, 8, 32, 2048, 64, 2, false);

  for (int Cin = 64; Cin <= 2048; Cin *= 2) check_filter(Cin, 64);
  check_filter(192, 128);
  check_filter(64, 2048);
  check_filter(2048, 2048);

  check_refused(1, 8, 8, 64, 64, 0);
  check_refused(1, 8, 8, 64, 64, 3);
  check_refused(1, 8, 8, 64, 64, -1);
  check_refused(1, 8, 8, 32, 64, 1);
  check_refused(1, 8, 8, 96, 64, 1);
  check_refused(1, 8, 8, 64, 96, 1);
  check_refused(1, 8, 8, 64, 32, 1);
  check_refused(1, 8, 8, 0, 64, 1);
  check_refused(1, 8, 8, 64, 0, 1);
  check_refused(1, 8, 8, -64, 64, 1);
  check_refused(1, 8, 8, 2112, 64, 1);
  check_refused(1, 8, 8, 64, 2112, 1);
  check_refused(0, 8, 8, 64, 64, 1);
  check_refused(1, 0, 8, 64, 64, 1);
  check_refused(1, 8, 0, 64, 64, 1);
  check_refused(-1, 8, 8, 64, 64, 1);
  check_refused(1, 1, 33554432, 64, 64, 1);              // 2^25 x 64 = 2^31
  check_refused(1, 1024, 1024, 2048, 64, 1);             // x: 2^31
  check_refused(1, 1024, 1024, 64, 2048, 1);             // y: 2^31
  check_refused(1, 2047, 2047, 64, 2048, 2);             // y: 2^20 x 2^11 = 2^31 (x: under 2^28)
  check_refused(1048576, 1, 1, 2048, 64, 1);
  check_refused(1, 65536, 65536, 64, 64, 1);
  check_refused(2147483648LL, 1, 1, 64, 64, 1);
  check_refused(INT64_MAX, 8, 8, 64, 64, 1);
  check_refused(1, INT64_MAX, 8, 64, 64, 2);
  check_refused(1, 8, INT64_MAX, 64, 64, 1);
  check_refused(1, INT64_MAX, INT64_MAX, 64, 64, 2);

  if (g_fail) { fprintf(stderr, "%d of %ld checks FAILED\n", g_fail, g_checks); return 1; }
  printf("%ld checks passed\n", g_checks);
  return 0;
}
