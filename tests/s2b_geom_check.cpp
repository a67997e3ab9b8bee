// Host-only check of torchseg_amd/csrc/s2b_geom.h, the plan of the fused stride-2 3x3 convolution + BatchNorm kernel
// (built and run by tests/test_s2bn_cpu.py with ASan + UBSan; UBSan stops on any signed overflow of an intermediate).
// For a sweep of shapes: OH, OW and the tile counts; every block id decodes to an (oc tile, slot) of its own; every OUTPUT
// pixel of every oc tile is owned by exactly one (block, tile step); the tiles of a block come from the walk slot, slot +
// nslots, ...; the largest element offset formed inside one image of x and of y / the residual stays below 2^31.  For the
// patch: (pr, pc) -> LDS pixel is a bijection of the 9 x 65 patch onto [0, 585); for every tile pixel and tap the LDS
// pixel the B fragment reads is the patch pixel whose input coordinates are (2 oh + kh - 1, 2 ow + kw - 1), so the patch
// covers every tap; and the 32 lanes of a fragment read consecutive LDS pixels.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../torchseg_amd/csrc/s2b_geom.h"

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
  S2bGeom g;
  if (!s2b_geom(&g, B, H, W, Cin, Cout)) { CHECK(false); return; }
  CHECK(g.B == B && g.H == H && g.W == W && g.Cin == Cin && g.Cout == Cout);
  const int64_t OH = (H + 1) / 2, OW = (W + 1) / 2;
  CHECK(g.OH == OH && g.OW == OW);
  CHECK(OH == (H + 2 - 3) / 2 + 1 && OW == (W + 2 - 3) / 2 + 1);          // the convolution's own formula
  CHECK(g.tiles_h == (OH + S2B_TH - 1) / S2B_TH && g.tiles_w == (OW + S2B_TW - 1) / S2B_TW);
  CHECK((int64_t)g.ntiles == B * g.tiles_h * g.tiles_w);
  CHECK(g.nchunks * CBN_KC == Cin && g.noct * CBN_BN == Cout);
  CHECK(g.nslots >= 8 && g.nslots % 8 == 0 && g.grid == g.nslots * g.noct);
  CHECK(g.nslots <= (g.ntiles + 7) / 8 * 8 || g.nslots == 8);             // no more than 7 idle slots beyond the tiles
  CHECK((int64_t)g.nslots * g.noct <= S2B_BLOCKS + 8 * g.noct || g.nslots == 8);
  // offsets: the last element of one image of x and of y / the residual (the 32-bit claim), the batch offset in int64
  CHECK(((H - 1) * W + (W - 1)) * Cin + Cin <= CBN_MAX_OFF);
  CHECK(((OH - 1) * OW + (OW - 1)) * Cout + Cout <= CBN_MAX_OFF);
  CHECK(B * H * W <= INT64_MAX / Cin && B * OH * OW <= INT64_MAX / Cout);
  // the last tap of the last output pixel: inside the image or exactly one row / column of padding beyond it
  CHECK(2 * (OH - 1) + 1 == H - 1 || 2 * (OH - 1) + 1 == H);
  CHECK(2 * (OW - 1) + 1 == W - 1 || 2 * (OW - 1) + 1 == W);
  std::vector<unsigned char> seen((size_t)g.grid, 0);
  std::vector<unsigned char> tile_owner((size_t)g.noct * g.ntiles, 0);
  std::vector<unsigned char> px;
  if (pixels) px.assign((size_t)g.noct * B * OH * OW, 0);
  for (int blk = 0; blk < g.grid; ++blk) {
    int oct, slot;
    s2b_block(g, blk, &oct, &slot);
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
      s2b_tile(g, (int)tile, &b, &oh0, &ow0);
      CHECK(b >= 0 && b < B && oh0 >= 0 && oh0 < OH && ow0 >= 0 && ow0 < OW && oh0 % S2B_TH == 0 && ow0 % S2B_TW == 0);
      if (b < 0 || b >= B) continue;
      // the patch of this tile: every tap of every stored pixel is the patch pixel with the convolution's coordinates
      if (oct == 0)
        for (int r = 0; r < S2B_TH; ++r)
          for (int c = 0; c < S2B_TW; c += (pixels ? 1 : 31))
            for (int kh = 0; kh < 3; ++kh)
              for (int kw = 0; kw < 3; ++kw) {
                const int pr = 2 * r + kh, pc = 2 * c + kw;
                CHECK(pr < S2B_PH && pc < S2B_PW);
                CHECK(s2b_patch_ih(oh0, pr) == 2 * (oh0 + r) + kh - 1 && s2b_patch_iw(ow0, pc) == 2 * (ow0 + c) + kw - 1);
                CHECK(s2b_tap_lds(r, c, kh, kw) == s2b_patch_lds(pr, pc));
              }
      if (!pixels) continue;
      for (int r = 0; r < S2B_TH; ++r)
        for (int c = 0; c < S2B_TW; ++c) {
          const int64_t oh = oh0 + r, ow = ow0 + c;
          if (oh >= OH || ow >= OW) continue;                               // the kernel's store predicate
          unsigned char& n = px[((size_t)oct * B + b) * OH * OW + oh * OW + ow];
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
  S2bGeom g;
  CHECK(!s2b_geom(&g, B, H, W, Cin, Cout));
}

int main() {
  snprintf(g_what, sizeof g_what, "patch planes");
  CHECK(S2B_PH == 2 * S2B_TH + 1 && S2B_PW == 2 * S2B_TW + 1 && S2B_NPX == S2B_PH * S2B_PW);
  CHECK(S2B_ODD0 == S2B_PH * S2B_EW && S2B_ODD0 + S2B_PH * S2B_DW == S2B_NPX);
  std::vector<unsigned char> lds((size_t)S2B_NPX, 0);
  for (int pr = 0; pr < S2B_PH; ++pr)
    for (int pc = 0; pc < S2B_PW; ++pc) {
      const int q = s2b_patch_lds(pr, pc);
      CHECK(q >= 0 && q < S2B_NPX);
      if (q < 0 || q >= S2B_NPX) continue;
      CHECK(lds[(size_t)q] == 0);
      lds[(size_t)q] = 1;
      CHECK((q < S2B_ODD0) == ((pc & 1) == 0));                             // even columns in the first plane
    }
  for (unsigned char s : lds) CHECK(s == 1);
  for (int r = 0; r < S2B_TH; ++r)
    for (int kh = 0; kh < 3; ++kh)
      for (int kw = 0; kw < 3; ++kw)
        for (int p = 0; p < S2B_TW; ++p) {
          const int q = s2b_tap_lds(r, p, kh, kw);
          CHECK(q >= 0 && q < S2B_NPX);
          CHECK(q == s2b_tap_lds(r, 0, kh, kw) + p);                        // a fragment's 32 lanes: consecutive pixels
        }

  const int sizes[] = {1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 66, 143, 511};
  const int couts[] = {64, 192, 512};
  for (int H : sizes)
    for (int W : sizes)
      for (int Cout : couts) {
        check_shape(1, H, W, 16, Cout, true);
        check_shape(3, H, W, 48, Cout, H * W <= 144 * 144);
      }
  // the stride-2 layers of BiSeNet-R18 and ResNet-50 at 768 x 1536 and 1024 x 2048, the GPU test's shapes, and the limits
  const int layers[8][3] = {{2, 64, 64}, {4, 64, 64}, {4, 64, 128}, {8, 128, 256}, {16, 256, 512},
                            {4, 128, 128}, {8, 256, 256}, {16, 512, 512}};
  for (const auto& s : layers) {
    check_shape(1, 768 / s[0], 1536 / s[0], s[1], s[2], false);
    check_shape(1, 1024 / s[0], 2048 / s[0], s[1], s[2], false);
    check_shape(16, 768 / s[0], 1536 / s[0], s[1], s[2], false);
  }
  check_shape(1, 1, 3, 16, 64, true);
  check_shape(1, 5, 7, 16, 64, true);
  check_shape(1, 6, 8, 16, 64, true);
  check_shape(2, 16, 64, 32, 64, true);
  check_shape(1, 17, 66, 48, 128, true);
  check_shape(1, 34, 79, 64, 192, true);
  check_shape(1, 143, 511, 16, 512, true);
  check_shape(1, 8192, 8192, 16, 64, false);             // 2^30 elements per image of x, 2^30 per image of y
  check_shape(1, 1, 67108861, 16, 64, false);            // OW = 2^25 - 1: (2^25 - 1) x 64 < 2^31 elements of y
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
  check_refused(1, 16384, 8192, 16, 64);                 // 2^31 elements per image of x
  check_refused(1, 8192, 8192, 32, 64);                  // 2^31 elements per image of x
  check_refused(1, 8192, 8192, 16, 128);                 // 2^31 elements per image of y
  check_refused(1, 1, 67108863, 16, 64);                 // OW = 2^25: 2^31 elements of y, x fits
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
