// Host-only check of torchseg_amd/csrc/sep_geom.h, the plan of the fused separable unit (built and run by
// tests/test_sepconv_cpu.py with ASan + UBSan; UBSan stops on any signed overflow of an intermediate).  For every accepted
// channel pair: the pack's sections are 16-byte aligned, in order and do not overlap; sep_row_cout is a bijection whose
// image puts the 16 accumulator rows of either lane half on 16 consecutive channels; sep_wp_frag_index sends every
// (co, ci) of the padded matrix to its own element of the section, and is the inverse of the decode the pack kernel uses.
// For a sweep of shapes: the strips tile [0, npix) exactly, the grid fits, the last byte any lane of a strip touches in x
// and y lies inside the tensor, and the LDS image of a strip fits the kernels' static arrays.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../torchseg_amd/csrc/sep_geom.h"

using namespace tsg;

static int g_fail = 0;
static long g_checks = 0;
static char g_what[160];
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { if (++g_fail < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_what); } \
  } while (0)

static void check_pack(int Cin, int Cout) {
  for (int bf = 0; bf < 2; ++bf) {
    snprintf(g_what, sizeof g_what, "pack Cin %d Cout %d bf16 %d", Cin, Cout, bf);
    SepGeom g;
    if (!sep_pack_layout(&g, Cin, Cout, bf != 0)) { CHECK(false); return; }
    CHECK(g.nvec * 8 == Cin && g.KP >= Cin && g.KP < Cin + 16 && g.KP % 16 == 0 && g.NKS * 16 == g.KP);
    CHECK(g.MT * 32 >= Cout && g.MT * 32 < Cout + 32);
    CHECK(g.ab_off == (size_t)Cin * 36 && g.ab_off % 16 == 0 && g.wp_off == g.ab_off + (size_t)Cout * 8 && g.wp_off % 16 == 0);
    CHECK(g.pack_bytes % 16 == 0 && g.pack_bytes > g.wp_off && g.pack_bytes < (1u << 20));
    if (!bf) { CHECK(g.pack_bytes - g.wp_off == (size_t)Cin * Cout * 4); continue; }
    const size_t n = (size_t)g.MT * g.NKS * 512;
    CHECK(g.pack_bytes - g.wp_off == n * 2);
    std::vector<unsigned char> seen(n, 0);
    for (int co = 0; co < g.MT * 32; ++co)
      for (int ci = 0; ci < g.KP; ++ci) {
        const int j = sep_wp_frag_index(co, ci, g.NKS);
        CHECK(j >= 0 && (size_t)j < n);
        if (j < 0 || (size_t)j >= n) continue;
        CHECK(seen[j] == 0);
        seen[j] = 1;
        // the pack kernel's decode of element j
        const int e = j & 7, lane = (j >> 3) & 63, blk = j >> 9, ks = blk % g.NKS, mt = blk / g.NKS;
        CHECK(mt * 32 + sep_row_cout(lane & 31) == co && ks * 16 + (lane >> 5) * 8 + e == ci);
      }
  }
}

static void check_shape(int Cin, int Cout, int stride, int64_t B, int H, int W) {
  for (int bf = 0; bf < 2; ++bf) {
    snprintf(g_what, sizeof g_what, "Cin %d Cout %d s %d B %lld H %d W %d bf16 %d", Cin, Cout, stride, (long long)B, H, W, bf);
    SepGeom g;
    CHECK(sep_shape_ok(Cin, Cout, stride, B, H, W));
    if (!sep_geom(&g, Cin, Cout, stride, B, H, W, bf != 0)) { CHECK(false); return; }
    CHECK(g.OH == (H - 1) / stride + 1 && g.OW == (W - 1) / stride + 1 && g.npix == B * g.OH * g.OW && g.npix >= 1);
    CHECK(bf ? (g.TP == SEP_TP_BIG || g.TP == SEP_TP_SMALL) : g.TP == SEP_TP_F32);
    CHECK(!bf || (g.TP == SEP_TP_BIG) == (g.npix >= SEP_BIG_FROM));
    CHECK(g.grid >= 1 && g.grid <= 0x7fffffffLL && (g.grid - 1) * g.TP < g.npix && g.grid * g.TP >= g.npix);
    // LDS: bf16 rows of KP + pad elements / fp64 rows of C_in elements inside the static arrays
    if (bf) CHECK((size_t)g.TP * (g.KP + SEP_LDS_PAD) <= (size_t)g.TP * (SEP_CIN_MAX + SEP_LDS_PAD) && (g.KP + SEP_LDS_PAD) % 8 == 0);
    else CHECK((size_t)g.TP * g.Cin <= (size_t)SEP_TP_F32 * SEP_CIN_MAX);
    // the last pixel's last tap and last store end inside the tensors (64-bit element offsets)
    const int64_t p = g.npix - 1, ow = p % g.OW, q = p / g.OW, oh = q % g.OH, b = q / g.OH;
    CHECK(b == B - 1 && oh * stride < H && ow * stride < W);
    const int64_t ih = oh * stride + 1 < H ? oh * stride + 1 : H - 1, iw = ow * stride + 1 < W ? ow * stride + 1 : W - 1;
    CHECK(((b * H + ih) * W + iw) * Cin + Cin <= B * H * W * Cin);
    CHECK(p * Cout + Cout == g.npix * Cout && g.npix * Cout <= SEP_ELEMS);
    // every thread of phase 1 has a group or is idle: pixel lanes x groups <= threads, at least one pixel lane
    const int npl = SEP_THREADS / g.nvec;
    CHECK(npl >= 1 && npl * g.nvec <= SEP_THREADS);
  }
}

static void check_refused(int Cin, int Cout, int stride, int64_t B, int H, int W) {
  snprintf(g_what, sizeof g_what, "refuse Cin %d Cout %d s %d B %lld H %d W %d", Cin, Cout, stride, (long long)B, H, W);
  SepGeom g;
  CHECK(!sep_shape_ok(Cin, Cout, stride, B, H, W));
  CHECK(!sep_geom(&g, Cin, Cout, stride, B, H, W, true) && !sep_geom(&g, Cin, Cout, stride, B, H, W, false));
}

int main() {
  // the row permutation
  snprintf(g_what, sizeof g_what, "sep_row_cout");
  unsigned seen = 0;
  for (int row = 0; row < 32; ++row) {
    const int c = sep_row_cout(row);
    CHECK(c >= 0 && c < 32 && !((seen >> c) & 1u));
    seen |= 1u << c;
  }
  CHECK(seen == 0xffffffffu);
  for (int h = 0; h < 2; ++h)
    for (int r = 0; r < 16; ++r)          // accumulator register r of lane half h: row (r & 3) + 8 (r >> 2) + 4 h
      CHECK(sep_row_cout((r & 3) + 8 * (r >> 2) + 4 * h) == 16 * h + r);

  for (int Cin = SEP_CIN_MIN; Cin <= SEP_CIN_MAX; Cin += 8)
    for (int Cout = SEP_COUT_MIN; Cout <= SEP_COUT_MAX; Cout += 16) check_pack(Cin, Cout);

  const int x39[15][3] = {{8, 64, 2},    {8, 16, 2},   {16, 16, 1},  {16, 64, 1},  {64, 16, 1},
                          {64, 128, 2},  {64, 32, 2},  {32, 32, 1},  {32, 128, 1}, {128, 32, 1},
                          {128, 256, 2}, {128, 64, 2}, {64, 64, 1},  {64, 256, 1}, {256, 64, 1}};
  const int sizes[][3] = {{1, 1, 1}, {2, 13, 19}, {1, 1, 9}, {3, 7, 5}, {2, 33, 47}, {1, 96, 192}, {1, 128, 256},
                          {1, 256, 512}, {16, 192, 384}, {1, 1, 32767}, {1, 32768, 1}};
  for (const auto& c : x39)
    for (const auto& s : sizes) check_shape(c[0], c[1], c[2], s[0], s[1], s[2]);
  check_shape(24, 48, 1, 2, 9, 11);                      // C_in % 16 == 8, three groups: 85 pixel lanes, one idle thread
  check_shape(248, 240, 2, 1, 5, 5);
  check_shape(256, 256, 1, 1, 65536, 65536);            // 2^32 pixels: the element offsets need 64 bits
  check_shape(8, 16, 2, 4096, 1024, 1024);
  check_shape(256, 256, 1, 1, 1, 1);

  check_refused(4, 16, 1, 1, 8, 8);
  check_refused(12, 16, 1, 1, 8, 8);
  check_refused(264, 16, 1, 1, 8, 8);
  check_refused(8, 8, 1, 1, 8, 8);
  check_refused(8, 24, 1, 1, 8, 8);
  check_refused(8, 272, 1, 1, 8, 8);
  check_refused(8, 16, 3, 1, 8, 8);
  check_refused(8, 16, 0, 1, 8, 8);
  check_refused(8, 16, 1, 0, 8, 8);
  check_refused(8, 16, 1, 1, 0, 8);
  check_refused(8, 16, 1, 1, 8, 0);
  check_refused(8, 16, 1, 1, -1, 8);
  check_refused(8, 16, 1, INT64_MAX, 8, 8);
  check_refused(256, 256, 2, 1, 2147483647, 2147483647);
  check_refused(8, 16, 1, 2, 65536, 65536);              // 2^33 pixels x 256: past the 2^40 elements accepted

  if (g_fail) { fprintf(stderr, "%d of %ld checks FAILED\n", g_fail, g_checks); return 1; }
  printf("%ld checks passed\n", g_checks);
  return 0;
}
