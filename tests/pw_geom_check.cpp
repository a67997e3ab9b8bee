// Host-only check of torchseg_amd/csrc/pw_geom.h, the plan of the 1x1 weight-gradient kernel (built and run by
// tests/test_pwwgrad_cpu.py with ASan + UBSan; UBSan stops on any signed overflow of an intermediate).  For every shape
// of a sweep: the slices' pixel ranges tile [0, P) exactly once and in order, all but the last are whole chunks, the grid
// reaches every (C_out tile, C_in tile, slice) exactly once and the channel tiles cover every channel, the workspace size
// is S C_out C_in 4 (0 for one slice), and -- for the shapes small enough to walk -- the byte offsets the kernel's threads
// step through (pw_pix + pw_advance) equal the exact 64-bit offsets of row(p) and p for every pixel below the slice's end.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../torchseg_amd/csrc/pw_geom.h"

using namespace tsg;

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { if (++g_fail < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_what); } \
  } while (0)
static char g_what[160];

struct Shape { int Cin, Cout; int64_t B; int H, W, stride; };

static void check_supported(const Shape& s, bool walk) {
  snprintf(g_what, sizeof g_what, "Cin %d Cout %d B %lld H %d W %d stride %d", s.Cin, s.Cout, (long long)s.B, s.H, s.W, s.stride);
  PwGeom g;
  CHECK(pw_shape_ok(s.Cin, s.Cout, s.B, s.H, s.W, s.stride));
  if (!pw_geom(&g, s.Cin, s.Cout, s.B, s.H, s.W, s.stride)) { CHECK(false); return; }
  CHECK(g.OH == (s.H - 1) / s.stride + 1 && g.OW == (s.W - 1) / s.stride + 1);
  CHECK(g.P == s.B * g.OH * g.OW && g.P >= 1);
  // both operands fit 32-bit byte offsets with room for the out-of-bounds marker
  CHECK((uint64_t)s.B * s.H * s.W * s.Cin * 2 <= 0xffffff80ull && (uint64_t)g.P * s.Cout * 2 <= 0xffffff80ull);
  // channel tiles cover every channel exactly
  CHECK((g.bm == 64 || g.bm == 128) && (g.bn == 64 || g.bn == 128));
  CHECK(g.tiles_m * g.bm == s.Cout && g.tiles_n * g.bn == s.Cin && g.tiles == g.tiles_m * g.tiles_n);
  // slices: [0, P) once, in order; whole chunks but for the last; at least one pixel each
  CHECK(g.S >= 1 && g.cps >= 1 && g.nchunks == (g.P + PW_KC - 1) / PW_KC);
  int64_t next = 0;
  for (int sl = 0; sl < g.S; ++sl) {
    int64_t p0, p1;
    pw_slice_range(g, sl, &p0, &p1);
    CHECK(p0 == next && p1 > p0 && p1 <= g.P);
    CHECK(p0 % PW_KC == 0 && (sl == g.S - 1 || p1 - p0 == g.cps * PW_KC));
    next = p1;
  }
  CHECK(next == g.P);
  CHECK(g.S == 1 || g.cps >= PW_MIN_CHUNKS);
  CHECK(pw_ws_bytes(g) == (g.S > 1 ? (uint64_t)g.S * s.Cout * s.Cin * 4 : 0));
  // the same shape plans the same way again
  PwGeom h;
  CHECK(pw_geom(&h, s.Cin, s.Cout, s.B, s.H, s.W, s.stride) && h.S == g.S && h.cps == g.cps && h.grid == g.grid);
  // grid: every (tile, slice) exactly once, the surplus ids carry slice >= S
  CHECK(g.grid >= (int64_t)g.tiles * g.S && g.grid <= (int64_t)g.tiles * (g.S + 7) && g.grid <= 0x7fffffffLL);
  std::vector<unsigned char> seen((size_t)g.tiles * g.S, 0);
  int64_t idle = 0;
  for (int64_t id = 0; id < g.grid; ++id) {
    int tm, tn, sl;
    pw_block(g, id, &tm, &tn, &sl);
    CHECK(tm >= 0 && tm < g.tiles_m && tn >= 0 && tn < g.tiles_n && sl >= 0);
    if (sl >= g.S) { ++idle; continue; }
    unsigned char& c = seen[((size_t)sl * g.tiles_m + tm) * g.tiles_n + tn];
    CHECK(c == 0);
    c = 1;
  }
  CHECK(g.grid - idle == (int64_t)g.tiles * g.S);
  if (!walk) return;
  // the threads' walk: thread pixel slot j (0 .. 63 of a chunk) starts at p0 + j and advances one chunk at a time
  const PwSteps st = pw_steps(g);
  for (int sl = 0; sl < g.S; ++sl) {
    int64_t p0, p1;
    pw_slice_range(g, sl, &p0, &p1);
    const int64_t nch = (p1 - p0 + PW_KC - 1) / PW_KC;
    for (int j = 0; j < PW_KC; ++j) {
      PwPix q = pw_pix(g, (int)(p0 + j));
      for (int64_t c = 0; c <= nch; ++c) {            // the kernel fetches one chunk past the slice (all lanes masked)
        const int64_t p = p0 + j + c * PW_KC;
        CHECK(q.p == p);
        if (p < p1) {
          const int64_t b = p / ((int64_t)g.OH * g.OW), r = p % ((int64_t)g.OH * g.OW), oh = r / g.OW, ow = r % g.OW;
          const int64_t row = (b * g.H + s.stride * oh) * g.W + s.stride * ow;
          CHECK(oh == q.oh && ow == q.ow);
          CHECK(s.stride * oh < g.H && s.stride * ow < g.W && b < s.B);
          CHECK((uint64_t)q.xo == (uint64_t)row * s.Cin * 2);
          CHECK((uint64_t)q.dyo == (uint64_t)p * s.Cout * 2);
          // the last 16-byte access of the last channel part ends inside the operand
          CHECK((uint64_t)q.xo + (uint64_t)s.Cin * 2 <= (uint64_t)s.B * s.H * s.W * s.Cin * 2);
        }
        pw_advance(g, st, &q);
      }
    }
  }
}

static void check_refused(int Cin, int Cout, int64_t B, int H, int W, int stride) {
  snprintf(g_what, sizeof g_what, "refuse Cin %d Cout %d B %lld H %d W %d stride %d", Cin, Cout, (long long)B, H, W, stride);
  PwGeom g;
  CHECK(!pw_shape_ok(Cin, Cout, B, H, W, stride));
  CHECK(!pw_geom(&g, Cin, Cout, B, H, W, stride));
}

int main() {
  const Shape walked[] = {
      {64, 64, 1, 1, 1, 1},        {64, 64, 1, 1, 1, 2},       {64, 128, 2, 5, 7, 1},      {128, 64, 1, 9, 9, 2},
      {64, 64, 2, 8, 6, 2},        {192, 320, 1, 6, 6, 1},     {2048, 512, 1, 3, 3, 1},    {512, 2048, 1, 3, 3, 1},
      {64, 64, 4, 64, 64, 1},      {256, 64, 2, 46, 45, 2},    {64, 64, 1, 1, 127, 1},     {64, 64, 127, 1, 1, 1},
      {64, 64, 1, 13, 1, 2},       {64, 64, 7, 13, 11, 2},     {64, 64, 5, 12, 10, 2},     {64, 64, 3, 7, 12, 2},
      {64, 64, 3, 12, 7, 2},       {128, 128, 1, 257, 1, 1},   {64, 64, 1, 1, 8191, 1},    {64, 64, 131, 2, 2, 2},
      {64, 64, 70, 1, 2, 2},       {64, 64, 9, 3, 200, 2},     {64, 64, 2, 200, 3, 2},     {64, 64, 1, 1031, 1, 2},
      {256, 512, 16, 32, 32, 1},   {256, 512, 2, 128, 128, 2}, {64, 64, 1, 97, 89, 1},     {1024, 2048, 2, 65, 65, 2},
  };
  for (const Shape& s : walked) check_supported(s, true);
  // the shapes the benchmarked networks produce, and the 2^31-element edge (too long to walk pixel by pixel)
  const Shape planned[] = {
      {64, 128, 16, 256, 256, 2},    {128, 128, 16, 128, 128, 1},  {2048, 512, 2, 32, 32, 1},   {256, 64, 2, 256, 256, 1},
      {64, 64, 1, 4096, 8191, 1},    {64, 64, 524287, 8, 8, 1},    {2048, 64, 1, 1023, 1024, 1}, {2048, 2048, 1, 1023, 1024, 2},
      {64, 2048, 4095, 16, 16, 1},   {64, 64, 1, 1, 33554431, 2},  {64, 64, 33554431, 1, 1, 1},
  };
  for (const Shape& s : planned) check_supported(s, false);
  // walk the thread offsets at the edge as well, for the first and last chunk of the first and last slice only
  {
    const Shape s = {2048, 64, 1, 1023, 1024, 1};
    PwGeom g;
    snprintf(g_what, sizeof g_what, "edge walk");
    CHECK(pw_geom(&g, s.Cin, s.Cout, s.B, s.H, s.W, s.stride));
    const PwSteps st = pw_steps(g);
    int64_t p0, p1;
    pw_slice_range(g, g.S - 1, &p0, &p1);
    for (int j = 0; j < PW_KC; ++j) {
      PwPix q = pw_pix(g, (int)(p0 + j));
      for (int64_t p = p0 + j; p < p1; p += PW_KC) {
        CHECK((uint64_t)q.xo == (uint64_t)p * s.Cin * 2 && (uint64_t)q.dyo == (uint64_t)p * s.Cout * 2);
        pw_advance(g, st, &q);
      }
    }
  }
  // outside the accepted set
  check_refused(72, 64, 1, 8, 8, 1);
  check_refused(64, 96, 1, 8, 8, 1);
  check_refused(32, 64, 1, 8, 8, 1);
  check_refused(64, 2112, 1, 8, 8, 1);
  check_refused(64, 64, 1, 8, 8, 3);
  check_refused(64, 64, 1, 8, 8, 0);
  check_refused(64, 64, 0, 8, 8, 1);
  check_refused(64, 64, -1, 8, 8, 1);
  check_refused(64, 64, 1, 0, 8, 1);
  check_refused(64, 64, 1, 8, 0, 2);
  check_refused(64, 64, 1, 4096, 8192, 1);                   // exactly 2^31 elements of x
  check_refused(64, 64, 33554432, 1, 1, 1);                  // exactly 2^31 elements
  check_refused(64, 128, 1, 4096, 4096, 1);                  // x fits, dy does not
  check_refused(2048, 2048, INT64_MAX, 2147483647, 2147483647, 2);
  check_refused(64, 64, INT64_MAX, 1, 1, 1);
  check_refused(64, 64, 1, 2147483647, 2147483647, 1);

  if (g_fail) { fprintf(stderr, "%d of %ld checks FAILED\n", g_fail, g_checks); return 1; }
  printf("%ld checks passed\n", g_checks);
  return 0;
}
