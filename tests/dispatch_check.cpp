// Host-only check of torchseg_amd/csrc/tsg_dispatch.h (built and run by tests/test_dispatch_cpu.py with ASan + UBSan):
// every dispatcher hands its callable exactly the documented tag for every accepted runtime value and passes the
// callable's return value through; for a value outside the accepted set the callable is not called and the documented
// error code comes back.
#include <cstdio>
#include <type_traits>
#include "../torchseg_amd/csrc/tsg_dispatch.h"

using namespace tsg;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { ++g_fail; fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
  } while (0)

// what a callable saw: how often it ran, and the tags of the last call as plain numbers
struct Seen { int calls = 0, elem = -1, v = -1, lab = -1, n = -1, flag = -1; };
template <typename T> constexpr int elem_code() {
  static_assert(std::is_same<T, float>::value || std::is_same<T, bf16_t>::value, "unexpected element type");
  return std::is_same<T, float>::value ? TSG_F32 : TSG_BF16;
}

int main() {
  static_assert(int_tag<7>() == 7 && bool_tag<true>(), "tags convert to their value in a constant expression");
  static_assert(std::is_same<type_tag<bf16_t>::type, bf16_t>::value, "type_tag names its type");
  static_assert(sizeof(float) * Vec<float>::N == 16 && sizeof(bf16_t) * Vec<bf16_t>::N == 16, "16-byte vectors");

  CHECK(native_vec(TSG_F32) == 4);
  CHECK(native_vec(TSG_BF16) == 8);

  // with_elem
  const int dtypes[2] = {TSG_F32, TSG_BF16};
  for (int dt : dtypes) {
    Seen s;
    const int r = with_elem(dt, [&](auto t) {
      ++s.calls; s.elem = elem_code<typename decltype(t)::type>();
      return 1000 + dt;
    });
    CHECK(r == 1000 + dt); CHECK(s.calls == 1); CHECK(s.elem == dt);
  }
  const int bad_dtypes[2] = {2, -1};
  for (int dt : bad_dtypes) {
    Seen s;
    CHECK(with_elem(dt, [&](auto) { ++s.calls; return 0; }) == TSG_E_DTYPE);
    CHECK(s.calls == 0);
    CHECK(with_elem_vec(dt, true, [&](auto, auto) { ++s.calls; return 0; }) == TSG_E_DTYPE);
    CHECK(with_elem_vec(dt, false, [&](auto, auto) { ++s.calls; return 0; }) == TSG_E_DTYPE);
    CHECK(s.calls == 0);
  }

  // with_elem_vec: f32 -> float, 4 | 1; bf16 -> bf16_t, 8 | 1
  for (int dt : dtypes)
    for (int vec = 0; vec < 2; ++vec) {
      Seen s;
      const int r = with_elem_vec(dt, vec != 0, [&](auto t, auto v) {
        constexpr int V = v();                      // usable as a template argument
        ++s.calls; s.elem = elem_code<typename decltype(t)::type>(); s.v = int_tag<V>::value;
        return 2000 + 10 * dt + vec;
      });
      CHECK(r == 2000 + 10 * dt + vec); CHECK(s.calls == 1); CHECK(s.elem == dt);
      CHECK(s.v == (vec ? (dt == TSG_BF16 ? 8 : 4) : 1));
    }

  // with_label
  const int ltypes[2] = {TSG_I64, TSG_U8};
  for (int lt : ltypes) {
    Seen s;
    const int r = with_label(lt, [&](auto l) { ++s.calls; s.lab = int_tag<l()>::value; return 3000 + lt; });
    CHECK(r == 3000 + lt); CHECK(s.calls == 1); CHECK(s.lab == lt);
  }
  {
    Seen s;
    CHECK(with_label(7, [&](auto) { ++s.calls; return 0; }) == TSG_E_DTYPE);
    CHECK(with_label(-1, [&](auto) { ++s.calls; return 0; }) == TSG_E_DTYPE);
    CHECK(s.calls == 0);
  }

  // with_flag
  for (int b = 0; b < 2; ++b) {
    Seen s;
    const int r = with_flag(b != 0, [&](auto f) { ++s.calls; s.flag = bool_tag<f()>::value ? 1 : 0; return 4000 + b; });
    CHECK(r == 4000 + b); CHECK(s.calls == 1); CHECK(s.flag == b);
  }

  // with_int: the sets the launchers use, 0 included, and values next to the members
  const int in_set[4] = {9, 21, 37, 0};
  for (int n : in_set) {
    Seen s;
    const int r = with_int<9, 21, 37, 0>(n, [&](auto c) { ++s.calls; s.n = int_tag<c()>::value; return 5000 + n; });
    CHECK(r == 5000 + n); CHECK(s.calls == 1); CHECK(s.n == n);
  }
  const int out_of_set[6] = {0, 8, 10, 22, -9, 1 << 30};
  for (int n : out_of_set) {
    Seen s;
    CHECK((with_int<9, 21, 37>(n, [&](auto) { ++s.calls; return 0; })) == TSG_E_SHAPE);
    CHECK(s.calls == 0);
  }
  {
    Seen s;                                          // a single-member set; a callable's own error code is passed through
    CHECK((with_int<16>(16, [&](auto c) { ++s.calls; s.n = c(); return TSG_E_ALIGN; })) == TSG_E_ALIGN);
    CHECK(s.calls == 1); CHECK(s.n == 16);
    CHECK((with_int<16>(32, [&](auto) { ++s.calls; return 0; })) == TSG_E_SHAPE);
    CHECK(s.calls == 1);
  }

  // nested, as a launcher writes it: every combination arrives exactly once
  int hits[2][2][2][2] = {};
  for (int dt : dtypes)
    for (int vec = 0; vec < 2; ++vec)
      for (int lt : ltypes)
        for (int b = 0; b < 2; ++b) {
          const int r = with_elem_vec(dt, vec != 0, [&](auto t, auto v) {
            return with_label(lt, [&](auto l) {
              return with_flag(b != 0, [&](auto f) {
                typedef typename decltype(t)::type T;
                ++hits[elem_code<T>()][v() == Vec<T>::N ? 1 : 0][l()][f() ? 1 : 0];
                return v() == 1 || v() == Vec<T>::N ? 0 : TSG_E_SHAPE;
              });
            });
          });
          CHECK(r == 0); CHECK(hits[dt][vec][lt][b] == 1);
        }

  if (g_fail) { fprintf(stderr, "dispatch_check: %d of %d checks FAILED\n", g_fail, g_checks); return 1; }
  printf("dispatch_check: %d checks passed\n", g_checks);
  return 0;
}
