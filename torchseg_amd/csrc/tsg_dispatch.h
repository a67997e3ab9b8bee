// Host-side dispatch of the launchers: one place that turns the runtime codes of the C ABI (dtype, "16-byte vectors
// allowed", label type, flags, small enumerations) into template arguments.  Each dispatcher hands the callable a tag
// and returns the callable's int (an error code of the ABI); a code outside the accepted set returns the documented
// error and the callable is not called.  A generic lambda is instantiated for EVERY tag its dispatcher can pass, so a
// site picks the dispatcher whose tag set is exactly its kernel set (with_elem + Vec<T>::N where only the vector form
// exists, with_elem_vec where the scalar form exists too).  TSG_HIP / TSG_CHECK_LAUNCH return from the lambda.
#pragma once
#include <type_traits>
#include "tsg_common.h"

namespace tsg {

template <typename T> struct type_tag { typedef T type; };
template <int N> using int_tag = std::integral_constant<int, N>;
template <bool B> using bool_tag = std::integral_constant<bool, B>;

// elements of one 16-byte access for a dtype code (4 for anything that is not bf16, as the launchers always had it)
static inline int native_vec(int dtype) { return dtype == TSG_BF16 ? Vec<bf16_t>::N : Vec<float>::N; }

template <typename F> static inline int with_elem(int dtype, F&& f) {
  if (dtype == TSG_F32) return f(type_tag<float>());
  if (dtype == TSG_BF16) return f(type_tag<bf16_t>());
  return TSG_E_DTYPE;
}

template <typename F> static inline int with_flag(bool b, F&& f) {
  return b ? f(bool_tag<true>()) : f(bool_tag<false>());
}

// f(type_tag<T>, int_tag<V>): V = Vec<T>::N when `vec`, else 1
template <typename F> static inline int with_elem_vec(int dtype, bool vec, F&& f) {
  return with_elem(dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    return vec ? f(t, int_tag<Vec<T>::N>()) : f(t, int_tag<1>());
  });
}

template <typename F> static inline int with_label(int ltype, F&& f) {
  if (ltype == TSG_I64) return f(int_tag<TSG_I64>());
  if (ltype == TSG_U8) return f(int_tag<TSG_U8>());
  return TSG_E_DTYPE;
}

// f(int_tag<N>) for the N of Ns... that equals v; TSG_E_SHAPE when there is none
template <int... Ns, typename F> static inline int with_int(int v, F&& f) {
  int r = TSG_E_SHAPE;
  (void)((v == Ns ? (r = f(int_tag<Ns>()), true) : false) || ...);
  return r;
}

}  // namespace tsg
