// Shared by the bf16 MFMA kernels: the operand vector types, the packed-bf16 helpers of their staging and epilogue code, and
// the fragment order of the prepared 3x3 filter.  A new MFMA kernel file includes this header instead of copying from a
// neighbour; tile constants, geometry structs and kernels stay in their own files under their own prefixes.
#pragma once
#include "tsg_common.h"

namespace tsg {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;     // A / B operand of v_mfma_f32_32x32x16_bf16
typedef __attribute__((ext_vector_type(16))) float f32x16;     // its accumulator
// what ds_read_b64_tr_b16 (__builtin_amdgcn_ds_read_tr16_b64_v4i16) returns: half an operand, from an LDS pointer
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef v4i16 __attribute__((address_space(3))) lds_v4i16;
// LDS images that are written with 16- and 32-bit stores and read back as 32- and 128-bit fragments: every
// access goes through may_alias types so that type-based alias analysis cannot reorder or drop them.
typedef uint32_t __attribute__((may_alias)) lds_u32;
typedef uint16_t __attribute__((may_alias)) lds_u16;
typedef bf16x8 __attribute__((may_alias)) lds_bf16x8;

// bf16(bf16 a + bf16 b) per element, fp32 add: what the eager `a + b` of two bf16 tensors computes
__device__ __forceinline__ uint4 add_bf16x8(uint4 a, uint4 b) {
  const uint32_t x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = pack2_bf16(__uint_as_float(x[i] << 16) + __uint_as_float(y[i] << 16),
                      __uint_as_float(x[i] & 0xffff0000u) + __uint_as_float(y[i] & 0xffff0000u));
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// Normalise-on-load: relu(a x + b) on eight packed bf16 with the values tsg_bn_apply_fwd would have stored (same fma, same
// rounding to bf16), so a convolution can read the input of a BatchNorm + ReLU and the normalised activation is never
// written or re-read.  The core takes the eight a and the eight b behind two pointers (conv3g: rows staged in LDS).
__device__ __forceinline__ uint4 affine_relu(uint4 v, const float* __restrict__ a, const float* __restrict__ b) {
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x0 = __uint_as_float(w[i] << 16), x1 = __uint_as_float(w[i] & 0xffff0000u);
    const float y0 = fmaf(x0, a[2 * i], b[2 * i]), y1 = fmaf(x1, a[2 * i + 1], b[2 * i + 1]);
    w[i] = pack2_bf16(y0 > 0.f ? y0 : 0.f, y1 > 0.f ? y1 : 0.f);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// a, b = rows 0 and 1 of an ab pack [2][C] (16-byte aligned) at channels part8 .. part8 + 7, fetched by two float4 loads
// per row (conv64, conv3wrw)
__device__ __forceinline__ uint4 affine_relu(uint4 v, const float* __restrict__ ab, int C, int part8) {
  const float4 a0 = *reinterpret_cast<const float4*>(ab + part8), a1 = *reinterpret_cast<const float4*>(ab + part8 + 4);
  const float4 b0 = *reinterpret_cast<const float4*>(ab + C + part8), b1 = *reinterpret_cast<const float4*>(ab + C + part8 + 4);
  const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  return affine_relu(v, a, b);
}

// ---- the prepared 3x3 filter: bf16 in MFMA fragment order
//   out[oc tile][chunk][tap][ocb][lane][e] = W'[oc = tile BN + ocb 32 + (lane & 31)][tap][ci = chunk 16 + (lane >> 5) 8 + e]
// BN = output channels per block of the kernel that will read it (32, 64 or 128), Ci = input channels of the convolution
// that will run.  tsg_conv3x3_gen_prep_filter and the weight-shadow refresh (csrc/sgd.hip) write this image; conv3g_fwd_k,
// conv3h_fwd_k, conv3s2d_k and dil3_fwd_k read it linearly: the [tap][ocb][lane][8] slab of one (tile, chunk) is 9 BN 16
// consecutive elements, an A fragment 1 KB of them.  frag_offset and frag_decode state this order; g3_prep_filter_k
// (csrc/conv3g.hip) keeps a 64-bit spelling of the decode, which must follow any change made here.
__device__ __forceinline__ int64_t frag_offset(int oc, int tap, int ci, int Ci, int BN) {
  const int nch = Ci >> 4, ocb_n = BN >> 5;
  const int tile = oc / BN, rem = oc - tile * BN, ocb = rem >> 5, ln = ((ci >> 3) & 1) * 32 + (rem & 31);
  return ((((int64_t)(tile * nch + (ci >> 4)) * 9 + tap) * ocb_n + ocb) * 64 + ln) * 8 + (ci & 7);
}
// the inverse: 16-byte vector `vec` of the image (element offset vec 8) holds W'[oc][tap][ci0 .. ci0 + 7]
struct FragPos {
  int tile, chunk, tap, ocb, lane;
  __device__ __forceinline__ int oc(int BN) const { return tile * BN + ocb * 32 + (lane & 31); }
  __device__ __forceinline__ int ci0() const { return chunk * 16 + (lane >> 5) * 8; }
};
// nch = Ci / 16 chunks, ocb_n = BN / 32 channel blocks
template <typename I>
__device__ __forceinline__ FragPos frag_decode(I vec, int nch, int ocb_n) {
  const int lane = (int)(vec & 63);
  I r = vec >> 6;
  const int ocb = (int)(r % ocb_n); r /= ocb_n;
  const int tap = (int)(r % 9); r /= 9;
  const int chunk = (int)(r % nch), tile = (int)(r / nch);
  return {tile, chunk, tap, ocb, lane};
}

}  // namespace tsg
