// Weight gradient of the whole-map 1x1 / padding 0 convolutions, stride 1 or 2, channels_last bf16 (the bottleneck 1x1 layers
// and `downsample` of furnace/base_model/resnet.py, RefineResidual.conv_1x1 / FeatureFusion.conv_1x1 of
// furnace/seg_opr/seg_oprs.py, SpatialPath.conv_1x1 of the bisenet network.py):
//
//     dw[co][ci] = sum_p dy[p][co] * x[row(p)][ci],   p = (b OH + oh) OW + ow,   row(p) = (b H + s oh) W + s ow
//
// A GEMM with M = C_out, N = C_in and K = pixels whose two operands both have the reduction index as their ROW and the
// channels contiguous: the situation of conv3_wrw_gen_k (csrc/conv3wrw.hip), and the same answer.  A chunk of PW_KC = 64
// pixels is staged pixel-major in LDS exactly as it comes from HBM (16-byte copies, rows of PW_RBE = 96 elements per 64
// channels: 64 + 32 pad, 192 B, conv3wrw's T3_RBE -- the two 16-lane groups of a transposing read hit 64 distinct banks) and
// ds_read_b64_tr_b16 forms the K-major fragments of v_mfma_f32_32x32x16_bf16.  The stride-2 sub-sampling is part of the
// address of a pixel's row: no gathered copy of x exists.
//
// Block = 4 waves = one (C_out tile, C_in tile, pixel slice) of csrc/pw_geom.h; the tiles are 64 or 128 channels wide (128
// where that divides the channel count, so no tile is ragged) and a wave owns a quarter: MI x NI accumulators of 32 x 32.
// The next chunk is fetched into registers by raw buffer loads while the current chunk's MFMAs run.  Each operand has ONE
// descriptor per block: base = the tile's first channel of the operand's first pixel, num_records = the bytes from there to
// the operand's end.  A pixel's offset is a 32-bit byte count (an operand has < 2^31 elements) kept up to date by adding a
// constant per chunk plus two carries (end of an output row, end of an image), and a pixel at or past the slice's end gets
// an offset beyond num_records, which the buffer unit answers with zeros without touching memory.
//
// S > 1 slices: every block writes its fp32 partial [slice][C_out][C_in] to the workspace and pw_wgrad_fold_k adds them in
// fp64 in slice order, rounding once.  S == 1: the block writes dw itself.  No atomics, no hand-offs between blocks, every
// loop bound comes from the launch geometry: bit-identical from run to run.
#include "tsg_mfma.h"
#include "pw_geom.h"

namespace tsg {

constexpr int PW_RBE = 96;                          // bf16 elements per pixel row of a 64-channel LDS image (= T3_RBE)
constexpr int PW_SUB = PW_KC * PW_RBE;              // elements of one 64-channel image of a chunk: 12,288 B
constexpr uint32_t PW_OOB = 0xffffffc0u;            // >= num_records of any accepted operand (<= 2^32 - 128 bytes), and no
                                                    // dword of a 16-byte access that starts here wraps

// MI, NI in {1, 2}: the block tile is 64 MI output channels x 64 NI input channels; LDS 24,576 .. 49,152 B
template <int MI, int NI>
__global__ __launch_bounds__(256, 2) void pw_wgrad_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                     float* __restrict__ dw, float* __restrict__ part, PwGeom g) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[(MI + NI) * PW_SUB];
  bf16_t* dyL = lds;                                  // [MI][64 pixels][PW_RBE]
  bf16_t* xL = lds + MI * PW_SUB;                     // [NI][64 pixels][PW_RBE]
  int tm, tn, slice;
  pw_block(g, blockIdx.x, &tm, &tn, &slice);
  if (slice >= g.S) return;                           // the grid rounds S up to the 8 XCDs (whole block: no barrier missed)
  int64_t p0_, p1_;
  pw_slice_range(g, slice, &p0_, &p1_);
  const int p0 = (int)p0_, p1 = (int)p1_;             // P < 2^25
  const int nch = (p1 - p0 + PW_KC - 1) / PW_KC;
  const int oc0 = tm * 64 * MI, ci0 = tn * 64 * NI;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wh = wave & 1;            // C_out half, C_in half of the tile
  const int half = lane >> 5, sub = (lane >> 4) & 1, i16 = lane & 15;

  // ---- fetch: chunk = (pixel, 8-channel part); thread -> part tid & 7, pixels (tid >> 3) and (tid >> 3) + 32 of a chunk
  const int spart = tid & 7, spix = tid >> 3;
  const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(x + ci0), 0, (int)(uint32_t)((g.B * g.H * g.W * g.Cin - ci0) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rd_ = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(dy + oc0), 0, (int)(uint32_t)((g.P * g.Cout - oc0) * 2), 0x00020000);
  const PwSteps steps = pw_steps(g);                  // one chunk further, as byte steps with two carries (pw_geom.h)
  PwPix px[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    px[u] = pw_pix(g, p0 + spix + 32 * u);
    px[u].xo += spart * 16u; px[u].dyo += spart * 16u;
  }
  uint4 rd[2 * MI], rx[2 * NI];
  auto fetch = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bool ok = px[u].p < p1;
#pragma unroll
      for (int j = 0; j < MI; ++j) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rd_, (int)(ok ? px[u].dyo + 128u * j : PW_OOB), 0, 0);
        rd[u * MI + j] = make_uint4(v.x, v.y, v.z, v.w);
      }
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rx_, (int)(ok ? px[u].xo + 128u * j : PW_OOB), 0, 0);
        rx[u * NI + j] = make_uint4(v.x, v.y, v.z, v.w);
      }
      pw_advance(g, steps, &px[u]);
    }
  };

  // ---- fragments: lane 4 q + r of a 16-lane group points at (pixel k0 + q, channels c0 + 4 r ..) and receives channel
  // c0 + (lane & 15) at pixels k0 .. k0 + 3 (conv3wrw.hip, variant 2): two reads make one operand of 8 pixels
  const int frow = (8 * half + (i16 >> 2)) * PW_RBE + 16 * sub + 4 * (i16 & 3);
  const lds_v4i16* afr[MI];
  const lds_v4i16* bfr[NI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int c = (wm * MI + i) * 32;                 // channel of the tile
    afr[i] = (const lds_v4i16*)(dyL + (c >> 6) * PW_SUB + frow + (c & 63));
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int c = (wh * NI + j) * 32;
    bfr[j] = (const lds_v4i16*)(xL + (c >> 6) * PW_SUB + frow + (c & 63));
  }

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  union Frag { v4i16 q[2]; bf16x8 v; };
  fetch();
  for (int c = 0; c < nch; ++c) {
    __syncthreads();                                  // the previous chunk's fragment reads are done
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int j = 0; j < MI; ++j)
        *reinterpret_cast<uint4*>(dyL + j * PW_SUB + (spix + 32 * u) * PW_RBE + spart * 8) = rd[u * MI + j];
#pragma unroll
      for (int j = 0; j < NI; ++j)
        *reinterpret_cast<uint4*>(xL + j * PW_SUB + (spix + 32 * u) * PW_RBE + spart * 8) = rx[u * NI + j];
    }
    __syncthreads();
    fetch();                                          // in flight during the MFMAs; past the slice every lane is out of bounds
#pragma unroll
    for (int ks = 0; ks < PW_KC / 16; ++ks) {
      Frag fa[MI], fb[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        fa[i].q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(afr[i] + (ks * 16 + 0) * (PW_RBE / 4)));
        fa[i].q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(afr[i] + (ks * 16 + 4) * (PW_RBE / 4)));
      }
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        fb[j].q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(bfr[j] + (ks * 16 + 0) * (PW_RBE / 4)));
        fb[j].q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(bfr[j] + (ks * 16 + 4) * (PW_RBE / 4)));
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i].v, fb[j].v, acc[i][j], 0, 0, 0);
    }
  }
  // acc[i][j][r]: co = oc0 + 32 (wm MI + i) + (r & 3) + 8 (r >> 2) + 4 half, ci = ci0 + 32 (wh NI + j) + (lane & 31)
  float* out = g.S > 1 ? part + (int64_t)slice * g.Cout * g.Cin : dw;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = oc0 + 32 * (wm * MI + i) + (r & 3) + 8 * (r >> 2) + 4 * half;
        out[(int64_t)co * g.Cin + ci0 + 32 * (wh * NI + j) + (lane & 31)] = acc[i][j][r];
      }
}

// dw = sum over the S partials, fp64, in slice order, one rounding.  T = 1, 4 or 16 row lanes share one float4 of the
// output: lane t adds slices t, t + T, .. in that order and the T sums are added in lane order (fixed by S alone).
__global__ __launch_bounds__(256) void pw_wgrad_fold_k(const float* __restrict__ part, float* __restrict__ dw, int S, int T,
                                                       int n4) {
  __shared__ double sm[256][4];
  const int outs = 256 / T;                           // float4 outputs per block; n4 = C_out C_in / 4 is a multiple of 256
  const int t = threadIdx.x / outs, o = threadIdx.x - t * outs;
  const int q = blockIdx.x * outs + o;
  const float4* src = reinterpret_cast<const float4*>(part) + q;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int s0 = t; s0 < S; s0 += 8 * T) {             // 8 predicated loads in flight, summed in order
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int s = s0 + u * T;
      v[u] = src[(int64_t)(s < S ? s : t) * n4];
      if (s >= S) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) { a0 += (double)v[u].x; a1 += (double)v[u].y; a2 += (double)v[u].z; a3 += (double)v[u].w; }
  }
  if (T > 1) {
    sm[threadIdx.x][0] = a0; sm[threadIdx.x][1] = a1; sm[threadIdx.x][2] = a2; sm[threadIdx.x][3] = a3;
    __syncthreads();
    if (t == 0)
      for (int k = 1; k < T; ++k) {
        const double* r = sm[k * outs + o];
        a0 += r[0]; a1 += r[1]; a2 += r[2]; a3 += r[3];
      }
  }
  if (t == 0) reinterpret_cast<float4*>(dw)[q] = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
}

}  // namespace tsg

using namespace tsg;

extern "C" {

int tsg_pw_wgrad_supported(int dtype, int Cin, int Cout, int64_t B, int H, int W, int stride) {
  return dtype == TSG_BF16 && pw_shape_ok(Cin, Cout, B, H, W, stride);
}

int tsg_pw_wgrad_slices(int Cin, int Cout, int64_t B, int H, int W, int stride) {
  PwGeom g;
  return pw_geom(&g, Cin, Cout, B, H, W, stride) ? g.S : 0;
}

size_t tsg_pw_wgrad_ws_bytes(int Cin, int Cout, int64_t B, int H, int W, int stride) {
  PwGeom g;
  return pw_geom(&g, Cin, Cout, B, H, W, stride) ? (size_t)pw_ws_bytes(g) : 0;
}

int tsg_pw_wgrad(const void* x, const void* dy, float* dw, int dtype, int64_t B, int H, int W, int Cin, int Cout,
                 int stride, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !dw) return TSG_E_NULL;
  if (dtype != TSG_BF16) return TSG_E_DTYPE;
  PwGeom g;
  if (!pw_geom(&g, Cin, Cout, B, H, W, stride)) return TSG_E_SHAPE;
  if (g.S > 1) {
    if (!ws) return TSG_E_NULL;
    if (ws_bytes < pw_ws_bytes(g)) return TSG_E_WS;
    if (!aligned16(ws)) return TSG_E_ALIGN;
  }
  if (!aligned16(x) || !aligned16(dy) || !aligned16(dw)) return TSG_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.grid), block(256);
  const bf16_t* xp = (const bf16_t*)x;
  const bf16_t* dp = (const bf16_t*)dy;
  if (g.bm == 128 && g.bn == 128) hipLaunchKernelGGL((pw_wgrad_k<2, 2>), grid, block, 0, st, xp, dp, dw, (float*)ws, g);
  else if (g.bm == 128) hipLaunchKernelGGL((pw_wgrad_k<2, 1>), grid, block, 0, st, xp, dp, dw, (float*)ws, g);
  else if (g.bn == 128) hipLaunchKernelGGL((pw_wgrad_k<1, 2>), grid, block, 0, st, xp, dp, dw, (float*)ws, g);
  else hipLaunchKernelGGL((pw_wgrad_k<1, 1>), grid, block, 0, st, xp, dp, dw, (float*)ws, g);
  TSG_CHECK_LAUNCH();
  if (g.S > 1) {
    const int T = g.S >= 64 ? 16 : g.S >= 16 ? 4 : 1;
    const int n4 = g.Cout * g.Cin / 4;
    hipLaunchKernelGGL(pw_wgrad_fold_k, dim3((unsigned)(n4 / (256 / T))), block, 0, st, (const float*)ws, dw, g.S, T, n4);
    TSG_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
