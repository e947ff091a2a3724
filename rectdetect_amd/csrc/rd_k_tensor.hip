// rectdetect-mi355x: model-ready tensors for gfx950 - the rectifier's patches in the element type, layout and channel order of the next model, normalised and box-
// filtered, from one launch.  The arithmetic is the contract in include/rectdetect_hip.h ("model-ready tensors"); a patch pixel's bytes come from patch_pixel<FMT>
// (rd_rectify_px.h), the very function k_rectify calls, so the two kernels cannot disagree on a tap.  Nothing here may reorder or contract the arithmetic
// (-ffp-contract=off, see rd_device.h): the scale and the bias are a multiplication and an addition, each rounded.
//
// Launch shape: k_rectify's (rd_k_rectify.hip) - one launch per job, quad = blockIdx.z, a block is ONE wave covering 32 x 8 PATCH pixels, no LDS, no barrier.
// With m = 1 a lane is a thread of k_rectify: 4 neighbouring elements of a row in all C channels.  With m > 1 that thread is spread over m x m neighbouring lanes:
// each samples ONE patch pixel of each of the 4 outputs, the box sums are made by log2(m * m) exchanges inside the group (integer sums: any order is exact), and
// the group's first lane converts and stores.  A wave then makes (32 / m) x (8 / m) outputs and a job has m x m times the waves - a job is small (ten 128 x 128
// outputs are 640 waves at m = 1, fewer than the device has SIMDs), so the extra taps run side by side instead of one after the other: DESIGN.md, "Model-ready
// tensors", has both forms' figures.
// Templates: the pixel format, the dtype, and the STORE SHAPE - three planes (NCHW, C = 3), interleaved (NHWC, C = 3), one plane (GRAY: both layouts are the same
// bytes) - 6 x 4 x 3 = 72 instantiations.  Uniform run-time values: the oversampling m (shifts and masks of the lane index, the exchange loop's bound) and BGR against RGB (which byte goes to which sum).
// Stores: 4 elements of a plane as one 4, 8 or 16 byte store, the 12 interleaved elements as dwords, 8 or 16 byte words - whatever the address is aligned to -
// and element by element in a row's tail (pw % 4) or at an address that is not dword-aligned.
#include <stdio.h>
#include <stdlib.h>
#include "rd_device.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"

#include "rd_rectify_px.h"

namespace {

enum { ST_PLANES3 = 0, ST_INTERLEAVED3 = 1, ST_PLANE1 = 2 };

constexpr int elem_size(int dt) { return dt == RD_TENSOR_U8 ? 1 : (dt == RD_TENSOR_F32 ? 4 : 2); }

// step 4 of the contract: the element's bits (in the low 8, 16 or 32 bits) from its box sum
template <int DT> __device__ __forceinline__ uint32_t element_bits(int sum, int m, int sh, float inv, float scale, float bias) {
  if (DT == RD_TENSOR_U8) return (uint32_t)((sum + ((m * m) >> 1)) >> sh);
  float v = (float)sum * inv;
  v = v * scale;
  v = v + bias;
  const uint32_t u = __float_as_uint(v);
  if (DT == RD_TENSOR_F32) return u;
  if (DT == RD_TENSOR_F16) return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v);      // v_cvt_f16_f32: nearest even, overflow to infinity, subnormals kept
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

template <int ES> __device__ __forceinline__ void store_element(uint8_t *p, uint32_t bits) {
  if (ES == 1) *p = (uint8_t)bits;
  else if (ES == 2) *(uint16_t *)p = (uint16_t)bits;
  else *(uint32_t *)p = bits;
}

// 4 * ES bytes: the elements e0 .. e3, side by side
template <int ES> __device__ __forceinline__ void store_four(uint8_t *p, uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3) {
  if (ES == 1) *(uint32_t *)p = e0 | (e1 << 8) | (e2 << 16) | (e3 << 24);
  else if (ES == 2) *(uint2 *)p = make_uint2(e0 | (e1 << 16), e2 | (e3 << 16));
  else *(uint4 *)p = make_uint4(e0, e1, e2, e3);
}

template <int FMT, int DT, int ST> __global__ __launch_bounds__(64) void k_rectify_tensor(uint8_t *out, PixFrame S, const rdk::RectifyQuad *quads, int pw, int ph, rd_tensor_spec T) {
  constexpr int C = ST == ST_PLANE1 ? 1 : 3, ES = elem_size(DT);
  // m * m neighbouring lanes make one thread of the classic kernel: lane `sub` of the group samples patch pixel (di, dj) of each of the group's 4 outputs
  const int m = T.oversample, sh = m == 1 ? 0 : (m == 2 ? 2 : 4), lm = sh >> 1, lper = 3 - lm, per = 1 << lper;      // per x per groups in a wave: 8, 4 or 2
  const int lane = threadIdx.y * 8 + threadIdx.x, g = lane >> sh, sub = lane & ((1 << sh) - 1);
  const int di = sub & (m - 1), dj = sub >> lm;
  const int i0 = (blockIdx.x * per + (g & (per - 1))) * 4, j = blockIdx.y * per + (g >> lper);
  if (i0 >= pw || j >= ph) return;      // (a whole group at a time: the exchanges below stay inside a group)
  const rdk::RectifyQuad Q = quads[blockIdx.z];
  const float inv = m == 1 ? 1.0f : (m == 2 ? 0.25f : 0.0625f);      // 1.0f / (m * m), without a division's fused steps in the instruction stream
  const bool rgb = T.channels == RD_TENSOR_RGB;
  const int cnt = min(4, pw - i0);      // elements of this group per channel (fewer than 4: the row's tail)
  int sum[4][C];
#pragma unroll
  for (int k = 0; k < 4; k++) {
#pragma unroll
    for (int c = 0; c < C; c++) sum[k][c] = 0;
    if (Q.status && k < cnt) {
      uint8_t o[3];
      patch_pixel<FMT>(S, Q, (i0 + k) * m + di, j * m + dj, pw * m, ph * m, o);
      if constexpr (C == 1) sum[k][0] = (29 * o[0] + 150 * o[1] + 77 * o[2] + 128) >> 8;
      else { sum[k][0] = rgb ? o[2] : o[0]; sum[k][1] = o[1]; sum[k][2] = rgb ? o[0] : o[2]; }
    }
  }
  for (int d = (1 << sh) >> 1; d >= 1; d >>= 1) {      // the box sums: integers, any order gives the same result
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int c = 0; c < C; c++) sum[k][c] += __shfl_xor(sum[k][c], d, 64);
  }
  if (sub != 0) return;      // the group's first lane converts and stores
  uint32_t e[4][C];
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int c = 0; c < C; c++) e[k][c] = Q.status && k < cnt ? element_bits<DT>(sum[k][c], m, sh, inv, T.scale[c], T.bias[c]) : 0u;      // (an invalid quad: zero bytes from the same launch)
  uint8_t *quad = out + (size_t)blockIdx.z * ((size_t)pw * ph * (C * ES));
  if constexpr (ST != ST_INTERLEAVED3) {
#pragma unroll
    for (int c = 0; c < C; c++) {
      uint8_t *dst = quad + (((size_t)c * ph + j) * pw + i0) * ES;
      if (cnt == 4 && ((uintptr_t)dst & (4 * ES - 1)) == 0) store_four<ES>(dst, e[0][c], e[1][c], e[2][c], e[3][c]);
      else {
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < cnt) store_element<ES>(dst + k * ES, e[k][c]);
      }
    }
  } else {
    uint8_t *dst = quad + ((size_t)j * pw + i0) * (3 * ES);
    if (cnt == 4 && ((uintptr_t)dst & 3) == 0) {      // 12 elements = 3 ES dwords
      constexpr int NW = 3 * ES;
      uint32_t w[NW];
#pragma unroll
      for (int q = 0; q < NW; q++) {
        if constexpr (ES == 1) w[q] = e[(4 * q) / 3][(4 * q) % 3] | (e[(4 * q + 1) / 3][(4 * q + 1) % 3] << 8) | (e[(4 * q + 2) / 3][(4 * q + 2) % 3] << 16) | (e[(4 * q + 3) / 3][(4 * q + 3) % 3] << 24);
        else if constexpr (ES == 2) w[q] = e[(2 * q) / 3][(2 * q) % 3] | (e[(2 * q + 1) / 3][(2 * q + 1) % 3] << 16);
        else w[q] = e[q / 3][q % 3];
      }
      if (NW % 4 == 0 && ((uintptr_t)dst & 15) == 0) {
#pragma unroll
        for (int q = 0; q < NW; q += 4) *(uint4 *)(dst + 4 * q) = make_uint4(w[q], w[(q + 1) % NW], w[(q + 2) % NW], w[(q + 3) % NW]);
      } else if (NW % 2 == 0 && ((uintptr_t)dst & 7) == 0) {
#pragma unroll
        for (int q = 0; q < NW; q += 2) *(uint2 *)(dst + 4 * q) = make_uint2(w[q], w[(q + 1) % NW]);
      } else {
#pragma unroll
        for (int q = 0; q < NW; q++) *(uint32_t *)(dst + 4 * q) = w[q];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (k < cnt) {
#pragma unroll
          for (int c = 0; c < 3; c++) store_element<ES>(dst + (3 * k + c) * ES, e[k][c]);
        }
    }
  }
}

template <class F> bool dispatch_dtype(int dt, F &&f) {
  switch (dt) {
    case RD_TENSOR_U8: f(std::integral_constant<int, RD_TENSOR_U8>()); return true;
    case RD_TENSOR_F16: f(std::integral_constant<int, RD_TENSOR_F16>()); return true;
    case RD_TENSOR_BF16: f(std::integral_constant<int, RD_TENSOR_BF16>()); return true;
    case RD_TENSOR_F32: f(std::integral_constant<int, RD_TENSOR_F32>()); return true;
    default: return false;
  }
}
template <class F> void dispatch_store(int st, F &&f) {
  if (st == ST_PLANES3) f(std::integral_constant<int, ST_PLANES3>());
  else if (st == ST_INTERLEAVED3) f(std::integral_constant<int, ST_INTERLEAVED3>());
  else f(std::integral_constant<int, ST_PLANE1>());
}

}  // namespace

namespace rdk {

void rectify_tensor(hipStream_t s, void *out, int fmt, const PixFrame &S, const RectifyQuad *quads, int n, int pw, int ph, const rd_tensor_spec &spec) {
  if (n <= 0) return;
  const int per = 8 / spec.oversample;      // a wave makes 4 per x per elements per channel
  const dim3 block(8, 8), grid((pw + 4 * per - 1) / (4 * per), (ph + per - 1) / per, n);
  const int st = spec.channels == RD_TENSOR_GRAY ? ST_PLANE1 : (spec.layout == RD_TENSOR_NCHW ? ST_PLANES3 : ST_INTERLEAVED3);
  const bool ok = dispatch(fmt, [&](auto f) {
    if (!dispatch_dtype(spec.dtype, [&](auto d) {
          dispatch_store(st, [&](auto l) { hipLaunchKernelGGL((k_rectify_tensor<f.value, d.value, l.value>), grid, block, 0, s, (uint8_t *)out, S, quads, pw, ph, spec); });
        })) {
      fprintf(stderr, "rdk::rectify_tensor: unknown dtype %d\n", spec.dtype); abort();      // (rd_rectifier_create_tensor refuses it first)
    }
  });
  if (!ok) { fprintf(stderr, "rdk::rectify_tensor: unknown pixel format %d\n", fmt); abort(); }      // (the entry points refuse it first)
}

}  // namespace rdk
