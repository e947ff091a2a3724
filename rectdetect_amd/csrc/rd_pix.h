// rectdetect-mi355x: the six pixel formats (RD_PIX_*, the contract in include/rectdetect_hip.h) - the ONE place in csrc/ that knows what a format is: its
// properties, a frame in it, the conversion contract's arithmetic (YUV -> BGR, BGR -> YUV, the 8.8 fixed point of a bilinear tap) and the step from a format
// number at run time to a kernel's template argument.  A new format, or a correction to the contract, is made here; a kernel or a service asks, and compares a
// format number only where it names the one it means.  Nothing here may reorder or contract the arithmetic (-ffp-contract=off, see rd_device.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rectdetect_hip.h"

namespace rdpix {

// ---- properties: constant expressions of the format number, for a kernel's template argument and for the host at run time alike
constexpr bool is_yuv(int fmt) { return fmt >= RD_PIX_NV12; }                                               // Y and subsampled chroma planes; else packed B, G, R (, A)
constexpr int planes(int fmt) { return !is_yuv(fmt) ? 1 : (fmt == RD_PIX_NV12 ? 2 : 3); }
constexpr int bpp(int fmt) { return is_yuv(fmt) ? 1 : (fmt == RD_PIX_BGR || fmt == RD_PIX_RGB ? 3 : 4); }    // bytes per pixel of plane 0
constexpr bool rb_swapped(int fmt) { return fmt == RD_PIX_RGB || fmt == RD_PIX_RGBA; }                      // a packed pixel begins with R, not B

// ---- a frame where a job or a kernel reads or writes it: planes (those the format has not: NULL, 0), their row strides in bytes, its size in pixels
struct PixFrame { uint8_t *pl[3]; int pitch[3]; int iw, ih; };

// ---- the conversion contract
// YUV -> BGR: BT.601 limited range, OpenCV's fixed point
__device__ __forceinline__ void yuv_bgr(int Y, int U, int V, int &b, int &g, int &r) {
  const int u = U - 128, v = V - 128, yy = max(Y - 16, 0) * 1220542;
  r = min(max((yy + 1673527 * v + (1 << 19)) >> 20, 0), 255);
  g = min(max((yy - 852492 * v - 409993 * u + (1 << 19)) >> 20, 0), 255);
  b = min(max((yy + 2116026 * u + (1 << 19)) >> 20, 0), 255);
}
// BGR -> YUV (what a drawn or pasted colour becomes in NV12 / I420), host and device
__host__ __device__ __forceinline__ int bgr_y(int B, int G, int R) { return ((66 * R + 129 * G + 25 * B + 128) >> 8) + 16; }
__host__ __device__ __forceinline__ int bgr_u(int B, int G, int R) { return ((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128; }
__host__ __device__ __forceinline__ int bgr_v(int B, int G, int R) { return ((112 * R - 94 * G - 18 * B + 128) >> 8) + 128; }

// (B, G, R) of pixel (x, y) of F, 0 <= x < iw, 0 <= y < ih
template <int FMT> __device__ __forceinline__ void tap(const PixFrame &F, int x, int y, int (&c)[3]) {
  if (!is_yuv(FMT)) {
    const uint8_t *q = F.pl[0] + (size_t)y * F.pitch[0] + (size_t)x * bpp(FMT);
    const int v0 = q[0], v1 = q[1], v2 = q[2];
    if (!rb_swapped(FMT)) { c[0] = v0; c[1] = v1; c[2] = v2; }
    else { c[0] = v2; c[1] = v1; c[2] = v0; }
  } else {
    const int Y = F.pl[0][(size_t)y * F.pitch[0] + x];
    int U, V;
    if (FMT == RD_PIX_NV12) {
      const uint8_t *q = F.pl[1] + (size_t)(y >> 1) * F.pitch[1] + (size_t)(x >> 1) * 2;
      U = q[0]; V = q[1];
    } else {
      U = F.pl[1][(size_t)(y >> 1) * F.pitch[1] + (x >> 1)];
      V = F.pl[2][(size_t)(y >> 1) * F.pitch[2] + (x >> 1)];
    }
    yuv_bgr(Y, U, V, c[0], c[1], c[2]);
  }
}

// a bilinear tap's coordinate in 8.8 fixed point: floor(v * 256) clamped to [0, hi] in double (anything not above 0, a NaN too, gives 0), then an integer
__device__ __forceinline__ int fix8(double v, double hi) {
  double q = floor(v * 256.0);
  q = q > 0.0 ? q : 0.0;
  q = q < hi ? q : hi;
  return (int)q;
}
// ... and one channel of its four neighbours blended by the fractions fx, fy of 256: blend8(lerp8(p00, p10, fx), lerp8(p01, p11, fx), fy), rounded once.
// a, b: bytes or integers, by reference - bytes in memory are loaded where they are used, which keeps the kernels' schedules what they were
template <class T> __device__ __forceinline__ int lerp8(const T &a, const T &b, int f) { return a * (256 - f) + b * f; }
__device__ __forceinline__ int blend8(int top, int bot, int fy) { return (top * (256 - fy) + bot * fy + 32768) >> 16; }

// ---- dispatch on the host: f(std::integral_constant<int, fmt>) for a format number known at run time only, so that f - a generic lambda - names a kernel's
// instantiation with f's argument; false, and no call, for a number that is no format (the caller says what that means)
template <class F> inline bool dispatch(int fmt, F &&f) {
  switch (fmt) {
    case RD_PIX_BGR: f(std::integral_constant<int, RD_PIX_BGR>()); return true;
    case RD_PIX_RGB: f(std::integral_constant<int, RD_PIX_RGB>()); return true;
    case RD_PIX_BGRA: f(std::integral_constant<int, RD_PIX_BGRA>()); return true;
    case RD_PIX_RGBA: f(std::integral_constant<int, RD_PIX_RGBA>()); return true;
    case RD_PIX_NV12: f(std::integral_constant<int, RD_PIX_NV12>()); return true;
    case RD_PIX_I420: f(std::integral_constant<int, RD_PIX_I420>()); return true;
    default: return false;
  }
}

}  // namespace rdpix
