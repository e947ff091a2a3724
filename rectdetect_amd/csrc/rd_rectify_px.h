// rectdetect-mi355x: a pixel of a rectified patch on the device - the source frame, the conversion of a tap and the 8.8 blend of the contract in
// include/rectdetect_hip.h ("rectified patches"), shared by the kernels that sample the inside of a quad: k_rectify (rd_k_rectify.hip) and k_signature
// (rd_k_match.hip).  Nothing here may reorder or contract the arithmetic (-ffp-contract=off, see rd_device.h).
#pragma once
#include "rd_device.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"

namespace {

struct RectifySrc { const uint8_t *pl[3]; int pitch[3]; int iw, ih; };

// BT.601 limited range, OpenCV's fixed point (the conversion contract in rectdetect_hip.h; rd_k_front.hip has the same lines for the detector's front end)
__device__ __forceinline__ void yuv_bgr(int Y, int U, int V, int &b, int &g, int &r) {
  const int u = U - 128, v = V - 128, yy = max(Y - 16, 0) * 1220542;
  r = min(max((yy + 1673527 * v + (1 << 19)) >> 20, 0), 255);
  g = min(max((yy - 852492 * v - 409993 * u + (1 << 19)) >> 20, 0), 255);
  b = min(max((yy + 2116026 * u + (1 << 19)) >> 20, 0), 255);
}

// (B, G, R) of source pixel (x, y), 0 <= x < iw, 0 <= y < ih: bytes from the caller's pitch
template <int FMT> __device__ __forceinline__ void tap(const RectifySrc &S, int x, int y, int (&c)[3]) {
  if (FMT <= RD_PIX_RGBA) {
    const int bpp = (FMT == RD_PIX_BGR || FMT == RD_PIX_RGB) ? 3 : 4;
    const uint8_t *q = S.pl[0] + (size_t)y * S.pitch[0] + (size_t)x * bpp;
    const int v0 = q[0], v1 = q[1], v2 = q[2];
    if (FMT == RD_PIX_BGR || FMT == RD_PIX_BGRA) { c[0] = v0; c[1] = v1; c[2] = v2; }
    else { c[0] = v2; c[1] = v1; c[2] = v0; }
  } else {
    const int Y = S.pl[0][(size_t)y * S.pitch[0] + x];
    int U, V;
    if (FMT == RD_PIX_NV12) {
      const uint8_t *q = S.pl[1] + (size_t)(y >> 1) * S.pitch[1] + (size_t)(x >> 1) * 2;
      U = q[0]; V = q[1];
    } else {
      U = S.pl[1][(size_t)(y >> 1) * S.pitch[1] + (x >> 1)];
      V = S.pl[2][(size_t)(y >> 1) * S.pitch[2] + (x >> 1)];
    }
    yuv_bgr(Y, U, V, c[0], c[1], c[2]);
  }
}

// floor(v * 256) clamped to [0, hi] in double (anything not above 0, a NaN too, gives 0), then an integer
__device__ __forceinline__ int fix8(double v, double hi) {
  double q = floor(v * 256.0);
  q = q > 0.0 ? q : 0.0;
  q = q < hi ? q : hi;
  return (int)q;
}

template <int FMT> __device__ __forceinline__ void patch_pixel(const RectifySrc &S, const rdk::RectifyQuad &Q, int i, int j, int pw, int ph, uint8_t (&o)[3]) {
  const double s = ((double)i + 0.5) / (double)pw, t = ((double)j + 0.5) / (double)ph;
  const double w = (Q.c[6] * s + Q.c[7] * t) + 1.0;
  const double x = ((Q.c[0] * s + Q.c[1] * t) + Q.c[2]) / w;
  const double y = ((Q.c[3] * s + Q.c[4] * t) + Q.c[5]) / w;
  const int xi = fix8(x, (double)(S.iw - 1) * 256.0), yi = fix8(y, (double)(S.ih - 1) * 256.0);
  const int x0 = xi >> 8, fx = xi & 255, x1 = min(x0 + 1, S.iw - 1);
  const int y0 = yi >> 8, fy = yi & 255, y1 = min(y0 + 1, S.ih - 1);
  int p00[3], p10[3], p01[3], p11[3];
  tap<FMT>(S, x0, y0, p00); tap<FMT>(S, x1, y0, p10); tap<FMT>(S, x0, y1, p01); tap<FMT>(S, x1, y1, p11);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int top = p00[c] * (256 - fx) + p10[c] * fx;
    const int bot = p01[c] * (256 - fx) + p11[c] * fx;
    o[c] = (uint8_t)((top * (256 - fy) + bot * fy + 32768) >> 16);
  }
}

}  // namespace
