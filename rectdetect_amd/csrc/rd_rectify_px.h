// rectdetect-mi355x: a pixel of a rectified patch on the device - the map of the contract in include/rectdetect_hip.h ("rectified patches") from a patch pixel
// into the source frame, shared by the kernels that sample the inside of a quad: k_rectify (rd_k_rectify.hip) and k_signature (rd_k_match.hip).  The taps and
// their blend: rd_pix.h.  Nothing here may reorder or contract the arithmetic (-ffp-contract=off, see rd_device.h).
#pragma once
#include "rd_device.h"
#include "rd_kernels.h"
#include "rd_pix.h"

namespace {

using namespace rdpix;

template <int FMT> __device__ __forceinline__ void patch_pixel(const PixFrame &S, const rdk::RectifyQuad &Q, int i, int j, int pw, int ph, uint8_t (&o)[3]) {
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
  for (int c = 0; c < 3; c++) o[c] = (uint8_t)blend8(lerp8(p00[c], p10[c], fx), lerp8(p01[c], p11[c], fx), fy);
}

}  // namespace
