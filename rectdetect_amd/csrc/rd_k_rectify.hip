// rectdetect-mi355x: rectified patches for gfx950 - the inside of each quad of a job as an upright pw x ph BGR image (perspective warp, bilinear taps
// in 8.8 fixed point).  The arithmetic is the contract in include/rectdetect_hip.h ("rectified patches"); nothing here may reorder or contract it
// (-ffp-contract=off, see rd_device.h).
//
// Launch shape: one launch per job, quad = blockIdx.z.  A block is ONE wave of 8 x 8 threads and a thread makes 4 neighbouring pixels of a patch row, so
// a wave covers 32 x 8 patch pixels: a near-square footprint in the source under any rotation of the quad (its taps share cache lines in both directions), and
// its stores are 96 contiguous bytes per row.  The kernel uses no LDS and no barrier, so a larger block would buy nothing - while a job is small (ten 128 x 128
// patches are 640 waves) and latency-bound on its gathers: one-wave blocks let the dispatcher spread it over all 256 CUs.  DESIGN.md, "Rectified patches".
#include <stdio.h>
#include <stdlib.h>
#include "rd_device.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"

#include "rd_rectify_px.h"

namespace {

template <int FMT> __global__ __launch_bounds__(64) void k_rectify(uint8_t *out, PixFrame S, const rdk::RectifyQuad *quads, int pw, int ph) {
  const int i0 = (blockIdx.x * 8 + threadIdx.x) * 4, j = blockIdx.y * 8 + threadIdx.y;
  if (i0 >= pw || j >= ph) return;
  const rdk::RectifyQuad Q = quads[blockIdx.z];
  uint8_t *dst = out + ((size_t)blockIdx.z * ph + j) * ((size_t)pw * 3) + (size_t)i0 * 3;
  const int m = min(4, pw - i0);      // pixels of this thread (fewer than 4: the row's tail)
  uint8_t o[4][3];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    o[k][0] = o[k][1] = o[k][2] = 0;      // (an invalid quad: zeros from the same launch)
    if (Q.status && k < m) patch_pixel<FMT>(S, Q, i0 + k, j, pw, ph, o[k]);
  }
  if (m == 4 && ((uintptr_t)dst & 3) == 0) {      // 12 bytes as three aligned dwords (always, when pw is a multiple of 4 and `out` is dword-aligned)
    uint32_t *d4 = (uint32_t *)dst;
    d4[0] = o[0][0] | (o[0][1] << 8) | (o[0][2] << 16) | ((uint32_t)o[1][0] << 24);
    d4[1] = o[1][1] | (o[1][2] << 8) | (o[2][0] << 16) | ((uint32_t)o[2][1] << 24);
    d4[2] = o[2][2] | (o[3][0] << 8) | (o[3][1] << 16) | ((uint32_t)o[3][2] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < m) { dst[3 * k] = o[k][0]; dst[3 * k + 1] = o[k][1]; dst[3 * k + 2] = o[k][2]; }
  }
}

}  // namespace

namespace rdk {

void rectify(hipStream_t s, uint8_t *out, int fmt, const PixFrame &S, const RectifyQuad *quads, int n, int pw, int ph) {
  if (n <= 0) return;
  const dim3 block(8, 8), grid((pw + 31) / 32, (ph + 7) / 8, n);
  if (!dispatch(fmt, [&](auto f) { hipLaunchKernelGGL(k_rectify<f.value>, grid, block, 0, s, out, S, quads, pw, ph); })) {
    fprintf(stderr, "rdk::rectify: unknown pixel format %d\n", fmt); abort();      // (the entry points refuse it first)
  }
}

}  // namespace rdk
