// rectdetect-mi355x: remapped frames for gfx950 - every pixel of an ow x oh BGR frame from the source position its table entry names (bilinear taps in 8.8
// fixed point), or the job's fill colour where the entry is outside.  The arithmetic is the contract in include/rectdetect_hip.h ("remapped frames"): the
// rectifier's taps and blend (rd_pix.h), integers only - the doubles of the lens were spent on the host, once, when the table was made (rd_remap_host.c).
//
// Launch shape: the rectifier's - one-wave blocks, a thread makes 4 neighbouring pixels of a row, 12 bytes go out as three aligned dwords when the destination
// allows, the tail bytewise, no LDS, no barrier - with another footprint of the wave: 32 x 2 threads, 128 x 2 output pixels.  A lens moves a pixel a long way
// but bends a row only slightly, so the wave's taps lie along two or three rows of the source, its table entries are 1 KB contiguous per row and its stores
// 384 contiguous bytes per row.  Measured at 1920 x 1080 against the rectifier's 8 x 8 threads and five other blocks of one to four waves: fastest on BGR and
// NV12 alike ("Remapped frames").  A thread's 4 table entries are 32 contiguous, 32-byte aligned bytes (the table's rows are padded to 4 entries on
// the device: rdk::remap_table_pitch), loaded as two dwordx4.
#include <stdio.h>
#include <stdlib.h>
#include "rd_device.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"

namespace {

using namespace rdpix;

// a tuning build may try another block (-DRD_REMAP_BX=8 -DRD_REMAP_BY=8, ...): BX x BY threads, whole waves
#ifndef RD_REMAP_BX
#define RD_REMAP_BX 32
#define RD_REMAP_BY 2
#endif
static_assert(RD_REMAP_BX * RD_REMAP_BY % 64 == 0 && RD_REMAP_BX * RD_REMAP_BY <= 1024, "a block is whole waves");

// Without a branch: an outside entry (-1, -1) taps pixel (0, 0) and then takes the fill colour, so the taps of a thread's 4 pixels are 16 independent loads in
// flight at once and not four dependent rounds behind four branches
template <int FMT> __device__ __forceinline__ void remap_pixel(const PixFrame &S, int xi, int yi, uint32_t fill, uint8_t (&o)[3]) {
  const bool inside = xi >= 0;
  xi = max(xi, 0); yi = max(yi, 0);
  const int x0 = xi >> 8, fx = xi & 255, x1 = min(x0 + 1, S.iw - 1);
  const int y0 = yi >> 8, fy = yi & 255, y1 = min(y0 + 1, S.ih - 1);
  int p00[3], p10[3], p01[3], p11[3];
  tap<FMT>(S, x0, y0, p00); tap<FMT>(S, x1, y0, p10); tap<FMT>(S, x0, y1, p01); tap<FMT>(S, x1, y1, p11);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int v = blend8(lerp8(p00[c], p10[c], fx), lerp8(p01[c], p11[c], fx), fy);
    o[c] = (uint8_t)(inside ? v : (int)(fill >> (8 * c)));
  }
}

// table: oh rows of tpitch entries (tpitch: ow rounded up to 4; the padding entries are outside), 256-byte aligned
typedef int entries2 __attribute__((ext_vector_type(4)));      // two entries: xi, yi, xi, yi

template <int FMT> __global__ __launch_bounds__(RD_REMAP_BX * RD_REMAP_BY) void k_remap(uint8_t *out, int out_pitch, PixFrame S, const entries2 *table, int tpitch, int ow, int oh, uint32_t fill) {
  const int i0 = (blockIdx.x * RD_REMAP_BX + threadIdx.x) * 4, j = blockIdx.y * RD_REMAP_BY + threadIdx.y;
  if (i0 >= ow || j >= oh) return;
  const entries2 *t = table + (((size_t)j * tpitch + i0) >> 1);      // i0 and tpitch are multiples of 4
  entries2 e01 = t[0], e23 = t[1];
  // the two loads stay two dwordx4 up here: left alone, the compiler cuts them into the dwords each pixel's branch uses and sinks some of them into the branches,
  // behind the taps' latency
  asm volatile("" : "+v"(e01), "+v"(e23));
  const int xi[4] = { e01.x, e01.z, e23.x, e23.z }, yi[4] = { e01.y, e01.w, e23.y, e23.w };
  uint8_t *dst = out + (size_t)j * out_pitch + (size_t)i0 * 3;
  const int m = min(4, ow - i0);      // pixels of this thread (fewer than 4: the row's tail, whose padding entries are outside)
  uint8_t o[4][3];
#pragma unroll
  for (int k = 0; k < 4; k++) remap_pixel<FMT>(S, xi[k], yi[k], fill, o[k]);
  if (m == 4 && ((uintptr_t)dst & 3) == 0) {      // 12 bytes as three aligned dwords (always, when `out` and out_pitch are dword-aligned and ow is a multiple of 4)
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

int remap_table_pitch(int ow) { return (ow + 3) & ~3; }

void remap(hipStream_t s, uint8_t *out, int out_pitch, int fmt, const PixFrame &S, const int32_t *table, int ow, int oh, uint32_t fill_bgr) {
  const dim3 block(RD_REMAP_BX, RD_REMAP_BY), grid((ow + 4 * RD_REMAP_BX - 1) / (4 * RD_REMAP_BX), (oh + RD_REMAP_BY - 1) / RD_REMAP_BY);
  const int tpitch = remap_table_pitch(ow);
  if (!dispatch(fmt, [&](auto f) { hipLaunchKernelGGL(k_remap<f.value>, grid, block, 0, s, out, out_pitch, S, (const entries2 *)table, tpitch, ow, oh, fill_bgr); })) {
    fprintf(stderr, "rdk::remap: unknown pixel format %d\n", fmt); abort();      // (the entry points refuse it first)
  }
}

}  // namespace rdk
