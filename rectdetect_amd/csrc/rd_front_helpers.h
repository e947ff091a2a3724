// rectdetect-mi355x: device helpers shared by the front-end kernels (rd_k_front.hip) and the fused gradient / suppression tile kernel
// (rd_k_nms.hip, a translation unit of its own because it is compiled without the SLP vectoriser: packed fp32 operations cost more than the two
// plain ones they replace in that kernel - profiles/NOTES_r04.md).
#pragma once
#include "rd_device.h"

namespace {
using namespace rd;

// iu:346-352 (5x5 kernel; double literals narrowed to float) and iu:395-420
__device__ __forceinline__ float v5c(int i) {
  const float t[25] = {
    (float)-4.667, (float)-4.083, (float)0.000, (float)4.083, (float)4.667,
    (float)-10.024, (float)-0.963, (float)0.000, (float)0.963, (float)10.024,
    (float)-14.120, (float)3.622, (float)0.000, (float)-3.622, (float)14.120,
    (float)-10.024, (float)-0.963, (float)0.000, (float)0.963, (float)10.024,
    (float)-4.667, (float)-4.083, (float)0.000, (float)4.083, (float)4.667,
  };
  return t[i];
}

__device__ __forceinline__ float ep_strength(const float (&n)[3], const float (&s)[3], const float (&w)[3], const float (&e)[3],
                                             const float (&nw)[3], const float (&ne)[3], const float (&sw)[3], const float (&se)[3]) {
  float sum[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float t = n[c] + w[c] - s[c] - e[c];
    float acc = 0;
    acc += (nw[c] - se[c]) * t;
    t = n[c] - w[c] + e[c] - s[c];
    acc += (ne[c] - sw[c]) * t;
    sum[c] = fmaxf(0.0f, acc);
  }
  const float tot = sum[0] + sum[1] + sum[2];
  return tot > 0 ? sqrtf(tot) : 0.0f;
}

#define TT_PITCH 72
__device__ __forceinline__ float bicubic_lds(const float *t, float x, float y, int x0, int y0) {
  const int ix = (int)x, iy = (int)y;
  const float fx = x - ix, fy = y - iy;
  const float *q = t + (iy - 1 - (y0 - 3)) * TT_PITCH + (ix - 1 - (x0 - 3));
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = cubic1(q[k * TT_PITCH], q[k * TT_PITCH + 1], q[k * TT_PITCH + 2], q[k * TT_PITCH + 3], fx);
  return cubic1(r[0], r[1], r[2], r[3], fy);
}

// cubic1's row polynomial with the position taken out: for the four cells p0..p3 that start at a column, {x, y, z, w} are the three bracketed terms of
// cubic1 and p1, so that cubic1(p0, p1, p2, p3, f) == ((x * f + y) * f + z) * f * 0.5f + w bit for bit (same operations in the same order)
__device__ __forceinline__ float4 cubic_coef(float p0, float p1, float p2, float p3) {
  const float v = p1 - p2, w = p3 - p0;
  return make_float4(v * 3.0f + w, -4.0f * v + (p0 - p1 - w), p2 - p0, p1);
}

// bicubic_lds on a tile of cubic_coef cells (pitch CF_PITCH, the cell of start column x0 - 3 and row y0 - 3 first): one 128-bit read per row
#define CF_PITCH 68
__device__ __forceinline__ float bicubic(const float4 *t, float x, float y, int x0, int y0) {
  const int ix = (int)x, iy = (int)y;
  const float fx = x - ix, fy = y - iy;
  const float4 *q = t + (iy - 1 - (y0 - 3)) * CF_PITCH + (ix - 1 - (x0 - 3));
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float4 c = q[k * CF_PITCH];
    float u = c.x;
    u = u * fx + c.y;
    u = u * fx + c.z;
    u = u * fx * 0.5f + c.w;
    r[k] = u;
  }
  return cubic1(r[0], r[1], r[2], r[3], fy);
}

}  // namespace
