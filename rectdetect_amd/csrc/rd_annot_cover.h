// rectdetect-mi355x: the coverage test of annotated frames (the contract: include/rectdetect_hip.h, "annotated frames") - ONE statement of it for the draw
// kernel (rd_k_annotate.hip), the host object (rd_annotate.hip: the records a job uploads) and the host test tap rd_annot_covers.  Integers only.
//
// A primitive becomes a line record: e is linear in the pixel's coordinates,
//   e(x, y) = c + ex * x + ey * y  =  2 (u - ua)(vb - va) + D - 2 D (v - va)          (u the major coordinate, v the minor one)
// and a pixel is covered when  ua <= u <= ub  and  elo <= e < ehi  with  elo = -2 D hi,  ehi = 2 D (lo + 1).
// D = 0 (a point: the contract's test is -lo <= v - va <= hi) is the same test with D = 1 and vb = va:  -2 hi <= 1 - 2 (v - va) < 2 (lo + 1)  <=>
// -lo <= v - va <= hi  for integers.  Magnitudes at the legal coordinates (|x|, |y| <= 2^20, so D and |vb - va| < 2^21; pixels < 2^16; thickness <= 255):
// |ex|, |ey| < 2^22, |c| < 2^44, |e| < 2^45, |elo|, |ehi| < 2^30 - all of it int64 with room to spare.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RD_ANNOT_HD __host__ __device__ __forceinline__
#else
#define RD_ANNOT_HD static inline
#endif

typedef struct {
  int64_t c, elo, ehi;
  int32_t ex, ey;      // e's steps to the next pixel right / down
  int32_t ua, ub;      // the major coordinate's span
  int32_t ymajor;      // 0: u = x, 1: u = y
  int32_t pad;
} rd_annot_line;

RD_ANNOT_HD void rd_annot_line_setup(rd_annot_line *L, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t t) {
  const int64_t dx = (int64_t)x1 - x0, dy = (int64_t)y1 - y0;
  const int ymajor = (dx < 0 ? -dx : dx) < (dy < 0 ? -dy : dy);
  int64_t ua = ymajor ? y0 : x0, va = ymajor ? x0 : y0, ub = ymajor ? y1 : x1, vb = ymajor ? x1 : y1;
  if (ua > ub) { int64_t s = ua; ua = ub; ub = s; s = va; va = vb; vb = s; }
  int64_t D = ub - ua, dv = vb - va;
  if (D == 0) { D = 1; dv = 0; }      // (the point, see above)
  const int64_t lo = (t - 1) / 2, hi = t / 2;
  const int64_t eu = 2 * dv, ev = -2 * D;      // e's steps along u and v
  L->c = D - eu * ua - ev * va;
  L->elo = -2 * D * hi;
  L->ehi = 2 * D * (lo + 1);
  L->ex = (int32_t)(ymajor ? ev : eu);
  L->ey = (int32_t)(ymajor ? eu : ev);
  L->ua = (int32_t)ua; L->ub = (int32_t)ub;
  L->ymajor = ymajor; L->pad = 0;
}

RD_ANNOT_HD int64_t rd_annot_line_e(const rd_annot_line *L, int32_t x, int32_t y) { return L->c + (int64_t)L->ex * x + (int64_t)L->ey * y; }

// pixel (x, y) whose e is known (the kernel steps e by ex / ey from one pixel of a thread to the next)
RD_ANNOT_HD int rd_annot_line_covers_e(const rd_annot_line *L, int32_t x, int32_t y, int64_t e) {
  const int32_t u = L->ymajor ? y : x;
  return u >= L->ua && u <= L->ub && e >= L->elo && e < L->ehi;
}

RD_ANNOT_HD int rd_annot_line_covers(const rd_annot_line *L, int32_t x, int32_t y) { return rd_annot_line_covers_e(L, x, y, rd_annot_line_e(L, x, y)); }

// May the line cover a pixel of the rectangle [x0, x1] x [y0, y1] (inclusive)?  The rectangle is cut to the span along u first; e is linear, so over what is left
// it lies between its values at the corners: the band elo <= e < ehi can hold a pixel only if it reaches into [min, max].  May say yes for a rectangle the line only
// passes close to (no lattice point in the band); never says no for a rectangle with a covered pixel.
RD_ANNOT_HD int rd_annot_line_touches(const rd_annot_line *L, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
  if (L->ymajor) { y0 = y0 > L->ua ? y0 : L->ua; y1 = y1 < L->ub ? y1 : L->ub; }
  else { x0 = x0 > L->ua ? x0 : L->ua; x1 = x1 < L->ub ? x1 : L->ub; }
  if (x0 > x1 || y0 > y1) return 0;
  const int64_t ax = (int64_t)L->ex * x0, bx = (int64_t)L->ex * x1, ay = (int64_t)L->ey * y0, by = (int64_t)L->ey * y1;
  const int64_t emin = L->c + (ax < bx ? ax : bx) + (ay < by ? ay : by), emax = L->c + (ax < bx ? bx : ax) + (ay < by ? by : ay);
  return emax >= L->elo && emin < L->ehi;
}
