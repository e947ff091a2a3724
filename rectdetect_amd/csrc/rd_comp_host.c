/* rectdetect-mi355x: composited quads - the host's part of the contract in include/rectdetect_hip.h ("composited quads"): coefficients, adjugate, pixel box, the
 * per-pixel coverage test (test tap) and the list of tiles an in-place job launches.  IEEE double, exactly the operations the header writes, never contracted
 * (-ffp-contract=off).  No HIP in here: tests/native/comp_host_check.c builds this file alone under the sanitizers. */
#include "rd_comp_host.h"
#include "rectdetect_hip.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* rd_rectify_coefficients (rd_rectify.hip), copied so that this file stands without HIP; tests/test_cpu_composite.py holds the two together */
static int forward_coefficients(const double quad[8], double coef[8]) {
  double x[4], y[4];
  for (int k = 0; k < 4; k++) { x[k] = quad[2 * k]; y[k] = quad[2 * k + 1]; if (!isfinite(x[k]) || !isfinite(y[k])) return 0; }
  int pos = 0, neg = 0;
  for (int i = 0; i < 4; i++) {
    const int j = (i + 1) & 3, k = (i + 2) & 3;
    const double cr = (x[j] - x[i]) * (y[k] - y[j]) - (y[j] - y[i]) * (x[k] - x[j]);
    pos += cr > 0.0; neg += cr < 0.0;
  }
  if (pos != 4 && neg != 4) return 0;
  const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], sx = ((x[0] - x[1]) + x[2]) - x[3];
  const double dy1 = y[1] - y[2], dy2 = y[3] - y[2], sy = ((y[0] - y[1]) + y[2]) - y[3];
  const double den = dx1 * dy2 - dx2 * dy1;
  const double g = (sx * dy2 - dx2 * sy) / den, h = (dx1 * sy - sx * dy1) / den;
  const double c[8] = { (x[1] - x[0]) + g * x[1], (x[3] - x[0]) + h * x[3], x[0], (y[1] - y[0]) + g * y[1], (y[3] - y[0]) + h * y[3], y[0], g, h };
  for (int k = 0; k < 8; k++) if (!isfinite(c[k])) return 0;
  for (int k = 0; k < 8; k++) coef[k] = c[k];
  return 1;
}

/* one axis of the pixel box: 0 when it is empty */
static int box_axis(const double v[4], int size, int32_t *lo, int32_t *hi) {
  double mn = v[0], mx = v[0];
  for (int k = 1; k < 4; k++) { mn = v[k] < mn ? v[k] : mn; mx = v[k] > mx ? v[k] : mx; }
  const double fl = floor(mn) - 1.0, ce = ceil(mx) + 1.0, last = (double)(size - 1);
  if (ce < 0.0 || fl > last) return 0;
  *lo = (int32_t)(fl > 0.0 ? fl : 0.0);
  *hi = (int32_t)(ce < last ? ce : last);
  return 1;
}

void rd_comp_make_rec(const double quad[8], int iw, int ih, rd_comp_rec *r) {
  for (int k = 0; k < 9; k++) r->inv[k] = 0.0;
  r->box[0] = r->box[1] = 0; r->box[2] = r->box[3] = -1;
  r->status = 0;
  double co[8];
  if (!forward_coefficients(quad, co)) return;
  const double a = co[0], b = co[1], c = co[2], d = co[3], e = co[4], f = co[5], g = co[6], h = co[7];
  const double inv[9] = { e - f * h, c * h - b, b * f - c * e,  f * g - d, a - c * g, c * d - a * f,  d * h - e * g, b * g - a * h, a * e - b * d };
  for (int k = 0; k < 9; k++) if (!isfinite(inv[k])) return;
  for (int k = 0; k < 9; k++) r->inv[k] = inv[k];
  r->status = 1;
  const double xs[4] = { quad[0], quad[2], quad[4], quad[6] }, ys[4] = { quad[1], quad[3], quad[5], quad[7] };
  int32_t x0, x1, y0, y1;
  if (iw < 1 || ih < 1 || !box_axis(xs, iw, &x0, &x1) || !box_axis(ys, ih, &y0, &y1)) return;      /* valid, covers nothing */
  r->box[0] = x0; r->box[1] = y0; r->box[2] = x1; r->box[3] = y1;
}

int rd_comp_rec_covers(const rd_comp_rec *r, int x, int y, double st[2]) {
  if (st) st[0] = st[1] = 0.0;
  if (!r->status || x < r->box[0] || x > r->box[2] || y < r->box[1] || y > r->box[3]) return 0;
  const double X = (double)x, Y = (double)y;
  const double wn = (r->inv[6] * X + r->inv[7] * Y) + r->inv[8];
  const double s = ((r->inv[0] * X + r->inv[1] * Y) + r->inv[2]) / wn;
  const double t = ((r->inv[3] * X + r->inv[4] * Y) + r->inv[5]) / wn;
  if (st) { st[0] = s; st[1] = t; }
  return s >= 0.0 && s < 1.0 && t >= 0.0 && t < 1.0;
}

/* the tiles a record's box reaches, marked; `span` (tx0, ty0, tx1, ty1, starting at gx, gy, -1, -1) grows to hold them */
static void mark_box(const rd_comp_rec *r, int gx, uint8_t *mark, int span[4]) {
  if (!r->status || r->box[0] > r->box[2] || r->box[1] > r->box[3]) return;
  const int tx0 = r->box[0] / RD_COMP_TILE_W, tx1 = r->box[2] / RD_COMP_TILE_W, ty0 = r->box[1] / RD_COMP_TILE_H, ty1 = r->box[3] / RD_COMP_TILE_H;
  for (int ty = ty0; ty <= ty1; ty++) memset(mark + (size_t)ty * gx + tx0, 1, (size_t)(tx1 - tx0 + 1));
  if (tx0 < span[0]) span[0] = tx0;
  if (ty0 < span[1]) span[1] = ty0;
  if (tx1 > span[2]) span[2] = tx1;
  if (ty1 > span[3]) span[3] = ty1;
}

/* the marked tiles in raster order - all of them lie inside `span` - and the marks are taken off again */
static int take_marks(int gx, const int span[4], uint8_t *mark, int32_t *tiles_xy, int max) {
  int m = 0;
  for (int ty = span[1]; ty <= span[3]; ty++) {
    uint8_t *row = mark + (size_t)ty * gx;
    for (int tx = span[0]; tx <= span[2]; tx++) {
      if (!row[tx]) continue;
      row[tx] = 0;
      if (m < max && tiles_xy) { tiles_xy[2 * (size_t)m] = tx; tiles_xy[2 * (size_t)m + 1] = ty; }
      m++;
    }
  }
  return m;
}

int rd_comp_tiles_of(const rd_comp_rec *recs, int n, int iw, int ih, uint8_t *mark, int32_t *tiles_xy, int max) {
  const int gx = (iw + RD_COMP_TILE_W - 1) / RD_COMP_TILE_W, gy = (ih + RD_COMP_TILE_H - 1) / RD_COMP_TILE_H;
  int span[4] = { gx, gy, -1, -1 };
  for (int k = 0; k < n; k++) mark_box(&recs[k], gx, mark, span);
  return take_marks(gx, span, mark, tiles_xy, max);
}

void rd_composite_coefficients(const double quad[8], int iw, int ih, double inv[9], int32_t box[4], int *status) {
  rd_comp_rec r;
  rd_comp_make_rec(quad, iw, ih, &r);
  if (inv) memcpy(inv, r.inv, sizeof(r.inv));
  if (box) memcpy(box, r.box, sizeof(r.box));
  if (status) *status = r.status;
}

int rd_composite_covers(const double quad[8], int iw, int ih, int x, int y, double st[2]) {
  rd_comp_rec r;
  rd_comp_make_rec(quad, iw, ih, &r);
  return rd_comp_rec_covers(&r, x, y, st);
}

int rd_composite_tiles(const rd_comp_item *items, int n, int iw, int ih, int32_t *tiles_xy, int max) {
  if (iw < 1 || ih < 1 || iw > 65536 || ih > 65536 || n < 0 || (n > 0 && !items)) return -1;
  const int gx = (iw + RD_COMP_TILE_W - 1) / RD_COMP_TILE_W, gy = (ih + RD_COMP_TILE_H - 1) / RD_COMP_TILE_H;
  uint8_t *mark = (uint8_t *)calloc((size_t)gx * gy, 1);
  if (!mark) return -1;
  int span[4] = { gx, gy, -1, -1 };
  for (int k = 0; k < n; k++) {
    rd_comp_rec r;
    rd_comp_make_rec(items[k].quad, iw, ih, &r);
    mark_box(&r, gx, mark, span);
  }
  const int m = take_marks(gx, span, mark, tiles_xy, max);
  free(mark);
  return m;
}

void rd_comp_limits(int32_t out[4]) {
  out[0] = RD_COMP_TILE_W; out[1] = RD_COMP_TILE_H; out[2] = RD_COMP_CHUNK; out[3] = 0;
}
