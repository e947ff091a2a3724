/* rectdetect-mi355x: remapped frames - the host's part of the contract in include/rectdetect_hip.h ("remapped frames"): the source position of an output pixel
 * under a lens and a view, and the table of 8.8 source coordinates a remapper uploads, from a lens or from a caller's float maps.  IEEE double, exactly the
 * operations the header writes, never contracted (-ffp-contract=off).  No HIP in here: tests/native/remap_host_check.c builds this file alone under the sanitizers. */
#include "rd_remap_host.h"
#include "rectdetect_hip.h"
#include <math.h>
#include <stddef.h>

/* the header's map, line by line */
static void source_position(const rd_lens *l, const rd_view *v, double u, double w, double *X, double *Y) {
  const double x = (u - v->cx) / v->fx, y = (w - v->cy) / v->fy;
  const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
  const double rad = ((l->k3 * r2 + l->k2) * r2 + l->k1) * r2 + 1.0;
  const double xd = (x * rad + (2.0 * l->p1) * xy) + l->p2 * (r2 + 2.0 * xx);
  const double yd = (y * rad + l->p1 * (r2 + 2.0 * yy)) + (2.0 * l->p2) * xy;
  *X = l->fx * xd + l->cx;
  *Y = l->fy * yd + l->cy;
}

/* one entry: 1 when it is inside.  The comparisons are made in double, so a NaN or an infinity is outside */
static int table_entry(double X, double Y, int iw, int ih, int32_t *e) {
  if (X >= 0.0 && X <= (double)(iw - 1) && Y >= 0.0 && Y <= (double)(ih - 1)) {
    e[0] = (int32_t)floor(X * 256.0);
    e[1] = (int32_t)floor(Y * 256.0);
    return 1;
  }
  e[0] = e[1] = -1;
  return 0;
}

int rd_remap_sizes_ok(int ow, int oh, int iw, int ih) {
  return ow >= 1 && oh >= 1 && ow <= RD_REMAP_MAX_OUT && oh <= RD_REMAP_MAX_OUT && iw >= 1 && ih >= 1 && iw <= RD_REMAP_MAX_SRC && ih <= RD_REMAP_MAX_SRC;
}

static int cameras_ok(const rd_lens *l, const rd_view *v) {
  if (!l || !v) return 0;
  const double f[13] = { l->fx, l->fy, l->cx, l->cy, l->k1, l->k2, l->p1, l->p2, l->k3, v->fx, v->fy, v->cx, v->cy };
  for (int k = 0; k < 13; k++) if (!isfinite(f[k])) return 0;
  return v->fx != 0.0 && v->fy != 0.0;
}

void rd_remap_points(const rd_lens *lens, const rd_view *view, const double *uv, int n, double *XY) {
  for (int k = 0; k < n; k++) source_position(lens, view, uv[2 * (size_t)k], uv[2 * (size_t)k + 1], &XY[2 * (size_t)k], &XY[2 * (size_t)k + 1]);
}

int rd_remap_table_lens(const rd_lens *lens, const rd_view *view, int ow, int oh, int iw, int ih, int32_t *table) {
  if (!table || !rd_remap_sizes_ok(ow, oh, iw, ih) || !cameras_ok(lens, view)) return -1;
  int inside = 0;
  for (int v = 0; v < oh; v++)
    for (int u = 0; u < ow; u++) {
      double X, Y;
      source_position(lens, view, (double)u, (double)v, &X, &Y);
      inside += table_entry(X, Y, iw, ih, table + 2 * ((size_t)v * ow + u));
    }
  return inside;
}

int rd_remap_table_map(const float *mapx, const float *mapy, int ow, int oh, int iw, int ih, int32_t *table) {
  if (!mapx || !mapy || !table || !rd_remap_sizes_ok(ow, oh, iw, ih)) return -1;
  int inside = 0;
  for (size_t k = 0; k < (size_t)ow * oh; k++) inside += table_entry((double)mapx[k], (double)mapy[k], iw, ih, table + 2 * k);
  return inside;
}

double rd_view_tan_aov(const rd_view *view, int ow) { return (double)(ow / 2) / view->fx; }

void rd_remap_limits(int32_t out[4]) {
  out[0] = 1; out[1] = RD_REMAP_MAX_OUT; out[2] = 1; out[3] = RD_REMAP_MAX_SRC;
}
