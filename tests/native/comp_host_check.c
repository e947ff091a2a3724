/* TEST INFRASTRUCTURE.  The compositor's host-only code (csrc/rd_comp_host.c: coefficients, adjugate, pixel box, tile list) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, as a plain process: built and run by tests/test_cpu_composite.py.  Extreme inputs - corners at +-1e6 and +-1e300, NaN, infinities,
 * degenerate and concave quads, boxes wholly outside, frames of one pixel and of 65536 pixels a side, tile lists shorter than the result - and a few exact expectations.
 * A sanitizer report ends the process with a non-zero exit code. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rd_comp_host.h"
#include "rectdetect_hip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "comp_host_check: line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static void quad_of(double q[8], double x0, double y0, double x1, double y1, double x2, double y2, double x3, double y3) {
  q[0] = x0; q[1] = y0; q[2] = x1; q[3] = y1; q[4] = x2; q[5] = y2; q[6] = x3; q[7] = y3;
}

int main(void) {
  int32_t lim[4];
  rd_comp_limits(lim);
  CHECK(lim[0] == RD_COMP_TILE_W && lim[1] == RD_COMP_TILE_H && lim[2] == RD_COMP_CHUNK && lim[3] == 0);
  const int TW = lim[0], TH = lim[1];
  double q[8], inv[9], st[2];
  int32_t box[4];
  int status;

  /* the axis-aligned 64 x 64 quad at integer alignment: exactly its pixels */
  quad_of(q, 9.5, 9.5, 73.5, 9.5, 73.5, 73.5, 9.5, 73.5);
  rd_composite_coefficients(q, 320, 200, inv, box, &status);
  CHECK(status == 1 && box[0] == 8 && box[1] == 8 && box[2] == 75 && box[3] == 75);
  int covered = 0;
  for (int y = 0; y < 200; y++)
    for (int x = 0; x < 320; x++) {
      const int c = rd_composite_covers(q, 320, 200, x, y, st);
      covered += c;
      CHECK(c == (x >= 10 && x <= 73 && y >= 10 && y <= 73));
      if (c) CHECK(st[0] * 64.0 - 0.5 == (double)(x - 10) && st[1] * 64.0 - 0.5 == (double)(y - 10));
    }
  CHECK(covered == 64 * 64);

  /* extreme, degenerate and non-finite corners: every call must return, an invalid item has zeros and the empty box */
  const double big[] = { 1e6, -1e6, 1e300, -1e300, 1.7976931348623157e308, -1.7976931348623157e308, 5e-324, 0.0, -0.0, NAN, INFINITY, -INFINITY };
  const int nbig = (int)(sizeof(big) / sizeof(big[0]));
  const int sizes[][2] = { { 1, 1 }, { 320, 200 }, { 65536, 2 }, { 2, 65536 } };
  for (int a = 0; a < nbig; a++)
    for (int b = 0; b < nbig; b++)
      for (int s = 0; s < 4; s++) {
        const int iw = sizes[s][0], ih = sizes[s][1];
        /* a parallelogram between two extreme points, the same scaled by one value, and a quad with one extreme corner */
        quad_of(q, big[a], big[a], big[b], big[a], big[b], big[b], big[a], big[b]);
        for (int form = 0; form < 3; form++) {
          if (form == 1) quad_of(q, 0.0, 0.0, big[a], 0.0, big[a], big[b], 0.0, big[b]);
          if (form == 2) quad_of(q, 10.0, 10.0, 100.0, 12.0, big[a], big[b], 8.0, 90.0);
          rd_composite_coefficients(q, iw, ih, inv, box, &status);
          CHECK(status == 0 || status == 1);
          for (int k = 0; k < 9; k++) CHECK(isfinite(inv[k]) && (status || inv[k] == 0.0));
          const int empty = box[0] == 0 && box[1] == 0 && box[2] == -1 && box[3] == -1;
          CHECK(empty || (0 <= box[0] && box[0] <= box[2] && box[2] < iw && 0 <= box[1] && box[1] <= box[3] && box[3] < ih));
          if (!status) CHECK(empty);
          (void)rd_composite_covers(q, iw, ih, 0, 0, st);
          (void)rd_composite_covers(q, iw, ih, iw - 1, ih - 1, NULL);
          rd_comp_item it;
          memset(&it, 0, sizeof(it));
          memcpy(it.quad, q, sizeof(q));
          it.patch = -1;
          int32_t few[2 * 3];
          const int m = rd_composite_tiles(&it, 1, iw, ih, few, 3);      /* (a list shorter than the result: only three pairs may be written) */
          const int gx = (iw + TW - 1) / TW, gy = (ih + TH - 1) / TH;
          CHECK(m >= 0 && (long long)m <= (long long)gx * gy && (m > 0) == (status && !empty));
          for (int k = 0; k < m && k < 3; k++) CHECK(few[2 * k] >= 0 && few[2 * k] < gx && few[2 * k + 1] >= 0 && few[2 * k + 1] < gy);
        }
      }

  /* wholly outside on each side: valid, the empty box, no tile */
  const double off[][2] = { { -500.0, 50.0 }, { 900.0, 50.0 }, { 50.0, -500.0 }, { 50.0, 900.0 }, { 1e6, 1e6 }, { -1e6, -1e6 } };
  for (int k = 0; k < 6; k++) {
    quad_of(q, off[k][0], off[k][1], off[k][0] + 40.0, off[k][1] + 3.0, off[k][0] + 44.0, off[k][1] + 50.0, off[k][0] - 2.0, off[k][1] + 41.0);
    rd_composite_coefficients(q, 320, 200, inv, box, &status);
    CHECK(status == 1 && box[2] == -1 && box[3] == -1);
    rd_comp_item it;
    memset(&it, 0, sizeof(it));
    memcpy(it.quad, q, sizeof(q));
    CHECK(rd_composite_tiles(&it, 1, 320, 200, NULL, 0) == 0);
  }

  /* many items, the whole frame and a thin diagonal among them: the list is sorted, without repetition, and as long as a second call says */
  enum { N = 200 };
  rd_comp_item *items = (rd_comp_item *)calloc(N, sizeof(rd_comp_item));
  for (int k = 0; k < N; k++) {
    const double x = (double)((k * 37) % 300), y = (double)((k * 53) % 190);
    quad_of(items[k].quad, x, y, x + 20.0 + k % 7, y + 1.0, x + 22.0, y + 15.0 + k % 5, x - 1.0, y + 13.0);
  }
  quad_of(items[0].quad, -1.0, -1.0, 320.0, -1.0, 320.0, 200.0, -1.0, 200.0);
  quad_of(items[1].quad, 0.0, 0.0, 2.0, 0.0, 319.0, 198.0, 317.0, 198.0);
  const int m = rd_composite_tiles(items, N, 320, 200, NULL, 0);
  CHECK(m == (320 / TW) * ((200 + TH - 1) / TH));
  int32_t *list = (int32_t *)malloc((size_t)m * 2 * sizeof(int32_t));
  CHECK(rd_composite_tiles(items, N, 320, 200, list, m) == m);
  for (int k = 1; k < m; k++) CHECK(list[2 * k + 1] > list[2 * k - 1] || (list[2 * k + 1] == list[2 * k - 1] && list[2 * k] > list[2 * k - 2]));
  CHECK(rd_composite_tiles(items, -1, 320, 200, NULL, 0) == -1 && rd_composite_tiles(NULL, 1, 320, 200, NULL, 0) == -1 && rd_composite_tiles(items, 1, 0, 200, NULL, 0) == -1);
  CHECK(rd_composite_tiles(NULL, 0, 320, 200, NULL, 0) == 0);
  free(list);
  /* the largest frame there is, covered as a whole: every one of its tiles */
  quad_of(items[0].quad, -1e300, -1e300, 1e300, -1e300, 1e300, 1e300, -1e300, 1e300);
  rd_composite_coefficients(items[0].quad, 65536, 65536, inv, box, &status);
  CHECK(status == 0 || (box[0] == 0 && box[1] == 0 && box[2] == 65535 && box[3] == 65535));
  quad_of(items[0].quad, -1e6, -1e6, 1e6, -1e6, 1e6, 1e6, -1e6, 1e6);
  CHECK(rd_composite_tiles(items, 1, 65536, 65536, NULL, 0) == (65536 / TW) * (65536 / TH));
  free(items);

  if (failures) { fprintf(stderr, "comp_host_check: %d check(s) failed\n", failures); return 1; }
  printf("comp_host_check: ok\n");
  return 0;
}
