/* TEST INFRASTRUCTURE.  The remapper's host-only code (csrc/rd_remap_host.c: the lens map, the table from a lens and from float maps) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, as a plain process: built and run by tests/test_cpu_remap.py.  Extreme inputs - coefficients and focal lengths at +-1e300, positions
 * that overflow to infinity or come out NaN (none of which may reach the conversion to an integer), maps of NaN, infinities and the floats next to the frame's
 * edges, a 1 x 1 table, tables allocated to the byte, every argument error - and a few exact expectations.  A sanitizer report ends the process with a non-zero
 * exit code. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rd_remap_host.h"
#include "rectdetect_hip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "remap_host_check: line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static int entries_ok(const int32_t *t, size_t n, int iw, int ih, int inside) {
  int in = 0;
  for (size_t k = 0; k < n; k++) {
    const int32_t xi = t[2 * k], yi = t[2 * k + 1];
    if (xi == -1 && yi == -1) continue;
    if (xi < 0 || yi < 0 || xi > (iw - 1) * 256 || yi > (ih - 1) * 256) return 0;
    in++;
  }
  return in == inside;
}

int main(void) {
  int32_t lim[4];
  rd_remap_limits(lim);
  CHECK(lim[0] == 1 && lim[1] == RD_REMAP_MAX_OUT && lim[2] == 1 && lim[3] == RD_REMAP_MAX_SRC && lim[1] == 16384 && lim[3] == 65536);
  CHECK(sizeof(rd_lens) == 72 && sizeof(rd_view) == 32);

  /* the identity: every operation exact */
  {
    const int iw = 37, ih = 23;
    const rd_lens l = { 64.0, 64.0, 18.0, 11.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    const rd_view v = { 64.0, 64.0, 18.0, 11.0 };
    int32_t *t = (int32_t *)malloc((size_t)iw * ih * 2 * sizeof(int32_t));      /* (to the byte: a write behind it is a report) */
    CHECK(rd_remap_table_lens(&l, &v, iw, ih, iw, ih, t) == iw * ih);
    for (int y = 0; y < ih; y++) for (int x = 0; x < iw; x++) CHECK(t[2 * (y * iw + x)] == 256 * x && t[2 * (y * iw + x) + 1] == 256 * y);
    free(t);
    const double uv[4] = { 3.25, 7.5, -2.0, 100.0 };
    double XY[4];
    rd_remap_points(&l, &v, uv, 2, XY);
    CHECK(XY[0] == 3.25 && XY[1] == 7.5 && XY[2] == -2.0 && XY[3] == 100.0);
    rd_remap_points(&l, &v, uv, 0, NULL);
    CHECK(rd_view_tan_aov(&v, 128) == 1.0 && rd_view_tan_aov(&v, 129) == 1.0 && rd_view_tan_aov(&v, 1) == 0.0);
  }

  /* a 1 x 1 table, from the smallest and from the largest source */
  {
    const rd_lens l = { 1.0, 1.0, 0.0, 0.0, -0.1, 0.0, 0.0, 0.0, 0.0 };
    const rd_view v = { 1.0, 1.0, 0.0, 0.0 };
    int32_t *t = (int32_t *)malloc(2 * sizeof(int32_t));
    CHECK(rd_remap_table_lens(&l, &v, 1, 1, 1, 1, t) == 1 && t[0] == 0 && t[1] == 0);
    CHECK(rd_remap_table_lens(&l, &v, 1, 1, 65536, 65536, t) == 1 && t[0] == 0 && t[1] == 0);
    const rd_lens far = { 1.0, 1.0, 65535.0, 65535.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    CHECK(rd_remap_table_lens(&far, &v, 1, 1, 65536, 65536, t) == 1 && t[0] == 65535 * 256 && t[1] == 65535 * 256);
    const float one = 0.5f;
    CHECK(rd_remap_table_map(&one, &one, 1, 1, 2, 2, t) == 1 && t[0] == 128 && t[1] == 128);
    CHECK(rd_remap_table_map(&one, &one, 1, 1, 1, 1, t) == 0 && t[0] == -1 && t[1] == -1);
    free(t);
  }

  /* extreme lenses and views: every call returns, every entry is (-1, -1) or within the source */
  {
    const double big[] = { 1.0, -1.0, 1e-300, -1e-300, 1e300, -1e300, DBL_MAX, -DBL_MAX, 5e-324, 0.0, -0.0, 0.25, 1000.0 };
    const int nbig = (int)(sizeof(big) / sizeof(big[0]));
    const int sizes[][4] = { { 1, 1, 1, 1 }, { 7, 5, 9, 6 }, { 3, 2, 65536, 1 }, { 2, 3, 1, 65536 } };
    for (int a = 0; a < nbig; a++)
      for (int b = 0; b < nbig; b++)
        for (int s = 0; s < 4; s++) {
          const int ow = sizes[s][0], oh = sizes[s][1], iw = sizes[s][2], ih = sizes[s][3];
          const rd_lens l = { big[a], big[b], big[b], big[a], big[a], big[b], big[b], big[a], big[a] };
          const rd_view v = { big[b], big[a], big[a], big[b] };
          int32_t *t = (int32_t *)malloc((size_t)ow * oh * 2 * sizeof(int32_t));
          const int n = rd_remap_table_lens(&l, &v, ow, oh, iw, ih, t);
          if (big[a] == 0.0 || big[b] == 0.0) CHECK(n == -1);      /* (a view with fx or fy of 0, either sign) */
          else CHECK(n >= 0 && n <= ow * oh && entries_ok(t, (size_t)ow * oh, iw, ih, n));
          free(t);
        }
  }

  /* maps: the floats at and next to the edges, and everything that is no position */
  {
    const int iw = 6, ih = 4;
    const float xs[] = { 5.0f, nextafterf(5.0f, INFINITY), -0.0f, -FLT_TRUE_MIN, NAN, INFINITY, -INFINITY, FLT_MAX, -FLT_MAX, 4.99999952f, 0.0f };
    const int n = (int)(sizeof(xs) / sizeof(xs[0]));
    float *mx = (float *)malloc((size_t)n * n * sizeof(float)), *my = (float *)malloc((size_t)n * n * sizeof(float));
    int32_t *t = (int32_t *)malloc((size_t)n * n * 2 * sizeof(int32_t));
    for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) { mx[j * n + i] = xs[i]; my[j * n + i] = xs[j] == 5.0f ? 3.0f : xs[j]; }
    const int in = rd_remap_table_map(mx, my, n, n, iw, ih, t);
    CHECK(in == 4 * 3 && entries_ok(t, (size_t)n * n, iw, ih, in));      /* inside in x: 5, -0, 4.9999995, 0; in y: 3 (for 5), -0, 0 */
    CHECK(t[0] == 5 * 256 && t[1] == 3 * 256 && t[2] == -1 && t[3] == -1 && t[4] == 0 && t[6] == -1 && t[2 * 9] == 5 * 256 - 1);
    free(mx); free(my); free(t);
  }

  /* argument errors: -1, and the table is not touched (it is not even there) */
  {
    const rd_lens l = { 4.0, 4.0, 3.0, 1.5, -0.1, 0.0, 0.0, 0.0, 0.0 };
    const rd_view v = { 4.0, 4.0, 2.0, 1.0 };
    const float m[1] = { 0.0f };
    int32_t t[2] = { 77, 77 };
    CHECK(rd_remap_table_lens(NULL, &v, 1, 1, 1, 1, t) == -1 && rd_remap_table_lens(&l, NULL, 1, 1, 1, 1, t) == -1 && rd_remap_table_lens(&l, &v, 1, 1, 1, 1, NULL) == -1);
    CHECK(rd_remap_table_map(NULL, m, 1, 1, 1, 1, t) == -1 && rd_remap_table_map(m, NULL, 1, 1, 1, 1, t) == -1 && rd_remap_table_map(m, m, 1, 1, 1, 1, NULL) == -1);
    const int bad[][4] = { { 0, 1, 1, 1 }, { 1, 0, 1, 1 }, { 1, 1, 0, 1 }, { 1, 1, 1, 0 }, { -1, 1, 1, 1 }, { 16385, 1, 1, 1 }, { 1, 16385, 1, 1 }, { 1, 1, 65537, 1 }, { 1, 1, 1, 65537 },
                           { INT32_MAX, INT32_MAX, 1, 1 }, { 1, 1, INT32_MIN, 1 } };
    for (int k = 0; k < (int)(sizeof(bad) / sizeof(bad[0])); k++) {
      CHECK(rd_remap_table_lens(&l, &v, bad[k][0], bad[k][1], bad[k][2], bad[k][3], t) == -1);
      CHECK(rd_remap_table_map(m, m, bad[k][0], bad[k][1], bad[k][2], bad[k][3], t) == -1);
      CHECK(!rd_remap_sizes_ok(bad[k][0], bad[k][1], bad[k][2], bad[k][3]));
    }
    const double nf[3] = { NAN, INFINITY, -INFINITY };
    for (int f = 0; f < 9; f++) for (int k = 0; k < 3; k++) { rd_lens x = l; ((double *)&x)[f] = nf[k]; CHECK(rd_remap_table_lens(&x, &v, 1, 1, 1, 1, t) == -1); }
    for (int f = 0; f < 4; f++) for (int k = 0; k < 3; k++) { rd_view x = v; ((double *)&x)[f] = nf[k]; CHECK(rd_remap_table_lens(&l, &x, 1, 1, 1, 1, t) == -1); }
    CHECK(t[0] == 77 && t[1] == 77);
    CHECK(rd_remap_sizes_ok(16384, 16384, 65536, 65536) && rd_remap_sizes_ok(1, 1, 1, 1));
  }

  if (failures) { fprintf(stderr, "remap_host_check: %d check(s) failed\n", failures); return 1; }
  printf("remap_host_check: ok\n");
  return 0;
}
