/* TEST INFRASTRUCTURE.  The grade rectifier's host-only code (csrc/rd_grade_host.c: whether a spec is legal, the bytes of a quad's output, the cell of a pixel, the
 * limits, the variance of the Laplacian, a percentile of the histogram) under AddressSanitizer + UndefinedBehaviorSanitizer, as a plain process: built and run by
 * tests/test_cpu_grade.py.  Every pixel of several sizes at every cells, records at the extremes of the contract's bounds - where a signed overflow or a bad
 * conversion would be reported -, histograms with every word at its largest, results read from and written next to guard words.  A sanitizer report ends the
 * process with a non-zero exit code. */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "rectdetect_hip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) fprintf(stderr, "grade_host_check: line %d: %s\n", __LINE__, #c); failures++; } } while (0)

int main(void) {
  int32_t lim[10];
  for (int k = 0; k < 10; k++) lim[k] = -7;
  rd_grade_limits(lim + 1);
  CHECK(lim[0] == -7 && lim[9] == -7);
  CHECK(lim[1] == 15 && lim[2] == 7 && lim[3] == 1020 && lim[4] >= 64 && lim[4] % 64 == 0 && lim[5] >= 1 && lim[6] == 48 && lim[7] == 1024 && lim[8] == 0);
  CHECK(sizeof(rd_grade_spec) == 32 && sizeof(rd_grade_cell) == 48 && offsetof(rd_grade_cell, sg) == 16 && offsetof(rd_grade_cell, sll) == 40);

  /* legal and illegal specs, and the bytes */
  const rd_grade_spec ok = { 4, 8, 247, 64, 1, 0, { 0, 0 } };
  rd_grade_spec bad;
  CHECK(rd_grade_spec_ok(&ok, 128, 96) == 1 && rd_grade_bytes(&ok, 128, 96) == 768 && rd_grade_spec_ok(NULL, 8, 8) == 0 && rd_grade_bytes(NULL, 8, 8) == 0 && rd_grade_cell_of(NULL, 8, 8, 0, 0) == -1);
  bad = ok; bad.hist = 1; CHECK(rd_grade_bytes(&bad, 4, 4) == 768 + 1024 && rd_grade_bytes(&bad, 3, 4) == 0 && rd_grade_bytes(&bad, 4, 3) == 0);
  bad.cells = 1; CHECK(rd_grade_bytes(&bad, 1, 1) == 48 + 1024 && rd_grade_bytes(&bad, 16384, 16384) == 48 + 1024 && rd_grade_bytes(&bad, 16385, 1) == 0 && rd_grade_bytes(&bad, 1, 16385) == 0 && rd_grade_bytes(&bad, 0, 1) == 0 && rd_grade_bytes(&bad, 1, -1) == 0);
  bad.oversample = 4; CHECK(rd_grade_spec_ok(&bad, 4096, 4096) == 1 && rd_grade_spec_ok(&bad, 4097, 8) == 0 && rd_grade_spec_ok(&bad, 8, 4097) == 0);
  bad = ok; bad.cells = 8; CHECK(rd_grade_bytes(&bad, 8, 8) == 3072 && rd_grade_spec_ok(&bad, 7, 8) == 0 && rd_grade_spec_ok(&bad, 8, 7) == 0);
  static const int32_t wrong[8][4] = { { 0, 3, 16, -1 }, { -1, 256, -1, 256 }, { -1, 256, -1, 256 }, { -1, 1021, -1, 1021 }, { 0, 3, 8, -1 }, { -1, 2, -1, 2 }, { 1, -1, 1, -1 }, { 1, -1, 1, -1 } };
  for (int field = 0; field < 8; field++)
    for (int k = 0; k < 4; k++) {
      bad = ok;
      ((int32_t *)&bad)[field] = wrong[field][k];
      CHECK(rd_grade_spec_ok(&bad, 64, 64) == 0 && rd_grade_bytes(&bad, 64, 64) == 0 && rd_grade_cell_of(&bad, 64, 64, 1, 1) == -1);
    }
  static const int32_t right[6][4] = { { 1, 2, 4, 8 }, { 0, 1, 254, 255 }, { 0, 1, 254, 255 }, { 0, 1, 1019, 1020 }, { 1, 2, 4, 4 }, { 0, 1, 0, 1 } };
  for (int field = 0; field < 6; field++)
    for (int k = 0; k < 4; k++) {
      bad = ok;
      ((int32_t *)&bad)[field] = right[field][k];
      CHECK(rd_grade_spec_ok(&bad, 64, 64) == 1);
    }

  /* the cell of every pixel: in range, non-decreasing along rows and columns, every cell met, the counts add up */
  static const int sizes[][2] = { { 8, 8 }, { 9, 5 }, { 65, 17 }, { 131, 15 }, { 16384, 8 } }, cs[] = { 1, 2, 4, 8 };
  long pixels = 0;
  for (unsigned si = 0; si < sizeof(sizes) / sizeof(sizes[0]); si++)
    for (int ci = 0; ci < 4; ci++) {
      const int pw = sizes[si][0], ph = sizes[si][1], c = cs[ci];
      rd_grade_spec s = ok;
      s.cells = c;
      if (ph < c) { CHECK(rd_grade_cell_of(&s, pw, ph, 0, 0) == -1); continue; }
      long count[64];
      memset(count, 0, sizeof(count));
      for (int j = 0; j < ph; j++)
        for (int i = 0; i < pw; i++) {
          const int r = rd_grade_cell_of(&s, pw, ph, i, j);
          CHECK(r >= 0 && r < c * c && r == (int)(((int64_t)j * c) / ph) * c + (int)(((int64_t)i * c) / pw));
          if (r >= 0 && r < 64) count[r]++;
          pixels++;
        }
      long total = 0;
      for (int r = 0; r < c * c; r++) { CHECK(count[r] > 0); total += count[r]; }
      CHECK(total == (long)pw * ph);
      CHECK(rd_grade_cell_of(&s, pw, ph, -1, 0) == -1 && rd_grade_cell_of(&s, pw, ph, pw, 0) == -1 && rd_grade_cell_of(&s, pw, ph, 0, -1) == -1 && rd_grade_cell_of(&s, pw, ph, 0, ph) == -1);
    }
  CHECK(pixels > 100000);

  /* sharpness: the empty record, small ones in closed form, the records at the contract's bounds */
  rd_grade_cell guard[3];
  memset(guard, 0xA5, sizeof(guard));
  rd_grade_cell *c = &guard[1];
  memset(c, 0, sizeof(*c));
  CHECK(rd_grade_sharpness(NULL) == 0.0 && rd_grade_sharpness(c) == 0.0);
  c->n = 4; c->sl = 2; c->sll = 10; CHECK(rd_grade_sharpness(c) == 2.25);
  c->n = 1; c->sl = -1020; c->sll = 1040400; CHECK(rd_grade_sharpness(c) == 0.0);
  c->n = 1 << 28; c->sl = 0; c->sll = (int64_t)(1 << 28) * 1040400; CHECK(rd_grade_sharpness(c) == 1040400.0);
  c->n = 1 << 28; c->sl = -(int64_t)(1 << 28) * 1020; c->sll = (int64_t)(1 << 28) * 1040400; CHECK(rd_grade_sharpness(c) == 0.0);
  c->n = 2147483647; c->sl = INT64_MAX; c->sll = INT64_MAX; CHECK(rd_grade_sharpness(c) < 0.0);      /* (no legal record; no undefined behaviour either) */
  c->n = -1; c->sl = INT64_MIN; c->sll = INT64_MIN; (void)rd_grade_sharpness(c);
  CHECK(((const uint8_t *)&guard[0])[47] == 0xA5 && ((const uint8_t *)&guard[2])[0] == 0xA5);
  CHECK((int64_t)(1 << 28) * 1040400 == 279280248422400LL && 66564LL * 65025 == 4328324100LL && 4328324100LL > 4294967296LL);

  /* percentiles: a histogram between guard words, every word at its largest, bad arguments */
  uint32_t buf[258];
  buf[0] = buf[257] = 0xA5A5A5A5u;
  uint32_t *h = buf + 1;
  memset(h, 0, 1024);
  CHECK(rd_grade_percentile(h, 1, 2) == -1 && rd_grade_percentile(NULL, 1, 2) == -1);
  h[10] = 5; h[200] = 5;
  CHECK(rd_grade_percentile(h, 0, 100) == 0 && rd_grade_percentile(h, 1, 100) == 10 && rd_grade_percentile(h, 50, 100) == 10 && rd_grade_percentile(h, 51, 100) == 200 && rd_grade_percentile(h, 100, 100) == 200);
  CHECK(rd_grade_percentile(h, -1, 100) == -1 && rd_grade_percentile(h, 101, 100) == -1 && rd_grade_percentile(h, 0, 0) == -1 && rd_grade_percentile(h, 1, -1) == -1 && rd_grade_percentile(h, 1, (1 << 20) + 1) == -1);
  for (int v = 0; v < 256; v++) h[v] = 0xFFFFFFFFu;
  CHECK(rd_grade_percentile(h, 1 << 20, 1 << 20) == 255 && rd_grade_percentile(h, 1 << 19, 1 << 20) == 127 && rd_grade_percentile(h, 1, 1 << 20) == 0 && rd_grade_percentile(h, (1 << 19) + 1, 1 << 20) == 128);
  CHECK(buf[0] == 0xA5A5A5A5u && buf[257] == 0xA5A5A5A5u);

  if (failures) { fprintf(stderr, "grade_host_check: %d check(s) failed\n", failures); return 1; }
  printf("grade_host_check: ok (%ld pixels)\n", pixels);
  return 0;
}
