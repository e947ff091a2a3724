/* TEST INFRASTRUCTURE.  The code rectifier's host-only code (csrc/rd_code_host.c: whether a spec is legal, the cell of a pixel, rotations, the distance of a
 * dictionary, the greedy generator, the image of a code, the upright quad) under AddressSanitizer + UndefinedBehaviorSanitizer, as a plain process: built and run by
 * tests/test_cpu_code.py.  Every pixel of sizes at the legality bounds and at 1024 - no cell is empty, the counts add up -, payloads with bit 63 set - where a shift
 * by 64 or a signed shift would be reported -, dictionaries of exactly the size asked for in heap blocks of exactly that size, images in blocks of exactly their
 * size.  A sanitizer report ends the process with a non-zero exit code. */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rectdetect_hip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) fprintf(stderr, "code_host_check: line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static void every_pixel(const rd_code_spec *s, int pw, int ph) {
  const int C = s->n + 2 * s->border;
  int cnt[144] = { 0 }, all[144] = { 0 };
  CHECK(rd_code_spec_ok(s, pw, ph) == 1 && rd_code_bytes(s, pw, ph) == 48);
  for (int j = 0; j < ph; j++)
    for (int i = 0; i < pw; i++) {
      int counted = -5;
      const int cell = rd_code_cell_of(s, pw, ph, i, j, &counted);
      CHECK(cell >= 0 && cell < C * C && (counted == 0 || counted == 1));
      if (cell < 0 || cell >= C * C) return;
      CHECK(cell == rd_code_cell_of(s, pw, ph, i, j, NULL));
      all[cell]++; cnt[cell] += counted;
      if (s->inset == 0) CHECK(counted == 1);
    }
  long total = 0;
  for (int c = 0; c < C * C; c++) { CHECK(cnt[c] >= 1 && cnt[c] <= all[c]); total += all[c]; }
  CHECK(total == (long)pw * ph);
  int counted = -5;
  CHECK(rd_code_cell_of(s, pw, ph, -1, 0, &counted) == -1 && rd_code_cell_of(s, pw, ph, pw, 0, &counted) == -1 && rd_code_cell_of(s, pw, ph, 0, -1, &counted) == -1 &&
        rd_code_cell_of(s, pw, ph, 0, ph, &counted) == -1 && counted == -5);
}

int main(void) {
  int32_t lim[10];
  for (int k = 0; k < 10; k++) lim[k] = -7;
  rd_code_limits(lim + 1);
  CHECK(lim[0] == -7 && lim[9] == -7);
  CHECK(lim[1] == 3 && lim[2] == 8 && lim[3] == 2 && lim[4] == 3 && lim[5] == 7 && lim[6] == 1024 && lim[7] == 4096 && lim[8] == 48);
  CHECK(sizeof(rd_code_spec) == 32 && sizeof(rd_code) == 48 && offsetof(rd_code, id) == 8 && offsetof(rd_code, reserved) == 44);

  /* legal and illegal specs */
  const rd_code_spec ok = { 6, 1, 2, 0, 1, 32, 0, 0 };
  rd_code_spec bad;
  CHECK(rd_code_spec_ok(&ok, 64, 64) == 1 && rd_code_spec_ok(NULL, 64, 64) == 0 && rd_code_bytes(NULL, 64, 64) == 0 && rd_code_cell_of(NULL, 64, 64, 0, 0, NULL) == -1);
  CHECK(rd_code_spec_ok(&ok, 32, 32) == 1 && rd_code_spec_ok(&ok, 31, 32) == 0 && rd_code_spec_ok(&ok, 32, 31) == 0 && rd_code_spec_ok(&ok, 1024, 1024) == 1 &&
        rd_code_spec_ok(&ok, 1025, 64) == 0 && rd_code_spec_ok(&ok, 64, 1025) == 0);
  bad = ok; bad.inset = 0; CHECK(rd_code_spec_ok(&bad, 8, 8) == 1 && rd_code_spec_ok(&bad, 7, 8) == 0 && rd_code_spec_ok(&bad, 8, 7) == 0);
  static const int32_t wrong[8][4] = { { 2, 9, -1, 0 }, { 0, 3, -1, 0 }, { -1, 4, -1, 4 }, { -1, 2, -1, 2 }, { 0, 3, 8, -1 }, { -1, 256, -1, 256 }, { -1, 29, -1, 29 }, { -1, 37, -1, 37 } };
  for (int field = 0; field < 8; field++)
    for (int k = 0; k < 4; k++) {
      bad = ok;
      ((int32_t *)&bad)[field] = wrong[field][k];
      CHECK(rd_code_spec_ok(&bad, 64, 64) == 0 && rd_code_bytes(&bad, 64, 64) == 0 && rd_code_cell_of(&bad, 64, 64, 1, 1, NULL) == -1);
    }
  static const int32_t right[8][4] = { { 3, 4, 7, 8 }, { 1, 2, 1, 2 }, { 0, 1, 2, 3 }, { 0, 1, 0, 1 }, { 1, 2, 4, 4 }, { 0, 1, 254, 255 }, { 0, 1, 27, 28 }, { 0, 1, 35, 36 } };
  for (int field = 2; field < 8; field++)
    for (int k = 0; k < 4; k++) {
      bad = ok;
      ((int32_t *)&bad)[field] = right[field][k];
      CHECK(rd_code_spec_ok(&bad, 64, 64) == 1);
    }

  /* every pixel: at the bounds of legality, at sizes that are no multiple of anything, at the largest */
  for (int n = 3; n <= 8; n++)
    for (int border = 1; border <= 2; border++)
      for (int inset = 0; inset <= 3; inset++) {
        const rd_code_spec s = { n, border, inset, 0, 1, 0, 0, 0 };
        const int C = n + 2 * border, least = inset ? 4 * C : C;
        every_pixel(&s, least, least);
        every_pixel(&s, least + 1, least + 3);
        every_pixel(&s, 100, 52);
        CHECK(rd_code_spec_ok(&s, least - 1, least) == 0 && rd_code_spec_ok(&s, least, least - 1) == 0);
      }
  { const rd_code_spec s = { 3, 1, 0, 0, 1, 0, 0, 0 }; every_pixel(&s, 1024, 5); every_pixel(&s, 5, 1024); }
  { const rd_code_spec s = { 8, 2, 3, 0, 1, 0, 0, 0 }; every_pixel(&s, 1024, 1023); }

  /* rotations: four are the identity, bit 63 travels, bits above n * n are dropped */
  for (int n = 3; n <= 8; n++) {
    const uint64_t mask = n == 8 ? ~(uint64_t)0 : (((uint64_t)1 << (n * n)) - 1);
    uint64_t v = 0x9E3779B97F4A7C15ull;
    for (int t = 0; t < 50; t++) {
      v = v * 6364136223846793005ull + 1442695040888963407ull;
      const uint64_t p = v & mask;
      CHECK(rd_code_rotate(rd_code_rotate(rd_code_rotate(rd_code_rotate(p, n, 1), n, 1), n, 1), n, 1) == p);
      CHECK(rd_code_rotate(p, n, 4) == p && rd_code_rotate(p, n, 0) == p && rd_code_rotate(p, n, -1) == rd_code_rotate(p, n, 3) && rd_code_rotate(p, n, 2) == rd_code_rotate(rd_code_rotate(p, n, 1), n, 1));
      CHECK(rd_code_rotate(v, n, 1) == rd_code_rotate(p, n, 1) && (rd_code_rotate(v, n, 1) & ~mask) == 0);
      CHECK(__builtin_popcountll(rd_code_rotate(p, n, 1)) == __builtin_popcountll(p));
    }
    CHECK(rd_code_rotate(1, n, 1) == (uint64_t)1 << (n - 1));      /* the top-left cell turns to the top-right */
  }
  CHECK(rd_code_rotate(~(uint64_t)0, 8, 1) == ~(uint64_t)0 && rd_code_rotate((uint64_t)1 << 63, 8, 1) == (uint64_t)1 << 56 && rd_code_rotate((uint64_t)1 << 56, 8, 1) == 1);
  CHECK(rd_code_rotate(5, 2, 1) == 0 && rd_code_rotate(5, 9, 1) == 0);

  /* distance and the generator, in blocks of exactly their size */
  CHECK(rd_code_distance(NULL, 0, 6) == 65 && rd_code_distance(NULL, 1, 6) == -1 && rd_code_distance(NULL, 0, 2) == -1);
  for (int n = 3; n <= 8; n++) {
    const int count = n == 3 ? 4 : 40, min_dist = n - 1;
    uint64_t *d = (uint64_t *)malloc(sizeof(uint64_t) * count), *e = (uint64_t *)malloc(sizeof(uint64_t) * count);
    const int got = rd_code_dictionary(n, count, min_dist, 12345, 200000, d);
    CHECK(got == count);
    CHECK(rd_code_dictionary(n, count, min_dist, 12345, 200000, e) == got && memcmp(d, e, sizeof(uint64_t) * got) == 0);
    CHECK(rd_code_distance(d, got, n) >= min_dist);
    CHECK(rd_code_dictionary(n, count, min_dist, 12345, 0, e) == 0 && rd_code_dictionary(n, 0, min_dist, 12345, 10, NULL) == 0);
    if (got > 1) { e[got - 1] = rd_code_rotate(e[0], n, 3); CHECK(rd_code_distance(e, got, n) == 0); }
    if (n < 8) { e[0] |= (uint64_t)1 << (n * n); CHECK(rd_code_distance(e, got, n) == -1); }
    free(d); free(e);
  }
  { uint64_t one = ~(uint64_t)0; CHECK(rd_code_distance(&one, 1, 8) == 0); one = 1; CHECK(rd_code_distance(&one, 1, 8) == 2); }
  { uint64_t tmp[1] = { 77 };
    CHECK(rd_code_dictionary(2, 1, 1, 0, 1, tmp) == -1 && rd_code_dictionary(6, 4097, 1, 0, 1, tmp) == -1 && rd_code_dictionary(6, 1, -1, 0, 1, tmp) == -1 &&
          rd_code_dictionary(6, 1, 1, 0, -1, tmp) == -1 && rd_code_dictionary(6, 1, 1, 0, 1, NULL) == -1 && tmp[0] == 77); }

  /* the image of a code, in a block of exactly its size */
  for (int n = 3; n <= 8; n++)
    for (int border = 1; border <= 2; border++)
      for (int pol = 0; pol <= 1; pol++) {
        const rd_code_spec s = { n, border, 0, pol, 1, 0, 0, 0 };
        const int C = n + 2 * border, px = 3, S = C * px;
        const uint64_t bits = n == 8 ? ~(uint64_t)0 : (((uint64_t)1 << (n * n)) - 1) & 0xA5A5F00F3C3C9669ull;
        uint8_t *img = (uint8_t *)malloc((size_t)S * S);
        CHECK(rd_code_render(&s, bits, px, img) == (size_t)S * S);
        CHECK(img[0] == (pol ? 255 : 0) && img[(size_t)S * S - 1] == (pol ? 255 : 0));
        for (int r = 0; r < n; r++)
          for (int c = 0; c < n; c++) CHECK(img[(size_t)((border + r) * px + 1) * S + (border + c) * px + 1] == ((((bits >> (r * n + c)) & 1) ^ (uint64_t)pol) ? 255 : 0));
        CHECK(rd_code_render(&s, bits, 0, img) == 0 && rd_code_render(&s, bits, 65, img) == 0 && rd_code_render(NULL, bits, px, img) == 0 && rd_code_render(&s, bits, px, NULL) == 0);
        if (n < 8) CHECK(rd_code_render(&s, (uint64_t)1 << (n * n), px, img) == 0);
        free(img);
      }

  /* the upright quad */
  const double quad[8] = { 0, 1, 2, 3, 4, 5, 6, 7 };
  double out[10];
  for (int rot = -4; rot <= 8; rot++) {
    for (int k = 0; k < 10; k++) out[k] = -7;
    rd_code_upright(quad, rot, out + 1);
    CHECK(out[0] == -7 && out[9] == -7);
    const int r = ((rot % 4) + 4) % 4;
    for (int c = 0; c < 4; c++) CHECK(out[1 + 2 * c] == quad[2 * ((c + 4 - r) % 4)] && out[2 + 2 * c] == quad[2 * ((c + 4 - r) % 4) + 1]);
  }
  rd_code_upright(NULL, 1, out); rd_code_upright(quad, 1, NULL);

  if (failures) { fprintf(stderr, "code_host_check: %d failure(s)\n", failures); return 1; }
  printf("code_host_check: ok\n");
  return 0;
}
