/* TEST INFRASTRUCTURE.  The matcher's host-only code (csrc/rd_match_host.c: the score of a record, the limits) under AddressSanitizer + UndefinedBehaviorSanitizer,
 * as a plain process: built and run by tests/test_cpu_match.py.  The extreme integers of the contract - every cell -128 or 127, all but one, a runner-up and none,
 * every status - and a few exact expectations.  A sanitizer report ends the process with a non-zero exit code. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "rectdetect_hip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "match_host_check: line %d: %s\n", __LINE__, #c); failures++; } } while (0)

/* sums of a signature of D cells: n of them v, one of them w */
static void sums_of(int D, int v, int w, int32_t *s, int64_t *ss) {
  *s = (int32_t)((D - 1) * v + w);
  *ss = (int64_t)(D - 1) * v * v + (int64_t)w * w;
}

int main(void) {
  int32_t lim[4];
  rd_match_limits(lim);
  CHECK(lim[0] == (8 | 16 | 32 | 64) && lim[1] == (1 | 2 | 4) && lim[2] == RD_MATCH_MAX_TEMPLATES && lim[3] == RD_MATCH_MAX_QUADS);
  CHECK(sizeof(rd_match) == 56);

  static const int grids[4] = { 8, 16, 32, 64 }, ext[2] = { -128, 127 };
  for (int g = 0; g < 4; g++) {
    const int G = grids[g], D = G * G;
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2; b++)
        for (int wa = 0; wa < 2; wa++)
          for (int wb = 0; wb < 2; wb++) {
            /* quad: all cells ext[a] but the first, which is ext[wa]; template: all ext[b] but the LAST, ext[wb]: flat when the odd one equals the rest */
            rd_match r;
            memset(&r, 0, sizeof(r));
            int32_t sb; int64_t sbb;
            sums_of(D, ext[a], ext[wa], &r.sa, &r.saa);
            sums_of(D, ext[b], ext[wb], &sb, &sbb);
            if (a == wa || b == wb) continue;      /* (flat: never scored) */
            r.status = 1; r.tmpl = 3; r.rot = 2; r.tmpl2 = -1;
            r.dot = (int32_t)((int64_t)(D - 2) * ext[a] * ext[b] + ext[wa] * ext[b] + ext[a] * ext[wb]);
            r.dot2 = 12345;      /* ignored without a runner-up */
            rd_match_score(&r, G, sb, sbb, 0, 0);
            CHECK(isfinite(r.score) && fabs(r.score) <= 1.0 + 1e-12 && r.score2 == 0.0 && r.tmpl == 3 && r.rot == 2);
            /* two signatures that differ from a constant in different single cells: correlation -1 / (D - 1) when both steps go the same way, else 1 / (D - 1) */
            CHECK(fabs(r.score - ((wa > a) == (wb > b) ? -1.0 : 1.0) / (D - 1)) < 1e-12);
            /* with a runner-up that is the quad itself: score2 = 1 */
            r.tmpl2 = 0; r.rot2 = 1; r.dot2 = (int32_t)r.saa;
            rd_match_score(&r, G, sb, sbb, r.sa, r.saa);
            CHECK(r.score2 == 1.0);
          }
    /* the greatest dot there is: every cell -128 in both but one cell, D * 2^14 = 2^26 at G = 64 */
    rd_match r;
    memset(&r, 0, sizeof(r));
    r.status = 1; r.tmpl2 = -1;
    sums_of(D, -128, 127, &r.sa, &r.saa);
    r.dot = (int32_t)r.saa;
    rd_match_score(&r, G, r.sa, r.saa, 0, 0);
    CHECK(r.score == 1.0);
    /* statuses 0, 2 and 3: everything else is zeroed */
    for (int st = 0; st < 4; st++) {
      if (st == 1) continue;
      rd_match z;
      memset(&z, 0x5a, sizeof(z));
      z.status = st;
      rd_match_score(&z, G, 1, 2, 3, 4);
      rd_match want;
      memset(&want, 0, sizeof(want));
      want.status = st;
      CHECK(memcmp(&z, &want, sizeof(z)) == 0);
    }
  }
  if (failures) { fprintf(stderr, "match_host_check: %d check(s) failed\n", failures); return 1; }
  printf("match_host_check: ok\n");
  return 0;
}
