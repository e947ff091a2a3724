/* rectdetect-mi355x: matched quads - the host's part of the contract in include/rectdetect_hip.h ("matched quads"): the score of a record from the integers the
 * device returned, and the limits.  int64 and IEEE double, exactly the operations the header writes, never contracted (-ffp-contract=off).  No HIP in here:
 * tests/native/match_host_check.c builds this file alone under the sanitizers. */
#include "rectdetect_hip.h"
#include <math.h>
#include <string.h>

/* num / sqrt(va * vb) of one column; va > 0 and vb > 0 (a flat signature has status 2, a flat template is never in the library) */
static double score_of(int64_t D, int32_t dot, int32_t sa, int64_t va, int32_t sb, int64_t sbb) {
  const int64_t num = D * (int64_t)dot - (int64_t)sa * (int64_t)sb;
  const int64_t vb = D * sbb - (int64_t)sb * (int64_t)sb;
  return (double)num / sqrt((double)va * (double)vb);
}

void rd_match_score(rd_match *rec, int grid, int32_t sb, int64_t sbb, int32_t sb2, int64_t sbb2) {
  if (rec->status != 1) {
    const int32_t status = rec->status;
    memset(rec, 0, sizeof(*rec));
    rec->status = status;
    return;
  }
  const int64_t D = (int64_t)grid * grid;
  const int64_t va = D * rec->saa - (int64_t)rec->sa * (int64_t)rec->sa;
  rec->score = score_of(D, rec->dot, rec->sa, va, sb, sbb);
  rec->score2 = rec->tmpl2 >= 0 ? score_of(D, rec->dot2, rec->sa, va, sb2, sbb2) : 0.0;
}

void rd_match_limits(int32_t out[4]) {
  out[0] = 8 | 16 | 32 | 64; out[1] = 1 | 2 | 4; out[2] = RD_MATCH_MAX_TEMPLATES; out[3] = RD_MATCH_MAX_QUADS;
}
