/* rectdetect-mi355x: graded quads - the host's part of the contract in include/rectdetect_hip.h ("graded quads"): whether a spec is legal, the bytes of a quad's
 * output, the cell of a pixel, the limits, and the two figures callers derive from the records: the variance of the Laplacian and a percentile of the histogram.
 * No HIP in here: tests/native/grade_host_check.c builds this file alone under the sanitizers. */
#include "rectdetect_hip.h"
#include "rd_grade_tile.h"

int rd_grade_spec_ok(const rd_grade_spec *spec, int pw, int ph) {
  if (!spec) return 0;
  if (spec->cells != 1 && spec->cells != 2 && spec->cells != 4 && spec->cells != RD_GRADE_MAX_CELLS) return 0;
  if (spec->dark < 0 || spec->dark > 255 || spec->bright < 0 || spec->bright > 255 || spec->edge < 0 || spec->edge > RD_GRADE_MAX_EDGE) return 0;
  if (spec->oversample != 1 && spec->oversample != 2 && spec->oversample != 4) return 0;
  if ((spec->hist != 0 && spec->hist != 1) || spec->reserved[0] != 0 || spec->reserved[1] != 0) return 0;
  return pw >= spec->cells && ph >= spec->cells && pw <= 16384 / spec->oversample && ph <= 16384 / spec->oversample;
}

size_t rd_grade_bytes(const rd_grade_spec *spec, int pw, int ph) {
  if (!rd_grade_spec_ok(spec, pw, ph)) return 0;
  return sizeof(rd_grade_cell) * (size_t)(spec->cells * spec->cells) + (spec->hist ? 256 * sizeof(uint32_t) : 0);
}

int rd_grade_cell_of(const rd_grade_spec *spec, int pw, int ph, int i, int j) {
  if (!rd_grade_spec_ok(spec, pw, ph) || i < 0 || i >= pw || j < 0 || j >= ph) return -1;
  return ((j * spec->cells) / ph) * spec->cells + (i * spec->cells) / pw;      /* at most 16383 * 8 */
}

void rd_grade_limits(int32_t out[8]) {
  out[0] = 1 | 2 | 4 | RD_GRADE_MAX_CELLS;
  out[1] = 1 | 2 | 4;
  out[2] = RD_GRADE_MAX_EDGE;
  out[3] = RD_GRADE_TILE_W;
  out[4] = RD_GRADE_TILE_H;
  out[5] = (int32_t)sizeof(rd_grade_cell);
  out[6] = (int32_t)(256 * sizeof(uint32_t));
  out[7] = 0;
}

double rd_grade_sharpness(const rd_grade_cell *cell) {
  if (!cell || cell->n == 0) return 0.0;
  const double n = (double)cell->n, sl = (double)cell->sl, sll = (double)cell->sll;
  const double sq = sl * sl;
  const double mean_sq = sq / n;
  const double d = sll - mean_sq;
  return d / n;
}

int rd_grade_percentile(const uint32_t hist[256], int num, int den) {
  if (!hist || den < 1 || den > (1 << 20) || num < 0 || num > den) return -1;
  int64_t total = 0, cum = 0;
  for (int v = 0; v < 256; v++) total += hist[v];
  if (total == 0) return -1;
  for (int v = 0; v < 256; v++) {
    cum += hist[v];
    if (cum * den >= num * total) return v;      /* below 2^40 * 2^20 */
  }
  return 255;      /* (not reached: cum == total at v = 255 and num <= den) */
}
