/* rectdetect-mi355x: page components - the host's part of the contract in include/rectdetect_hip.h ("page components"): whether a spec is legal, the bytes of a
 * quad's output, the limits, and steps 2-7 for one page of packed bits (rd_blob_page_host): the contract's statement in C and the host baseline of
 * tools/bench_blobs.py.  Integers only.  No HIP in here: tests/native/blob_host_check.c builds this file alone under the sanitizers.
 *
 * rd_blob_page_host works on RUNS (maximal horizontal stretches of ink in a row), numbered in raster order: a union-find over runs whose hooks go towards the
 * smaller number, so that a root is the component's first run and `first` its first pixel; runs of neighbouring rows are joined by one sweep of two cursors per row
 * pair; the roots are numbered in ascending order - ascending `first` - and every run adds its closed-form sums to its root's record. */
#include "rectdetect_hip.h"
#include "rd_blob_tile.h"
#include <stdlib.h>
#include <string.h>

int rd_blob_spec_ok(const rd_blob_spec *spec, int pw, int ph) {
  if (!spec) return 0;
  if (spec->radius < 0 || spec->radius > RD_BLOB_MAX_RADIUS || spec->k < 0 || spec->k > 255 || spec->d < 0 || spec->d > 255 || (spec->radius == 0 && spec->d != 0)) return 0;
  if (spec->oversample != 1 && spec->oversample != 2 && spec->oversample != 4) return 0;
  if ((spec->invert != 0 && spec->invert != 1) || (spec->connectivity != 4 && spec->connectivity != 8) || (spec->page != 0 && spec->page != 1)) return 0;
  if (spec->min_area < 1 || spec->min_area > RD_BLOB_MAX_PIXELS) return 0;
  if (spec->max_area != 0 && (spec->max_area < spec->min_area || spec->max_area > RD_BLOB_MAX_PIXELS)) return 0;
  if (spec->max_blobs < 1 || spec->max_blobs > RD_BLOB_MAX_BLOBS || spec->reserved[0] != 0 || spec->reserved[1] != 0) return 0;
  if (pw < 1 || ph < 1 || pw > 16384 / spec->oversample || ph > 16384 / spec->oversample) return 0;
  return (int64_t)pw * ph <= RD_BLOB_MAX_PIXELS;
}

size_t rd_blob_bytes(const rd_blob_spec *spec, int pw, int ph) {
  if (!rd_blob_spec_ok(spec, pw, ph)) return 0;
  const size_t page = spec->page ? ((size_t)((pw + 7) >> 3) * (size_t)ph + 7) & ~(size_t)7 : 0;
  return sizeof(rd_blob_head) + sizeof(rd_blob) * (size_t)spec->max_blobs + page;
}

void rd_blob_limits(int32_t out[8]) {
  out[0] = 1 << 4 | 1 << 8;
  out[1] = 1 | 2 | 4;
  out[2] = RD_BLOB_MAX_RADIUS;
  out[3] = RD_BLOB_MAX_BLOBS;
  out[4] = RD_BLOB_MAX_PIXELS;
  out[5] = RD_BLOB_TILE_W;
  out[6] = RD_BLOB_TILE_H;
  out[7] = 0;
}

typedef struct { int32_t x0, x1, j, up; } blob_run;      /* columns x0 .. x1 of row j; up: the run this one hangs under (itself: a root), later the component's number */

static int32_t run_root(blob_run *runs, int32_t a) {
  int32_t r = a;
  while (runs[r].up != r) r = runs[r].up;
  while (runs[a].up != r) { const int32_t next = runs[a].up; runs[a].up = r; a = next; }
  return r;
}

static int page_bit(const uint8_t *row, int i) { return row[i >> 3] >> (7 - (i & 7)) & 1; }

int rd_blob_page_host(const uint8_t *bits, int pw, int ph, const rd_blob_spec *spec, void *out) {
  const size_t bytes = rd_blob_bytes(spec, pw, ph);
  if (!bits || !out || !bytes || ((uintptr_t)out & 7)) return 0;
  const int rb = (pw + 7) >> 3, reach = spec->connectivity == 8 ? 1 : 0;
  /* the runs, row by row: counted first, so that the work space is as large as the page needs and no larger */
  size_t nruns = 0;
  for (int j = 0; j < ph; j++) {
    const uint8_t *row = bits + (size_t)j * rb;
    for (int i = 0, before = 0; i < pw; i++) { const int b = page_bit(row, i); nruns += b && !before; before = b; }
  }
  blob_run *runs = (blob_run *)malloc((nruns ? nruns : 1) * sizeof(blob_run));
  int32_t *row_start = (int32_t *)malloc(((size_t)ph + 1) * sizeof(int32_t));
  if (!runs || !row_start) { free(runs); free(row_start); return 0; }
  int32_t n = 0, ink = 0;
  for (int j = 0; j < ph; j++) {
    const uint8_t *row = bits + (size_t)j * rb;
    row_start[j] = n;
    for (int i = 0; i < pw; i++) {
      if (!page_bit(row, i)) continue;
      const int x0 = i;
      while (i + 1 < pw && page_bit(row, i + 1)) i++;
      runs[n].x0 = x0; runs[n].x1 = i; runs[n].j = j; runs[n].up = n;
      ink += i - x0 + 1;
      n++;
    }
  }
  row_start[ph] = n;
  /* step 2: runs of neighbouring rows that touch belong together */
  for (int j = 1; j < ph; j++) {
    int32_t a = row_start[j - 1], b = row_start[j];
    const int32_t a_end = row_start[j], b_end = row_start[j + 1];
    while (a < a_end && b < b_end) {
      if (runs[a].x0 <= runs[b].x1 + reach && runs[b].x0 <= runs[a].x1 + reach) {
        const int32_t ra = run_root(runs, a), rb2 = run_root(runs, b);
        if (ra < rb2) runs[rb2].up = ra; else if (rb2 < ra) runs[ra].up = rb2;
      }
      if (runs[a].x1 < runs[b].x1) a++; else b++;      /* the run that ends first can touch nothing further on */
    }
  }
  /* the components in ascending `first`: a root is its component's first run, and runs are numbered in raster order */
  int32_t all = 0;
  for (int32_t r = 0; r < n; r++) if (run_root(runs, r) == r) all++;
  rd_blob *comp = (rd_blob *)calloc(all ? (size_t)all : 1, sizeof(rd_blob));
  if (!comp) { free(runs); free(row_start); return 0; }
  all = 0;
  for (int32_t r = 0; r < n; r++) {
    const int32_t root = runs[r].up;      /* (flat after run_root; a root's own field already holds its NUMBER, which is never larger than the root) */
    int32_t c;
    if (root == r) {
      c = all++;
      comp[c].x0 = runs[r].x0; comp[c].y0 = runs[r].j; comp[c].x1 = runs[r].x1; comp[c].y1 = runs[r].j;
      comp[c].first = runs[r].j * pw + runs[r].x0;
    } else c = runs[root].up;
    runs[r].up = c;
    const int64_t len = runs[r].x1 - runs[r].x0 + 1;
    if (runs[r].x0 < comp[c].x0) comp[c].x0 = runs[r].x0;
    if (runs[r].x1 > comp[c].x1) comp[c].x1 = runs[r].x1;
    if (runs[r].j > comp[c].y1) comp[c].y1 = runs[r].j;
    comp[c].area += (int32_t)len;
    comp[c].sx += len * runs[r].x0 + len * (len - 1) / 2;
    comp[c].sy += len * runs[r].j;
  }
  /* steps 3-6 */
  memset(out, 0, bytes);
  rd_blob_head *head = (rd_blob_head *)out;
  rd_blob *recs = (rd_blob *)(head + 1);
  uint8_t *page = (uint8_t *)(recs + spec->max_blobs);
  head->ink = ink; head->all = all;
  for (int32_t c = 0; c < all; c++) {
    const int32_t area = comp[c].area;
    if (area > head->largest) head->largest = area;
    const int kept = spec->min_area <= area && (spec->max_area == 0 || area <= spec->max_area);
    if (kept) {
      if (head->found < spec->max_blobs) recs[head->found] = comp[c];
      head->found++;
      head->ink_kept += area;
    } else comp[c].area = 0;      /* (marks it for the page) */
  }
  head->written = head->found < spec->max_blobs ? head->found : spec->max_blobs;
  head->flags = head->found > spec->max_blobs ? RD_BLOB_OVERFLOW : 0;
  if (spec->page)
    for (int32_t r = 0; r < n; r++) {
      if (!comp[runs[r].up].area) continue;
      uint8_t *row = page + (size_t)runs[r].j * rb;
      for (int i = runs[r].x0; i <= runs[r].x1; i++) row[i >> 3] |= (uint8_t)(0x80 >> (i & 7));
    }
  free(comp); free(runs); free(row_start);
  return 1;
}
