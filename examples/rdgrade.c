/* rdgrade - is this frame's view of each detected rectangle worth keeping?  rdscan's sequence with a grade spec on the command line.  rdrect's call sequence on one
 * still image (the reference's C API, rect.cpp:47-138, image decoded by rdimage.c), then every rectangle graded by a rectifier made with rd_rectifier_create_grade
 * (rectdetect_hip.h, "graded quads"): per cell how many pixels are black, blown out and on an edge, and the variance of the Laplacian; from the histogram the 1st and
 * the 99th percentile.  A patch is `width` pixels wide and as high as the rectangle's estimated pose makes it: height = round(width * rd_rect_aspect), at least
 * `cells` - so every rectangle has a rectifier of its own.
 *
 *   rdgrade <image.ppm|png> [device number] [width] [cells] [dark] [bright] [edge] [oversample]
 *
 * Defaults: 128 wide, 4 x 4 cells, dark 8, bright 247, edge 64, oversample 1.  Prints a line per rectangle, a line per cell and a line for the whole patch; doubles
 * with %.17g, so that they can be compared bit for bit.  Links against librectdetect_hip.so only. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <CL/cl.h>
#include "helper.h"
#include "oclhelper.h"
#include "oclimgutil.h"
#include "oclpolyline.h"
#include "vec234.h"
#include "oclrect.h"
#include "rectdetect_hip.h"
#include "rdimage.h"

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "Usage : %s <image file name (.ppm or .png)> [device number] [width] [cells] [dark] [bright] [edge] [oversample]\n\nAvailable devices :\n", argv[0]);
    simpleGetDevice(-1);
    return 1;
  }
  const int did = argc >= 3 ? atoi(argv[2]) : 0;
  const int pw = argc >= 4 ? atoi(argv[3]) : 128;
  rd_grade_spec spec = { 4, 8, 247, 64, 1, 1, { 0, 0 } };      /* with the histogram */
  if (argc >= 5) spec.cells = atoi(argv[4]);
  if (argc >= 6) spec.dark = atoi(argv[5]);
  if (argc >= 7) spec.bright = atoi(argv[6]);
  if (argc >= 8) spec.edge = atoi(argv[7]);
  if (argc >= 9) spec.oversample = atoi(argv[8]);
  if (!rd_grade_spec_ok(&spec, pw, spec.cells)) { fprintf(stderr, "%s: not a legal grade spec for patches %d wide\n", argv[0], pw); return 1; }

  cl_device_id device = simpleGetDevice(did);
  printf("%s\n", getDeviceName(device));
  cl_context context = simpleCreateContext(device);
  cl_command_queue queue = clCreateCommandQueue(context, device, CL_QUEUE_PROFILING_ENABLE, NULL);

  rdimage img;
  if (rdimage_load(argv[1], &img) != 0) return 1;

  struct oclimgutil_t *iu = init_oclimgutil(device, context);
  struct oclpolyline_t *pl = init_oclpolyline(device, context);
  struct oclrect_t *rc = init_oclrect(iu, pl, device, context, queue, img.iw, img.ih);

  const double tanAOV = tan(72.0 / 2 / 180.0 * M_PI);
  rect_t *ret = oclrect_executeOnce(rc, img.bgr, img.ws, tanAOV);
  const int n = ret->nItems - 1;      /* element 0 is the header */
  printf("%d rectangle(s)\n", n);

  const void *const planes[3] = { img.bgr, NULL, NULL };
  const int pitches[3] = { img.ws, 0, 0 };
  for (int i = 0; i < n; i++) {
    const double aspect = rd_rect_aspect(&ret[i + 1]), h = floor(pw * aspect + 0.5);      /* height / width of the estimated pose */
    const int most = 16384 / spec.oversample, ph = !(h >= spec.cells) ? spec.cells : (h > most ? most : (int)h);
    rd_rectifier *rf = rd_rectifier_create_grade(did, pw, ph, 1, 1, &spec);
    if (!rf) { fprintf(stderr, "rd_rectifier_create_grade(%d, %d, %d, 1, 1): bad arguments\n", did, pw, ph); return 1; }
    double quad[8];
    rd_rect_quads(ret + 1 + i, 1, quad);      /* c2[0], c2[3], c2[2], c2[1]: clockwise on screen, not mirrored */
    const size_t bytes = rd_rectifier_patch_bytes(rf);
    uint8_t *out = (uint8_t *)rd_host_alloc(bytes), status = 0;      /* pinned (and aligned): the copy engine writes the records here */
    if (rd_rectifier_enqueue(rf, RD_PIX_BGR, planes, pitches, img.iw, img.ih, RD_FRAME_HOST, quad, 1, out, RD_FRAME_HOST_PINNED) < 0) {
      fprintf(stderr, "rd_rectifier_enqueue: argument error\n");
      return 1;
    }
    rd_rectifier_wait(rf, &status);
    const rd_grade_cell *cells = (const rd_grade_cell *)out;
    const uint32_t *hist = (const uint32_t *)(out + sizeof(rd_grade_cell) * (size_t)(spec.cells * spec.cells));
    printf("rect %d status %u aspect %.4f patch %d x %d cells %d bytes %zu%s\n", i, ret[i + 1].status, aspect, pw, ph, spec.cells, bytes, status ? "" : " (not a convex quad: zeros)");
    rd_grade_cell all;
    memset(&all, 0, sizeof(all));
    for (int c = 0; c < spec.cells * spec.cells; c++) {
      const rd_grade_cell *r = &cells[c];
      printf("  rect %d cell %d %d : n %d lo %d hi %d ne %d sharpness %.17g\n", i, c % spec.cells, c / spec.cells, r->n, r->lo, r->hi, r->ne, rd_grade_sharpness(r));
      all.n += r->n; all.lo += r->lo; all.hi += r->hi; all.ne += r->ne; all.sg += r->sg; all.sgg += r->sgg; all.sl += r->sl; all.sll += r->sll;
    }
    printf("  rect %d whole : n %d lo %d hi %d ne %d sharpness %.17g p1 %d p99 %d\n", i, all.n, all.lo, all.hi, all.ne, rd_grade_sharpness(&all), rd_grade_percentile(hist, 1, 100), rd_grade_percentile(hist, 99, 100));
    rd_host_free(out);
    rd_rectifier_destroy(rf);
  }
  free(ret);

  dispose_oclrect(rc);
  dispose_oclpolyline(pl);
  dispose_oclimgutil(iu);
  ce(clReleaseCommandQueue(queue));
  ce(clReleaseContext(context));
  rdimage_free(&img);
  return 0;
}
