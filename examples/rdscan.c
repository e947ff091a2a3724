/* rdscan - the detected rectangles as scanned pages: rdpatches' sequence with a scan spec on the command line.  rdrect's call sequence on one still image (the
 * reference's C API, rect.cpp:47-138, image decoded by rdimage.c), then every rectangle as a clean page from a rectifier made with rd_rectifier_create_scan
 * (rectdetect_hip.h, "scanned pages").  A page is `width` pixels wide and as high as the rectangle's estimated pose makes it: height = round(width *
 * rd_rect_aspect), at least 1 - so every page has a rectifier of its own.
 *
 *   rdscan <image.ppm|png> [device number] [output prefix] [width] [flat|bilevel|bits] [radius] [k] [d] [white] [oversample] [invert]
 *
 * Writes <prefix>K.pbm (bits: "P4", the job's output verbatim behind the header) or <prefix>K.pgm (flat, bilevel: "P5") - default "page_", 256 wide, bits, radius 15,
 * k 26, d 0, white 230, oversample 1, invert 0 - and prints one line per page.  Links against librectdetect_hip.so only. */
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
  static const char *const modes[3] = { "flat", "bilevel", "bits" };
  if (argc < 2) {
    fprintf(stderr, "Usage : %s <image file name (.ppm or .png)> [device number] [output prefix] [width] [flat|bilevel|bits] [radius] [k] [d] [white] [oversample] [invert]\n\n"
            "Available devices :\n", argv[0]);
    simpleGetDevice(-1);
    return 1;
  }
  const int did = argc >= 3 ? atoi(argv[2]) : 0;
  const char *prefix = argc >= 4 ? argv[3] : "page_";
  const int pw = argc >= 5 ? atoi(argv[4]) : 256;
  rd_scan_spec spec = { RD_SCAN_BITS, 15, 26, 0, 230, 1, 0, 0 };
  if (argc >= 6) { spec.mode = -1; for (int k = 0; k < 3; k++) if (strcmp(argv[5], modes[k]) == 0) spec.mode = k; }
  if (argc >= 7) spec.radius = atoi(argv[6]);
  if (argc >= 8) spec.k = atoi(argv[7]);
  if (argc >= 9) spec.d = atoi(argv[8]);
  if (argc >= 10) spec.white = atoi(argv[9]);
  if (argc >= 11) spec.oversample = atoi(argv[10]);
  if (argc >= 12) spec.invert = atoi(argv[11]);
  if (!rd_scan_spec_ok(&spec, pw, 1)) { fprintf(stderr, "%s: not a legal scan spec for pages %d wide\n", argv[0], pw); return 1; }

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
    const int most = 16384 / spec.oversample, ph = !(h >= 1.0) ? 1 : (h > most ? most : (int)h);
    rd_rectifier *rf = rd_rectifier_create_scan(did, pw, ph, 1, 1, &spec);
    if (!rf) { fprintf(stderr, "rd_rectifier_create_scan(%d, %d, %d, 1, 1): bad arguments\n", did, pw, ph); return 1; }
    double quad[8];
    rd_rect_quads(ret + 1 + i, 1, quad);      /* c2[0], c2[3], c2[2], c2[1]: clockwise on screen, not mirrored */
    const size_t bytes = rd_rectifier_patch_bytes(rf);
    uint8_t *out = (uint8_t *)rd_host_alloc(bytes), status = 0;      /* pinned: the copy engine writes the page here */
    if (rd_rectifier_enqueue(rf, RD_PIX_BGR, planes, pitches, img.iw, img.ih, RD_FRAME_HOST, quad, 1, out, RD_FRAME_HOST_PINNED) < 0) {
      fprintf(stderr, "rd_rectifier_enqueue: argument error\n");
      return 1;
    }
    rd_rectifier_wait(rf, &status);
    char name[1024];
    snprintf(name, sizeof(name), "%s%d.%s", prefix, i, spec.mode == RD_SCAN_BITS ? "pbm" : "pgm");
    FILE *f = fopen(name, "wb");
    const int head = !f ? -1 : (spec.mode == RD_SCAN_BITS ? fprintf(f, "P4\n%d %d\n", pw, ph) : fprintf(f, "P5\n%d %d\n255\n", pw, ph));
    if (head < 0 || fwrite(out, 1, bytes, f) != bytes || fclose(f) != 0) { fprintf(stderr, "%s: cannot write %s\n", argv[0], name); return 1; }
    printf("status %u aspect %.4f page %d x %d %s bytes %zu %s %s\n", ret[i + 1].status, aspect, pw, ph, modes[spec.mode], bytes, status ? "->" : "(not a convex quad: zeros) ->", name);
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
