/* rdblobs - the detected rectangles' pages as objects: rdscan's sequence with a blob spec on the command line.  rdrect's call sequence on one still image (the
 * reference's C API, rect.cpp:47-138, image decoded by rdimage.c), then every rectangle's connected ink regions from a rectifier made with
 * rd_rectifier_create_blobs (rectdetect_hip.h, "page components").  A page is `width` pixels wide and as high as the rectangle's estimated pose makes it, exactly
 * as rdscan sizes it - at most (1 << 22) / width rows -, so every page has a rectifier of its own.
 *
 *   rdblobs <image.ppm|png> [device number] [output prefix] [width] [radius] [k] [d] [oversample] [invert] [connectivity] [min_area] [max_area] [max_blobs]
 *
 * Prints one line per page with its head and one line per component with its box, and writes <prefix>K.pbm ("P4"): the cleaned page - what rdscan would have
 * written as page_K.pbm with the components outside [min_area, max_area] removed.  Defaults: "clean_", 256 wide, radius 15, k 26, d 0, oversample 1, invert 0,
 * connectivity 8, min_area 4, max_area 0 (no upper bound), max_blobs 64.  Links against librectdetect_hip.so only. */
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
    fprintf(stderr, "Usage : %s <image file name (.ppm or .png)> [device number] [output prefix] [width] [radius] [k] [d] [oversample] [invert] [connectivity] [min_area] [max_area] [max_blobs]\n\n"
            "Available devices :\n", argv[0]);
    simpleGetDevice(-1);
    return 1;
  }
  const int did = argc >= 3 ? atoi(argv[2]) : 0;
  const char *prefix = argc >= 4 ? argv[3] : "clean_";
  const int pw = argc >= 5 ? atoi(argv[4]) : 256;
  rd_blob_spec spec = { 15, 26, 0, 1, 0, 8, 4, 0, 64, 1, { 0, 0 } };
  int32_t *const fields[9] = { &spec.radius, &spec.k, &spec.d, &spec.oversample, &spec.invert, &spec.connectivity, &spec.min_area, &spec.max_area, &spec.max_blobs };
  for (int k = 0; k < 9 && 5 + k < argc; k++) *fields[k] = atoi(argv[5 + k]);
  if (!rd_blob_spec_ok(&spec, pw, 1)) { fprintf(stderr, "%s: not a legal blob spec for pages %d wide\n", argv[0], pw); return 1; }

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
    int most = 16384 / spec.oversample;
    if (most > (1 << 22) / pw) most = (1 << 22) / pw;
    const int ph = !(h >= 1.0) ? 1 : (h > most ? most : (int)h);
    rd_rectifier *rf = rd_rectifier_create_blobs(did, pw, ph, 1, 1, &spec);
    if (!rf) { fprintf(stderr, "rd_rectifier_create_blobs(%d, %d, %d, 1, 1): bad arguments\n", did, pw, ph); return 1; }
    double quad[8];
    rd_rect_quads(ret + 1 + i, 1, quad);      /* c2[0], c2[3], c2[2], c2[1]: clockwise on screen, not mirrored */
    const size_t bytes = rd_rectifier_patch_bytes(rf), page_bytes = (size_t)((pw + 7) >> 3) * ph;
    uint8_t *out = (uint8_t *)rd_host_alloc(bytes), status = 0;      /* pinned (and 8-byte aligned): the copy engine writes the records here */
    if (rd_rectifier_enqueue(rf, RD_PIX_BGR, planes, pitches, img.iw, img.ih, RD_FRAME_HOST, quad, 1, out, RD_FRAME_HOST_PINNED) < 0) {
      fprintf(stderr, "rd_rectifier_enqueue: argument error\n");
      return 1;
    }
    rd_rectifier_wait(rf, &status);
    const rd_blob_head *head = (const rd_blob_head *)out;
    const rd_blob *recs = (const rd_blob *)(head + 1);
    char name[1024];
    snprintf(name, sizeof(name), "%s%d.pbm", prefix, i);
    FILE *f = fopen(name, "wb");
    if (!f || fprintf(f, "P4\n%d %d\n", pw, ph) < 0 || fwrite((const uint8_t *)(recs + spec.max_blobs), 1, page_bytes, f) != page_bytes || fclose(f) != 0) {
      fprintf(stderr, "%s: cannot write %s\n", argv[0], name);
      return 1;
    }
    printf("status %u aspect %.4f page %d x %d ink %d all %d found %d written %d ink_kept %d largest %d flags %d %s %s\n", ret[i + 1].status, aspect, pw, ph, head->ink, head->all,
           head->found, head->written, head->ink_kept, head->largest, head->flags, status ? "->" : "(not a convex quad: zeros) ->", name);
    for (int k = 0; k < head->written; k++)
      printf("  blob %d box %d %d %d %d area %d first %d sx %lld sy %lld\n", k, recs[k].x0, recs[k].y0, recs[k].x1, recs[k].y1, recs[k].area, recs[k].first, (long long)recs[k].sx, (long long)recs[k].sy);
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
