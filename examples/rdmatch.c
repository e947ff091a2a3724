/* rdmatch - WHICH known picture is inside each detected rectangle: rdrect's call sequence on one still image (the reference's C API, rect.cpp:47-138, images
 * decoded by rdimage.c), then every rectangle matched on the device against a library of template images (rectdetect_hip.h: "matched quads", rd_matcher_*).
 *
 *   rdmatch <frame.ppm|png> <template.ppm|png> [more templates ...]
 *
 * Every template is its whole image.  Prints one line per rectangle: the best template, the quad's corner where the template's first corner lies (rot), the score,
 * and the runner-up.  Device 0, grid 32, oversampling 4.  Links against librectdetect_hip.so only. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
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
  if (argc < 3) {
    fprintf(stderr, "Usage : %s <frame (.ppm or .png)> <template (.ppm or .png)> [more templates ...]\n\nAvailable devices :\n", argv[0]);
    simpleGetDevice(-1);
    return 1;
  }
  const int did = 0, nt = argc - 2;
  cl_device_id device = simpleGetDevice(did);
  printf("%s\n", getDeviceName(device));
  cl_context context = simpleCreateContext(device);
  cl_command_queue queue = clCreateCommandQueue(context, device, CL_QUEUE_PROFILING_ENABLE, NULL);

  rdimage img;
  if (rdimage_load(argv[1], &img) != 0) return 1;

  struct oclimgutil_t *iu = init_oclimgutil(device, context);
  struct oclpolyline_t *pl = init_oclpolyline(device, context);
  struct oclrect_t *rc = init_oclrect(iu, pl, device, context, queue, img.iw, img.ih);
  rect_t *ret = oclrect_executeOnce(rc, img.bgr, img.ws, tan(72.0 / 2 / 180.0 * M_PI));
  const int n = ret->nItems - 1;      /* element 0 is the header */
  printf("%d rectangle(s)\n", n);

  rd_matcher *mt = rd_matcher_create(did, 32, 4, nt, n > 0 ? n : 1, 1);
  if (!mt) { fprintf(stderr, "rd_matcher_create(%d, 32, 4, %d, %d, 1): bad arguments\n", did, nt, n); return 1; }
  int *name_of = (int *)malloc(sizeof(int) * nt);      /* template number -> argv index (a refused template has no number) */
  for (int k = 0; k < nt; k++) {
    rdimage t;
    if (rdimage_load(argv[2 + k], &t) != 0) return 1;
    const void *const planes[3] = { t.bgr, NULL, NULL };
    const int pitches[3] = { t.ws, 0, 0 };
    const int id = rd_matcher_add(mt, RD_PIX_BGR, planes, pitches, t.iw, t.ih, RD_FRAME_HOST, NULL);
    if (id >= 0) name_of[id] = 2 + k;
    else fprintf(stderr, "%s: %s\n", argv[2 + k], id == -2 ? "a flat image, not added" : "not added");
    rdimage_free(&t);
  }
  printf("%d template(s)\n", rd_matcher_templates(mt));

  if (n > 0) {
    double *quads = (double *)malloc(sizeof(double) * 8 * n);
    rd_rect_quads(ret + 1, n, quads);      /* c2[0], c2[3], c2[2], c2[1]: clockwise on screen */
    rd_match *recs = (rd_match *)malloc(sizeof(rd_match) * n);
    const void *const planes[3] = { img.bgr, NULL, NULL };
    const int pitches[3] = { img.ws, 0, 0 };
    if (rd_matcher_enqueue(mt, RD_PIX_BGR, planes, pitches, img.iw, img.ih, RD_FRAME_HOST, quads, n, 0) < 0) {
      fprintf(stderr, "rd_matcher_enqueue: argument error\n");
      return 1;
    }
    rd_matcher_wait(mt, recs, NULL);
    for (int i = 0; i < n; i++) {
      const rd_match *r = &recs[i];
      if (r->status != 1) { printf("rect %d status %d (%s)\n", i, r->status, r->status == 0 ? "not a convex quad" : r->status == 2 ? "a flat area" : "no templates"); continue; }
      printf("rect %d template %d (%s) rot %d score %.6f", i, r->tmpl, argv[name_of[r->tmpl]], r->rot, r->score);
      if (r->tmpl2 >= 0) printf(" runner-up %d (%s) rot %d score %.6f\n", r->tmpl2, argv[name_of[r->tmpl2]], r->rot2, r->score2);
      else printf(" no runner-up\n");
    }
    free(recs); free(quads);
  }
  free(name_of);
  rd_matcher_destroy(mt);
  free(ret);

  dispose_oclrect(rc);
  dispose_oclpolyline(pl);
  dispose_oclimgutil(iu);
  ce(clReleaseCommandQueue(queue));
  ce(clReleaseContext(context));
  rdimage_free(&img);
  return 0;
}
