/* rdpatches - what is INSIDE the detected rectangles: rdrect's call sequence on one still image (the reference's C API, rect.cpp:47-138, image decoded by
 * rdimage.c), then every rectangle's contents as an upright patch of fixed size from the rectifier (rectdetect_hip.h: rd_rect_quads, rd_rectifier_*), one
 * PPM per rectangle.
 *
 *   rdpatches <image.ppm|png> [device number] [output prefix] [patch width] [patch height]
 *
 * Writes <prefix>NN.ppm (default prefix "patch", 128 x 128 pixels) and prints one line per rectangle: status, the aspect ratio of its estimated pose
 * (rd_rect_aspect: height / width in the orientation of rd_rect_quads - a caller with one rectifier per shape would pick the patch shape from it), the file.  Links against librectdetect_hip.so only. */
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
  if (argc < 2) {
    fprintf(stderr, "Usage : %s <image file name (.ppm or .png)> [device number] [output prefix] [patch width] [patch height]\n\nAvailable devices :\n", argv[0]);
    simpleGetDevice(-1);
    return 1;
  }
  const int did = argc >= 3 ? atoi(argv[2]) : 0;
  const char *prefix = argc >= 4 ? argv[3] : "patch";
  const int pw = argc >= 5 ? atoi(argv[4]) : 128, ph = argc >= 6 ? atoi(argv[5]) : pw;
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

  if (n > 0) {
    rd_rectifier *rf = rd_rectifier_create(did, pw, ph, n, 1);
    if (!rf) { fprintf(stderr, "rd_rectifier_create(%d, %d, %d, %d, 1): bad arguments\n", did, pw, ph, n); return 1; }
    double *quads = (double *)malloc(sizeof(double) * 8 * n);
    rd_rect_quads(ret + 1, n, quads);      /* c2[0], c2[3], c2[2], c2[1]: clockwise on screen, patches not mirrored */
    const size_t patch = (size_t)pw * ph * 3;
    uint8_t *out = (uint8_t *)rd_host_alloc(patch * n);      /* pinned: the copy engine writes the patches here */
    uint8_t *status = (uint8_t *)malloc(n);
    const void *const planes[3] = { img.bgr, NULL, NULL };
    const int pitches[3] = { img.ws, 0, 0 };
    if (rd_rectifier_enqueue(rf, RD_PIX_BGR, planes, pitches, img.iw, img.ih, RD_FRAME_HOST, quads, n, out, RD_FRAME_HOST_PINNED) < 0) {
      fprintf(stderr, "rd_rectifier_enqueue: argument error\n");
      return 1;
    }
    rd_rectifier_wait(rf, status);
    for (int i = 0; i < n; i++) {
      char name[1024];
      snprintf(name, sizeof(name), "%s%02d.ppm", prefix, i);
      rdimage p = { pw, ph, pw * 3, out + patch * i };
      rdimage_save_ppm(name, &p);
      printf("status %u aspect %.4f patch %s %s\n", ret[i + 1].status, rd_rect_aspect(&ret[i + 1]), status[i] ? "->" : "(not a convex quad: zeros) ->", name);
    }
    free(status); free(quads);
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
