/* rdtensors - what is INSIDE the detected rectangles, ready for a model: rdpatches with a tensor spec on the command line.  rdrect's call sequence on one still
 * image (the reference's C API, rect.cpp:47-138, image decoded by rdimage.c), then every rectangle's contents as one tensor from a rectifier made with
 * rd_rectifier_create_tensor (rectdetect_hip.h, "model-ready tensors").
 *
 *   rdtensors <image.ppm|png> [device number] [output file] [width] [height] [u8|f16|bf16|f32] [nhwc|nchw] [bgr|rgb|gray] [oversample] [scale] [bias]
 *
 * Writes the raw tensor of all rectangles (default "tensors.raw": 128 x 128, f16, nchw, rgb, oversample 2, scale 1/255, bias 0 - the same scale and bias for every
 * channel) and prints its shape, dtype and bytes, then one line per rectangle.  Links against librectdetect_hip.so only. */
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

/* the index of word in names (n of them), or -1 */
static int pick(const char *word, const char *const *names, int n) {
  for (int k = 0; k < n; k++) if (strcmp(word, names[k]) == 0) return k;
  return -1;
}

int main(int argc, char **argv) {
  static const char *const dtypes[4] = { "u8", "f16", "bf16", "f32" }, *const layouts[2] = { "nhwc", "nchw" }, *const kinds[3] = { "bgr", "rgb", "gray" };
  if (argc < 2) {
    fprintf(stderr, "Usage : %s <image file name (.ppm or .png)> [device number] [output file] [width] [height] [u8|f16|bf16|f32] [nhwc|nchw] [bgr|rgb|gray] [oversample] [scale] [bias]\n\n"
            "Available devices :\n", argv[0]);
    simpleGetDevice(-1);
    return 1;
  }
  const int did = argc >= 3 ? atoi(argv[2]) : 0;
  const char *path = argc >= 4 ? argv[3] : "tensors.raw";
  const int pw = argc >= 5 ? atoi(argv[4]) : 128, ph = argc >= 6 ? atoi(argv[5]) : pw;
  rd_tensor_spec spec;
  spec.dtype = argc >= 7 ? pick(argv[6], dtypes, 4) : RD_TENSOR_F16;
  spec.layout = argc >= 8 ? pick(argv[7], layouts, 2) : RD_TENSOR_NCHW;
  spec.channels = argc >= 9 ? pick(argv[8], kinds, 3) : RD_TENSOR_RGB;
  spec.oversample = argc >= 10 ? atoi(argv[9]) : 2;
  for (int c = 0; c < 3; c++) { spec.scale[c] = argc >= 11 ? (float)atof(argv[10]) : 1.0f / 255.0f; spec.bias[c] = argc >= 12 ? (float)atof(argv[11]) : 0.0f; }
  if (!rd_tensor_spec_ok(&spec, pw, ph)) { fprintf(stderr, "%s: not a legal tensor spec for %d x %d outputs\n", argv[0], pw, ph); return 1; }

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
    rd_rectifier *rf = rd_rectifier_create_tensor(did, pw, ph, n, 1, &spec);
    if (!rf) { fprintf(stderr, "rd_rectifier_create_tensor(%d, %d, %d, %d, 1): bad arguments\n", did, pw, ph, n); return 1; }
    double *quads = (double *)malloc(sizeof(double) * 8 * n);
    rd_rect_quads(ret + 1, n, quads);      /* c2[0], c2[3], c2[2], c2[1]: clockwise on screen, not mirrored */
    const size_t one = rd_rectifier_patch_bytes(rf);
    uint8_t *out = (uint8_t *)rd_host_alloc(one * n);      /* pinned: the copy engine writes the tensors here */
    uint8_t *status = (uint8_t *)malloc(n);
    const void *const planes[3] = { img.bgr, NULL, NULL };
    const int pitches[3] = { img.ws, 0, 0 };
    if (rd_rectifier_enqueue(rf, RD_PIX_BGR, planes, pitches, img.iw, img.ih, RD_FRAME_HOST, quads, n, out, RD_FRAME_HOST_PINNED) < 0) {
      fprintf(stderr, "rd_rectifier_enqueue: argument error\n");
      return 1;
    }
    rd_rectifier_wait(rf, status);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(out, one, n, f) != (size_t)n || fclose(f) != 0) { fprintf(stderr, "%s: cannot write %s\n", argv[0], path); return 1; }
    const int C = spec.channels == RD_TENSOR_GRAY ? 1 : 3;
    if (spec.layout == RD_TENSOR_NCHW) printf("shape %d x %d x %d x %d dtype %s bytes %zu -> %s\n", n, C, ph, pw, dtypes[spec.dtype], one * n, path);
    else printf("shape %d x %d x %d x %d dtype %s bytes %zu -> %s\n", n, ph, pw, C, dtypes[spec.dtype], one * n, path);
    for (int i = 0; i < n; i++)
      printf("status %u aspect %.4f tensor %d %s\n", ret[i + 1].status, rd_rect_aspect(&ret[i + 1]), i, status[i] ? "" : "(not a convex quad: zero bytes)");
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
