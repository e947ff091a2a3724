/* rdcodes - what do the detected rectangles SAY?  Makes a frame of its own: four square grid codes of a generated dictionary (rd_code_dictionary: 6 x 6 payloads,
 * 50 codes at distance >= 9), each rendered (rd_code_render) at another size and turned by another number of quarter turns, on light paper.  Then rdrect's call
 * sequence (the reference's C API, rect.cpp:47-138) finds the rectangles, and one job of a rectifier made with rd_rectifier_create_code (rectdetect_hip.h, "decoded
 * quads") reads them all: per rectangle the id, the rotation, the Hamming distance to the nearest and to the second nearest code, the ring's errors and the verdict,
 * and the corners from which the code stands upright (rd_code_upright).
 *
 *   rdcodes [device number] [frame.ppm to write] [patch side] [inset] [max_hamming]
 *
 * Defaults: device 0, no file, 64 x 64 patches, inset 2, max_hamming 2.  Doubles with %.17g, so that they can be compared bit for bit.  Links against
 * librectdetect_hip.so only. */
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

#define IW 640
#define IH 480
#define NDICT 50
#define PAPER 225

int main(int argc, char **argv) {
  const int did = argc >= 2 ? atoi(argv[1]) : 0;
  const char *ppm = argc >= 3 && strcmp(argv[2], "-") != 0 ? argv[2] : NULL;
  const int side = argc >= 4 ? atoi(argv[3]) : 64;
  rd_code_spec spec = { 6, 1, 2, 0, 1, 32, 0, 2 };
  if (argc >= 5) spec.inset = atoi(argv[4]);
  if (argc >= 6) spec.max_hamming = atoi(argv[5]);
  if (!rd_code_spec_ok(&spec, side, side)) { fprintf(stderr, "%s: not a legal code spec for patches of %d x %d\n", argv[0], side, side); return 1; }

  uint64_t dict[NDICT];
  const int ndict = rd_code_dictionary(spec.n, NDICT, 9, 1, 1 << 20, dict);
  if (ndict != NDICT) { fprintf(stderr, "rd_code_dictionary: %d of %d codes\n", ndict, NDICT); return 1; }
  printf("dictionary %d codes of %d x %d distance %d\n", ndict, spec.n, spec.n, rd_code_distance(dict, ndict, spec.n));

  /* the frame: BGR, four codes; code k is dictionary entry shown[k], its payload turned so that an upright reader sees it k quarter turns off */
  static const int shown[4] = { 3, 17, 29, 41 }, cell_px[4] = { 12, 16, 10, 14 }, at[4][2] = { { 60, 50 }, { 330, 40 }, { 90, 300 }, { 400, 270 } };
  const int ws = IW * 3;
  uint8_t *frame = (uint8_t *)malloc((size_t)ws * IH), *img = (uint8_t *)malloc(8 * 64 * 8 * 64);
  memset(frame, PAPER, (size_t)ws * IH);
  for (int k = 0; k < 4; k++) {
    const int S = (spec.n + 2 * spec.border) * cell_px[k];
    if (rd_code_render(&spec, rd_code_rotate(dict[shown[k]], spec.n, 4 - k), cell_px[k], img) != (size_t)S * S) { fprintf(stderr, "rd_code_render failed\n"); return 1; }
    for (int y = 0; y < S; y++)
      for (int x = 0; x < S; x++) memset(frame + (size_t)(at[k][1] + y) * ws + 3 * (at[k][0] + x), img[y * S + x] ? PAPER : 20, 3);
    printf("code %d : id %d shown %d quarter turn(s) off at %d %d side %d\n", k, shown[k], k, at[k][0], at[k][1], S);
  }
  free(img);
  if (ppm) {
    FILE *f = fopen(ppm, "wb");
    if (!f) { perror(ppm); return 1; }
    fprintf(f, "P6\n%d %d\n255\n", IW, IH);
    for (size_t p = 0; p < (size_t)IW * IH; p++) { const uint8_t rgb[3] = { frame[3 * p + 2], frame[3 * p + 1], frame[3 * p] }; fwrite(rgb, 1, 3, f); }
    fclose(f);
  }

  cl_device_id device = simpleGetDevice(did);
  printf("%s\n", getDeviceName(device));
  cl_context context = simpleCreateContext(device);
  cl_command_queue queue = clCreateCommandQueue(context, device, CL_QUEUE_PROFILING_ENABLE, NULL);
  struct oclimgutil_t *iu = init_oclimgutil(device, context);
  struct oclpolyline_t *pl = init_oclpolyline(device, context);
  struct oclrect_t *rc = init_oclrect(iu, pl, device, context, queue, IW, IH);

  const double tanAOV = tan(72.0 / 2 / 180.0 * M_PI);
  rect_t *ret = oclrect_executeOnce(rc, frame, ws, tanAOV);
  const int n = ret->nItems - 1;      /* element 0 is the header */
  printf("%d rectangle(s)\n", n);

  if (n > 0) {
    rd_rectifier *rf = rd_rectifier_create_code(did, side, side, n, 1, &spec, dict, ndict);
    if (!rf) { fprintf(stderr, "rd_rectifier_create_code(%d, %d, %d, %d, 1): bad arguments\n", did, side, side, n); return 1; }
    double *quads = (double *)malloc(sizeof(double) * 8 * n);
    rd_rect_quads(ret + 1, n, quads);      /* c2[0], c2[3], c2[2], c2[1]: clockwise on screen, not mirrored */
    rd_code *out = (rd_code *)rd_host_alloc(rd_rectifier_patch_bytes(rf) * (size_t)n);      /* pinned (and aligned): the copy engine writes the records here */
    uint8_t *status = (uint8_t *)calloc(n, 1);
    const void *const planes[3] = { frame, NULL, NULL };
    const int pitches[3] = { ws, 0, 0 };
    if (rd_rectifier_enqueue(rf, RD_PIX_BGR, planes, pitches, IW, IH, RD_FRAME_HOST, quads, n, out, RD_FRAME_HOST_PINNED) < 0) {
      fprintf(stderr, "rd_rectifier_enqueue: argument error\n");
      return 1;
    }
    rd_rectifier_wait(rf, status);
    for (int i = 0; i < n; i++) {
      const rd_code *c = &out[i];
      double up[8];
      rd_code_upright(quads + 8 * i, c->rot, up);
      printf("rect %d status %u : id %d rot %d hamming %d second %d border_errors %d lo %d hi %d margin %d ok %d bits %016llx%s\n", i, ret[i + 1].status, c->id, c->rot, c->hamming, c->second,
             c->border_errors, c->lo, c->hi, c->margin, c->ok, (unsigned long long)c->bits, status[i] ? "" : " (not a convex quad: zeros)");
      printf("  rect %d upright : %.17g %.17g  %.17g %.17g  %.17g %.17g  %.17g %.17g\n", i, up[0], up[1], up[2], up[3], up[4], up[5], up[6], up[7]);
    }
    free(status);
    rd_host_free(out);
    free(quads);
    rd_rectifier_destroy(rf);
  }
  free(ret);
  free(frame);

  dispose_oclrect(rc);
  dispose_oclpolyline(pl);
  dispose_oclimgutil(iu);
  ce(clReleaseCommandQueue(queue));
  ce(clReleaseContext(context));
  return 0;
}
