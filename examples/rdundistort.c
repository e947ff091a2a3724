/* rdundistort - rectangles in the picture of a real lens: the frame is remapped on the device to what an ideal pinhole camera would have seen
 * (rectdetect_hip.h, "remapped frames": rd_remapper_*), the detector runs on the remapped frame where it lies in device memory, and the rectangles come back in
 * the undistorted frame's coordinates - with rd_remap_points, in the original's as well.
 *
 *   rdundistort <image.ppm|png> <fx> <fy> <cx> <cy> <k1> <k2> <p1> <p2> <k3> [output.ppm] [device number]
 *
 * The nine numbers are the camera matrix and the Brown-Conrady coefficients of a calibration (OpenCV's order).  The view - the ideal camera of the output - takes
 * the lens's fx, fy, cx, cy, and the output has the size of the input.  Prints one line per rectangle: its status and its four corners in the undistorted frame
 * and in the original one; writes the undistorted frame (default "undistorted.ppm").  Links against librectdetect_hip.so only. */
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
  if (argc < 11) {
    fprintf(stderr, "Usage : %s <image file name (.ppm or .png)> <fx> <fy> <cx> <cy> <k1> <k2> <p1> <p2> <k3> [output.ppm] [device number]\n", argv[0]);
    return 1;
  }
  rd_lens lens;
  double *field = &lens.fx;
  for (int k = 0; k < 9; k++) field[k] = atof(argv[2 + k]);
  const rd_view view = { lens.fx, lens.fy, lens.cx, lens.cy };
  const char *outname = argc >= 12 ? argv[11] : "undistorted.ppm";
  const int did = argc >= 13 ? atoi(argv[12]) : 0;
  if (rd_device_count() <= did) { fprintf(stderr, "no HIP device %d\n", did); return 1; }

  rdimage img;
  if (rdimage_load(argv[1], &img) != 0) return 1;
  const int iw = img.iw, ih = img.ih, pitch = (iw * 3 + 3) & ~3;

  rd_remapper *rm = rd_remapper_create_lens(did, &lens, &view, iw, ih, iw, ih, 1);
  if (!rm) { fprintf(stderr, "rd_remapper_create_lens: bad arguments (a lens field that is not finite, fx or fy of 0, an image larger than 16384 a side)\n"); return 1; }
  printf("%d of %d pixels of the undistorted frame lie inside the original\n", rd_remapper_inside(rm), iw * ih);

  /* the remapped frame stays on the device: the detector reads it there */
  rd_select_device(did);
  uint8_t *d_frame = (uint8_t *)rd_device_alloc((size_t)pitch * ih);
  const void *const planes[3] = { img.bgr, NULL, NULL };
  const int pitches[3] = { img.ws, 0, 0 };
  if (rd_remapper_enqueue(rm, RD_PIX_BGR, planes, pitches, RD_FRAME_HOST, 0, d_frame, pitch, RD_FRAME_DEVICE) < 0) { fprintf(stderr, "rd_remapper_enqueue: argument error\n"); return 1; }
  rd_remapper_wait(rm);

  rd_detector *det = rd_detector_create(did, iw, ih, 1, 0);
  rd_detector_enqueue(det, d_frame, pitch, RD_FRAME_DEVICE);
  rect_t *ret = (rect_t *)rd_detector_poll(det, rd_view_tan_aov(&view, iw));      /* (d_frame stays until this returned) */
  const int n = ret->nItems - 1;      /* element 0 is the header */
  printf("%d rectangle(s)\n", n);
  for (int i = 1; i <= n; i++) {
    double uv[8], XY[8];
    memcpy(uv, ret[i].c2, sizeof(uv));
    rd_remap_points(&lens, &view, uv, 4, XY);
    printf("status %u undistorted", ret[i].status);
    for (int k = 0; k < 4; k++) printf(" (%.2f, %.2f)", uv[2 * k], uv[2 * k + 1]);
    printf(" original");
    for (int k = 0; k < 4; k++) printf(" (%.2f, %.2f)", XY[2 * k], XY[2 * k + 1]);
    printf("\n");
  }
  free(ret);

  rdimage und = { iw, ih, pitch, (uint8_t *)malloc((size_t)pitch * ih) };
  rd_download(und.bgr, d_frame, (size_t)pitch * ih);
  const int bad = rdimage_save_ppm(outname, &und);
  if (!bad) printf("wrote %s\n", outname);
  free(und.bgr);

  rd_detector_destroy(det);
  rd_remapper_destroy(rm);
  rd_device_free(d_frame);
  rdimage_free(&img);
  return bad;
}
