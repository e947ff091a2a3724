/* rdvidpoly - the loop of the reference's vidpoly.cpp:160-200 (line segments of every frame of a stream) without OpenCV, through the polyline
 * kind of rd_detector: several frames in flight instead of one operator sequence per frame.  Frames come from the synthetic stream generator of
 * this library (rd_synth_frame).
 *
 *   rdvidpoly <device> <width>x<height> <frames> [frames in flight] [strength threshold] [minerror] [size threshold]
 *
 * Defaults are vidpoly.cpp's parameters (2000, 1, 10) and 8 frames in flight.  Prints, per frame, the number of records, the number of valid
 * ones (polyid != 0) and the CRC32 of the valid records, then the frame rate. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "helper.h"
#include "rectdetect_hip.h"

typedef struct { float x0, y0, x1, y1; int startIndex, endIndex, leftPtr, rightPtr, startCount, endCount, maxDist, polyid, npix, level; } segment_t;   /* linesegment_t */

static void report(int k, const segment_t *ls) {
  const int n = *(const int *)ls;
  int valid = 0;
  uLong crc = crc32(0L, Z_NULL, 0);
  for (int i = 1; i <= n; i++)      /* >>>> this starts from 1 <<<< (vidpoly.cpp:196) */
    if (ls[i].polyid != 0) { valid++; crc = crc32(crc, (const Bytef *)&ls[i], sizeof(segment_t)); }
  printf("frame %d: records %d valid %d crc %08lx\n", k, n, valid, (unsigned long)crc);
}

int main(int argc, char **argv) {
  int iw = 0, ih = 0;
  if (argc < 4 || sscanf(argv[2], "%dx%d", &iw, &ih) != 2) {
    fprintf(stderr, "Usage : %s <device> <width>x<height> <frames> [frames in flight] [strength threshold] [minerror] [size threshold]\n", argv[0]);
    return 1;
  }
  const int did = atoi(argv[1]), nframes = atoi(argv[3]);
  const int nslots = argc >= 5 ? atoi(argv[4]) : 8;
  const int sthr = argc >= 6 ? atoi(argv[5]) : 2000;
  const float minerror = argc >= 7 ? (float)atof(argv[6]) : 1.0f;
  const int sizethr = argc >= 8 ? atoi(argv[7]) : 10;
  rd_detector *d = rd_polyline_detector_create(did, iw, ih, nslots, sthr, minerror, sizethr);
  if (!d) { fprintf(stderr, "%s: invalid arguments\n", argv[0]); return 1; }
  const int ws = iw * 3;
  uint8_t *bgr = (uint8_t *)malloc((size_t)ws * ih);      /* host frames are copied by the enqueue: one buffer will do */
  const uint64_t t0 = currentTimeMillis();
  int polled = 0;
  for (int n = 0; n < nframes; n++) {
    if (n - polled == nslots) { segment_t *ls = (segment_t *)rd_detector_poll_segments(d, NULL); report(polled++, ls); free(ls); }
    rd_synth_frame(bgr, iw, ih, ws, 0x5EED0000ull, n, 1);
    rd_detector_enqueue(d, bgr, ws, RD_FRAME_HOST);
  }
  while (polled < nframes) { segment_t *ls = (segment_t *)rd_detector_poll_segments(d, NULL); report(polled++, ls); free(ls); }
  const uint64_t t1 = currentTimeMillis();
  printf("%d frames, %.1f frames/s (synthetic frames generated on the host included)\n", nframes, t1 > t0 ? 1000.0 * nframes / (double)(t1 - t0) : 0.0);
  rd_detector_destroy(d);
  free(bgr);
  return 0;
}
