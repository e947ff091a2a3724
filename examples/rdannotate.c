/* rdannotate - vidrect's / vidpoly's picture without OpenCV and without host drawing: a YUV4MPEG2 stream (8-bit 4:2:0) in, the same stream out with every detected
 * rectangle's edges and diagonals drawn into the frame (vidrect.cpp: showRect) or, with "poly", every line segment in white on black (vidpoly.cpp).  The frames stay
 * I420 all the way: they are uploaded once by the detector, drawn on the device (rd_annotator, rd_detector_annotate_polled) from the copy the detector holds, and
 * come back through pinned memory - what would go to a hardware encoder instead of a file.
 *
 *   rdannotate <in.y4m | -> <out.y4m | -> [device number] [poly] [angle of view in degrees]
 *
 * ffmpeg -i in.mp4 -pix_fmt yuv420p -f yuv4mpegpipe - | rdannotate - - | ffplay - */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rectdetect_hip.h"

/* the stream header "YUV4MPEG2 W<w> H<h> ... [C<colour space>]", kept in `copy` for the output: 0 on success */
static int read_header(FILE *f, int *iw, int *ih, char *copy, size_t len) {
  char line[1024];
  if (!fgets(line, sizeof(line), f) || strncmp(line, "YUV4MPEG2 ", 10) != 0) { fprintf(stderr, "rdannotate: not a YUV4MPEG2 stream\n"); return 1; }
  snprintf(copy, len, "%s", line);
  *iw = *ih = 0;
  for (char *t = strtok(line + 10, " \n"); t; t = strtok(NULL, " \n")) {
    if (t[0] == 'W') *iw = atoi(t + 1);
    else if (t[0] == 'H') *ih = atoi(t + 1);
    else if (t[0] == 'C' && strcmp(t, "C420") != 0 && strcmp(t, "C420jpeg") != 0 && strcmp(t, "C420paldv") != 0 && strcmp(t, "C420mpeg2") != 0) {
      fprintf(stderr, "rdannotate: colour space %s - only 8-bit 4:2:0 (C420, C420jpeg, C420paldv, C420mpeg2) is supported\n", t);
      return 1;
    }
  }
  if (*iw < 16 || *ih < 16 || (*iw & 1) || (*ih & 1)) { fprintf(stderr, "rdannotate: frame size %dx%d (4:2:0 needs even sizes, the detector at least 16x16)\n", *iw, *ih); return 1; }
  return 0;
}

static int read_frame(FILE *f, uint8_t *buf, size_t bytes) {
  char line[1024];
  if (!fgets(line, sizeof(line), f)) return 0;
  if (strncmp(line, "FRAME", 5) != 0) { fprintf(stderr, "rdannotate: frame marker expected\n"); return 0; }
  return fread(buf, 1, bytes, f) == bytes;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "Usage : %s <in.y4m | -> <out.y4m | -> [device] [poly] [aov]\n", argv[0]); return 1; }
  FILE *f = strcmp(argv[1], "-") == 0 ? stdin : fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  FILE *o = strcmp(argv[2], "-") == 0 ? stdout : fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  const int did = argc >= 4 ? atoi(argv[3]) : 0;
  const int poly = argc >= 5 && strcmp(argv[4], "poly") == 0;
  const double aov = argc >= 6 ? atof(argv[5]) : 72.0;
  const double tanAOV = tan(aov / 2 / 180.0 * M_PI);
  int iw, ih;
  char header[1024];
  if (read_header(f, &iw, &ih, header, sizeof(header))) return 1;
  const size_t ny = (size_t)iw * ih, nc = ny / 4, bytes = ny + 2 * nc;
  enum { MAX_PRIMS = 16384 };

  rd_detector *d = poly ? rd_polyline_detector_create(did, iw, ih, 1, 2000, 1.0f, 10) : rd_detector_create(did, iw, ih, 1, 0);      /* (vidpoly.cpp's parameters) */
  rd_annotator *a = rd_annotator_create(did, MAX_PRIMS, 1);
  if (!d || !a) { fprintf(stderr, "rdannotate: no detector or annotator on device %d\n", did); return 1; }
  uint8_t *in = (uint8_t *)rd_host_alloc(bytes), *out = (uint8_t *)rd_host_alloc(bytes);      /* pinned: the copy engine reads and writes them in place */
  rd_annot_prim *prims = (rd_annot_prim *)malloc(MAX_PRIMS * sizeof(rd_annot_prim));
  const void *planes[3] = { in, in + ny, in + ny + nc };
  void *out_planes[3] = { out, out + ny, out + ny + nc };
  const int pitches[3] = { iw, iw / 2, iw / 2 };
  fputs(header, o);
  int frames = 0;
  long drawn = 0;
  while (read_frame(f, in, bytes)) {
    if (rd_detector_enqueue_planes(d, RD_PIX_I420, planes, pitches, RD_FRAME_HOST_PINNED) < 0) { fprintf(stderr, "rdannotate: frame refused\n"); return 1; }
    int n;
    if (poly) {
      void *ls = rd_detector_poll_segments(d, NULL);
      n = rd_annot_segments(ls, RD_ANNOT_SEG_ALL, 1, prims, MAX_PRIMS);
      free(ls);
    } else {
      void *ret = rd_detector_poll(d, tanAOV);
      int nr = *(int *)ret - 1;      /* (element 0 holds nItems, as rect_t of oclrect.h) */
      if (nr > MAX_PRIMS / 6) nr = MAX_PRIMS / 6;
      n = rd_annot_rects((const char *)ret + 176, nr, 1, NULL, prims);
      free(ret);
    }
    if (n > MAX_PRIMS) n = MAX_PRIMS;
    if (rd_detector_annotate_polled(d, a, prims, n, poly ? RD_ANNOT_CLEAR : 0, out_planes, pitches, RD_FRAME_HOST_PINNED) < 0) { fprintf(stderr, "rdannotate: job refused\n"); return 1; }
    rd_annotator_wait(a);
    fputs("FRAME\n", o);
    if (fwrite(out, 1, bytes, o) != bytes) { perror("rdannotate: write"); return 1; }
    frames++;
    drawn += n;
  }
  fprintf(stderr, "rdannotate: %d frame(s), %ld primitive(s) drawn\n", frames, drawn);
  rd_annotator_destroy(a);
  rd_detector_destroy(d);
  rd_host_free(in);
  rd_host_free(out);
  free(prims);
  if (o != stdout) fclose(o);
  if (f != stdin) fclose(f);
  return 0;
}
