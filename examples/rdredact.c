/* rdredact - redaction that never leaves the device: a YUV4MPEG2 stream (8-bit 4:2:0) in, the same stream out with every detected rectangle filled with a colour
 * or, with "mosaic", replaced by a coarse version of itself: the rectangle is rectified into an 8 x 8 patch (rd_rectifier, rd_detector_rectify_polled) and the patch
 * pasted back into its quad (rd_compositor, rd_detector_composite_polled).  The frames stay I420 all the way: they are uploaded once by the detector, read and
 * written on the device from the copy the detector holds, and come back through pinned memory - what would go to a hardware encoder instead of a file.
 *
 *   rdredact <in.y4m | -> <out.y4m | -> [device number] [fill | mosaic] [angle of view in degrees]
 *
 * ffmpeg -i in.mp4 -pix_fmt yuv420p -f yuv4mpegpipe - | rdredact - - 0 mosaic | ffplay - */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rectdetect_hip.h"

/* the stream header "YUV4MPEG2 W<w> H<h> ... [C<colour space>]", kept in `copy` for the output: 0 on success */
static int read_header(FILE *f, int *iw, int *ih, char *copy, size_t len) {
  char line[1024];
  if (!fgets(line, sizeof(line), f) || strncmp(line, "YUV4MPEG2 ", 10) != 0) { fprintf(stderr, "rdredact: not a YUV4MPEG2 stream\n"); return 1; }
  snprintf(copy, len, "%s", line);
  *iw = *ih = 0;
  for (char *t = strtok(line + 10, " \n"); t; t = strtok(NULL, " \n")) {
    if (t[0] == 'W') *iw = atoi(t + 1);
    else if (t[0] == 'H') *ih = atoi(t + 1);
    else if (t[0] == 'C' && strcmp(t, "C420") != 0 && strcmp(t, "C420jpeg") != 0 && strcmp(t, "C420paldv") != 0 && strcmp(t, "C420mpeg2") != 0) {
      fprintf(stderr, "rdredact: colour space %s - only 8-bit 4:2:0 (C420, C420jpeg, C420paldv, C420mpeg2) is supported\n", t);
      return 1;
    }
  }
  if (*iw < 16 || *ih < 16 || (*iw & 1) || (*ih & 1)) { fprintf(stderr, "rdredact: frame size %dx%d (4:2:0 needs even sizes, the detector at least 16x16)\n", *iw, *ih); return 1; }
  return 0;
}

static int read_frame(FILE *f, uint8_t *buf, size_t bytes) {
  char line[1024];
  if (!fgets(line, sizeof(line), f)) return 0;
  if (strncmp(line, "FRAME", 5) != 0) { fprintf(stderr, "rdredact: frame marker expected\n"); return 0; }
  return fread(buf, 1, bytes, f) == bytes;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "Usage : %s <in.y4m | -> <out.y4m | -> [device] [fill | mosaic] [aov]\n", argv[0]); return 1; }
  FILE *f = strcmp(argv[1], "-") == 0 ? stdin : fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  FILE *o = strcmp(argv[2], "-") == 0 ? stdout : fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  const int did = argc >= 4 ? atoi(argv[3]) : 0;
  const int mosaic = argc >= 5 && strcmp(argv[4], "mosaic") == 0;
  const double aov = argc >= 6 ? atof(argv[5]) : 72.0;
  const double tanAOV = tan(aov / 2 / 180.0 * M_PI);
  int iw, ih;
  char header[1024];
  if (read_header(f, &iw, &ih, header, sizeof(header))) return 1;
  const size_t ny = (size_t)iw * ih, nc = ny / 4, bytes = ny + 2 * nc;
  enum { MAX_ITEMS = 1024, PW = 8, PH = 8 };

  rd_detector *d = rd_detector_create(did, iw, ih, 1, 0);
  rd_compositor *c = rd_compositor_create(did, PW, PH, MAX_ITEMS, 1);
  rd_rectifier *r = mosaic ? rd_rectifier_create(did, PW, PH, MAX_ITEMS, 1) : NULL;
  if (!d || !c || (mosaic && !r)) { fprintf(stderr, "rdredact: no detector, compositor or rectifier on device %d\n", did); return 1; }
  uint8_t *in = (uint8_t *)rd_host_alloc(bytes), *out = (uint8_t *)rd_host_alloc(bytes);      /* pinned: the copy engine reads and writes them in place */
  void *patches = mosaic ? rd_device_alloc((size_t)MAX_ITEMS * PW * PH * 3) : NULL;           /* the patches never leave the device */
  double *quads = (double *)malloc(MAX_ITEMS * 8 * sizeof(double));
  rd_comp_item *items = (rd_comp_item *)calloc(MAX_ITEMS, sizeof(rd_comp_item));
  const void *planes[3] = { in, in + ny, in + ny + nc };
  void *out_planes[3] = { out, out + ny, out + ny + nc };
  const int pitches[3] = { iw, iw / 2, iw / 2 };
  fputs(header, o);
  int frames = 0;
  long redacted = 0;
  while (read_frame(f, in, bytes)) {
    if (rd_detector_enqueue_planes(d, RD_PIX_I420, planes, pitches, RD_FRAME_HOST_PINNED) < 0) { fprintf(stderr, "rdredact: frame refused\n"); return 1; }
    void *ret = rd_detector_poll(d, tanAOV);
    int n = *(int *)ret - 1;      /* (element 0 holds nItems, as rect_t of oclrect.h) */
    if (n > MAX_ITEMS) n = MAX_ITEMS;
    rd_rect_quads((const char *)ret + 176, n, quads);
    free(ret);
    for (int k = 0; k < n; k++) {
      memcpy(items[k].quad, quads + 8 * k, 8 * sizeof(double));
      items[k].patch = mosaic ? k : -1;
      items[k].b = items[k].g = items[k].r = 0;      /* fill: black */
    }
    if (mosaic && n > 0) {
      if (rd_detector_rectify_polled(d, r, quads, n, patches, RD_FRAME_DEVICE) < 0) { fprintf(stderr, "rdredact: rectifier job refused\n"); return 1; }
      rd_rectifier_wait(r, NULL);      /* (the compositor has a stream of its own: the patches must be there before its job starts) */
    }
    if (rd_detector_composite_polled(d, c, items, n, patches, mosaic ? n : 0, RD_FRAME_DEVICE, out_planes, pitches, RD_FRAME_HOST_PINNED) < 0) { fprintf(stderr, "rdredact: job refused\n"); return 1; }
    rd_compositor_wait(c, NULL);
    fputs("FRAME\n", o);
    if (fwrite(out, 1, bytes, o) != bytes) { perror("rdredact: write"); return 1; }
    frames++;
    redacted += n;
  }
  fprintf(stderr, "rdredact: %d frame(s), %ld rectangle(s) %s\n", frames, redacted, mosaic ? "replaced by their mosaic" : "filled");
  rd_compositor_destroy(c);
  if (r) rd_rectifier_destroy(r);
  rd_detector_destroy(d);
  if (patches) rd_device_free(patches);
  rd_host_free(in);
  rd_host_free(out);
  free(quads);
  free(items);
  if (o != stdout) fclose(o);
  if (f != stdin) fclose(f);
  return 0;
}
