/* rdy4m - the rectangle detector over a YUV4MPEG2 file (4:2:0 only), through rd_detector_enqueue_planes with RD_PIX_I420 host frames and several frames
 * in flight: a real video without OpenCV (ffmpeg -i in.mp4 -pix_fmt yuv420p -f yuv4mpegpipe out.y4m; "-" reads standard input).  8-bit samples only: C420,
 * C420jpeg, C420paldv, C420mpeg2 or no C tag; C420p10 / C420p12 and the other chroma layouts are refused.
 *
 *   rdy4m <file.y4m | -> [device number] [angle of view in degrees] [frames in flight] [half]
 *
 * half: detect at half the stream's size (rd_detector_enqueue_scaled, scale 2: the detector is W/2 x H/2 and averages 2x2 as it reads the full-size planes) -
 * a 3840x2160 stream at the rate of a 1920x1080 one.
 *
 * Prints the number of rectangles per frame, in the shape of rdvid, and the frame rate once per second. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include "rectdetect_hip.h"

static double now_ms(void) { struct timeval tv; gettimeofday(&tv, NULL); return tv.tv_sec * 1000.0 + tv.tv_usec / 1000.0; }

/* the stream header "YUV4MPEG2 W<w> H<h> ... [C<colour space>]": 0 on success */
static int read_header(FILE *f, int *iw, int *ih) {
  char line[1024];
  if (!fgets(line, sizeof(line), f) || strncmp(line, "YUV4MPEG2 ", 10) != 0) { fprintf(stderr, "rdy4m: not a YUV4MPEG2 stream\n"); return 1; }
  *iw = *ih = 0;
  for (char *t = strtok(line + 10, " \n"); t; t = strtok(NULL, " \n")) {
    if (t[0] == 'W') *iw = atoi(t + 1);
    else if (t[0] == 'H') *ih = atoi(t + 1);
    else if (t[0] == 'C' && strcmp(t, "C420") != 0 && strcmp(t, "C420jpeg") != 0 && strcmp(t, "C420paldv") != 0 && strcmp(t, "C420mpeg2") != 0) {
      fprintf(stderr, "rdy4m: colour space %s - only 8-bit 4:2:0 (C420, C420jpeg, C420paldv, C420mpeg2) is supported%s\n", t,
              strncmp(t, "C420p", 5) == 0 ? " (this stream has more than 8 bits per sample: ffmpeg ... -pix_fmt yuv420p -f yuv4mpegpipe)" : "");
      return 1;
    }
  }
  if (*iw <= 0 || *ih <= 0 || (*iw & 1) || (*ih & 1)) { fprintf(stderr, "rdy4m: frame size %dx%d (4:2:0 needs even sizes)\n", *iw, *ih); return 1; }
  return 0;
}

/* one frame: the "FRAME[ params]" line, then Y, U and V: 1 on success, 0 at the end of the stream */
static int read_frame(FILE *f, uint8_t *buf, size_t bytes) {
  char line[1024];
  if (!fgets(line, sizeof(line), f)) return 0;
  if (strncmp(line, "FRAME", 5) != 0) { fprintf(stderr, "rdy4m: frame marker expected\n"); return 0; }
  return fread(buf, 1, bytes, f) == bytes;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "Usage : %s <file.y4m | -> [device] [aov] [frames in flight] [half]\n", argv[0]); return 1; }
  FILE *f = strcmp(argv[1], "-") == 0 ? stdin : fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  const int did = argc >= 3 ? atoi(argv[2]) : 0;
  const double aov = argc >= 4 ? atof(argv[3]) : 72.0;
  const int nslots = argc >= 5 ? atoi(argv[4]) : 4;
  const int scale = argc >= 6 && strcmp(argv[5], "half") == 0 ? 2 : 1;
  if (argc >= 6 && scale == 1) { fprintf(stderr, "rdy4m: unknown option %s\n", argv[5]); return 1; }
  const double tanAOV = tan(aov / 2 / 180.0 * M_PI);
  int iw, ih;
  if (read_header(f, &iw, &ih)) return 1;
  const size_t ny = (size_t)iw * ih, nc = ny / 4;

  rd_detector *d = rd_detector_create(did, iw / scale, ih / scale, nslots, 0);
  uint8_t *buf = (uint8_t *)malloc(ny + 2 * nc);      /* host frames are copied before the call returns: one buffer will do */
  double tm = now_ms();
  int pending = 0, polled = 0, last = 0, n = 0;
  for (int more = 1;;) {
    if (more && pending < nslots && (more = read_frame(f, buf, ny + 2 * nc))) {
      const void *planes[3] = { buf, buf + ny, buf + ny + nc };
      const int pitches[3] = { iw, iw / 2, iw / 2 };
      if (rd_detector_enqueue_scaled(d, RD_PIX_I420, planes, pitches, scale, RD_FRAME_HOST) < 0) { fprintf(stderr, "rdy4m: frame refused\n"); return 1; }
      pending++; n++;
      continue;
    }
    if (!pending) break;
    void *ret = rd_detector_poll(d, tanAOV);
    printf("frame %d: %d rectangle(s)\n", polled++, *(int *)ret - 1);      /* (element 0 holds nItems, as rect_t of oclrect.h) */
    free(ret);
    pending--;
    const double t = now_ms();
    if (t - tm > 1000) { printf("%.3g fps\n", 1000.0 * (n - last) / (t - tm)); tm = t; last = n; }
  }
  rd_detector_destroy(d);
  free(buf);
  if (f != stdin) fclose(f);
  return 0;
}
