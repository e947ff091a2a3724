// rectdetect-mi355x: the matcher - which template is inside each quad, behind the detector's poll (the contract: include/rectdetect_hip.h, "matched quads";
// the kernels: rd_k_match.hip; the score on the host: rd_match_host.c; the jobs in flight, the frame's checks and its way to the device: rd_jobs.h).
#include "rd_jobs.h"
#include "rd_kernels.h"
#include <stdio.h>

using namespace rdjob;

struct rd_matcher {
  Ring ring;                                // (first: rd_jobs.h)
  int G, m, D, max_templates, T;
  int rows, cols;                           // max_quads and 4 * max_templates, rounded up to the 16 x 16 tile of the dot kernel
  rdk::RectifyQuad *d_quads, *h_quads;      // njobs blocks of max_quads each (+ one record behind them for a template's quad), a job's at slot * max_quads
  int8_t *d_sig;                            // rows x D: the signatures of the job on the stream (jobs follow one another there); padding rows stay zero
  int *d_sums;                              // sa, saa per quad of the job on the stream
  int8_t *d_lib;                            // cols x D: column c at c * D; padding columns stay zero
  int *d_colsums, *h_colsums;               // sb, sbb per column: for the pick kernel, and for the scores on the host
  int *d_dots;                              // rows x cols
  rd_match *d_recs, *h_recs;                // max_quads records of the job on the stream; njobs pinned blocks of max_quads each
  int **h_dots;                             // per slot: a pinned block of max_quads x 4 * max_templates, allocated with the first RD_MATCH_DOTS job of the slot
  int *job_T, *job_flags;                   // per slot: the library's size at enqueue, the job's flags
  int8_t *d_tsig; int *d_tsums, *h_tsums;   // a template on its way into the library: its signature and sums
  DevBuf frame;                             // host and pinned frames travel through here
};

static bool pow2_in(int v, int mask) { return v > 0 && (v & (v - 1)) == 0 && (v & mask) == v; }

extern "C" {

rd_matcher *rd_matcher_create(int device, int grid, int oversample, int max_templates, int max_quads, int njobs) {
  int32_t lim[4];
  rd_match_limits(lim);
  if (!pow2_in(grid, lim[0]) || !pow2_in(oversample, lim[1]) || max_templates < 1 || max_templates > lim[2] || max_quads < 1 || max_quads > lim[3] || !ring_args_ok(device, njobs)) return NULL;
  rd_matcher *m = (rd_matcher *)calloc(1, sizeof(*m));
  ring_create(&m->ring, RD_MAGIC_MATCHER, device, max_quads, njobs);
  m->G = grid; m->m = oversample; m->D = grid * grid; m->max_templates = max_templates;
  m->rows = (max_quads + 15) & ~15; m->cols = (4 * max_templates + 15) & ~15;
  const size_t nq = (size_t)njobs * max_quads + 1;
  RD_HIP(hipMalloc((void **)&m->d_quads, nq * sizeof(rdk::RectifyQuad)));
  RD_HIP(hipHostMalloc((void **)&m->h_quads, nq * sizeof(rdk::RectifyQuad), hipHostMallocDefault));
  RD_HIP(hipMalloc((void **)&m->d_sig, (size_t)m->rows * m->D));
  RD_HIP(hipMalloc((void **)&m->d_sums, (size_t)max_quads * 2 * sizeof(int)));
  RD_HIP(hipMalloc((void **)&m->d_lib, (size_t)m->cols * m->D));
  RD_HIP(hipMalloc((void **)&m->d_colsums, (size_t)m->cols * 2 * sizeof(int)));
  RD_HIP(hipMalloc((void **)&m->d_dots, (size_t)m->rows * m->cols * sizeof(int)));
  RD_HIP(hipMalloc((void **)&m->d_recs, (size_t)max_quads * sizeof(rd_match)));
  RD_HIP(hipMalloc((void **)&m->d_tsig, (size_t)m->D));
  RD_HIP(hipMalloc((void **)&m->d_tsums, 2 * sizeof(int)));
  RD_HIP(hipHostMalloc((void **)&m->h_tsums, 2 * sizeof(int), hipHostMallocDefault));
  RD_HIP(hipHostMalloc((void **)&m->h_recs, (size_t)njobs * max_quads * sizeof(rd_match), hipHostMallocDefault));
  m->h_colsums = (int *)calloc((size_t)m->cols * 2, sizeof(int));
  m->h_dots = (int **)calloc(njobs, sizeof(int *));
  m->job_T = (int *)calloc(njobs, sizeof(int));
  m->job_flags = (int *)calloc(njobs, sizeof(int));
  // the padding rows and columns are computed on: they hold zeros from here on
  RD_HIP(hipMemsetAsync(m->d_sig, 0, (size_t)m->rows * m->D, m->ring.st));
  RD_HIP(hipMemsetAsync(m->d_lib, 0, (size_t)m->cols * m->D, m->ring.st));
  RD_HIP(hipMemsetAsync(m->d_colsums, 0, (size_t)m->cols * 2 * sizeof(int), m->ring.st));
  RD_HIP(hipStreamSynchronize(m->ring.st));
  return m;
}

void rd_matcher_destroy(rd_matcher *m) {
  if (!m) return;
  Ring *g = ring_of(m, RD_MAGIC_MATCHER, "rd_matcher_destroy");
  const int njobs = g->njobs;
  ring_destroy(g);
  for (int k = 0; k < njobs; k++) if (m->h_dots[k]) RD_HIP(hipHostFree(m->h_dots[k]));
  RD_HIP(hipFree(m->d_quads)); RD_HIP(hipHostFree(m->h_quads));
  RD_HIP(hipFree(m->d_sig)); RD_HIP(hipFree(m->d_sums)); RD_HIP(hipFree(m->d_lib)); RD_HIP(hipFree(m->d_colsums)); RD_HIP(hipFree(m->d_dots)); RD_HIP(hipFree(m->d_recs));
  RD_HIP(hipFree(m->d_tsig)); RD_HIP(hipFree(m->d_tsums)); RD_HIP(hipHostFree(m->h_tsums)); RD_HIP(hipHostFree(m->h_recs));
  m->frame.release();
  free(m->h_colsums); free(m->h_dots); free(m->job_T); free(m->job_flags);
  free(m);
}

int rd_matcher_templates(rd_matcher *m) {
  ring_of(m, RD_MAGIC_MATCHER, "rd_matcher_templates");
  return m->T;
}

// the frame where the kernels read it: a device frame in place, any other through the matcher's own buffer
static PixFrame frame_on_device(rd_matcher *m, const char *who, const PixLayout &L, const void *const planes[3], const int pitches[3], int on_device) {
  if (on_device == RD_FRAME_DEVICE) return planes_at(planes, pitches, L);
  m->frame.grow(m->ring.st, L.bytes);
  const PixFrame src = m->frame.packed(L);
  bring(m->ring.st, who, L, src, planes, pitches, on_device);
  return src;
}

int rd_matcher_add(rd_matcher *m, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device, const double *quad) {
  static const char who[] = "rd_matcher_add";
  Ring *g = ring_of(m, RD_MAGIC_MATCHER, who);
  PixLayout L;
  if (!frame_ok(format, planes, pitches, iw, ih, on_device, &L) || m->T >= m->max_templates) return -1;
  const double whole[8] = { -0.5, -0.5, (double)iw - 0.5, -0.5, (double)iw - 0.5, (double)ih - 0.5, -0.5, (double)ih - 0.5 };
  const size_t at = (size_t)g->njobs * g->per_job;      // the record behind the jobs' blocks
  rdk::RectifyQuad *q = &m->h_quads[at];
  q->pad = 0;
  rd_rectify_coefficients(quad ? quad : whole, q->c, &q->status);
  if (!q->status) return -2;
  RD_HIP(hipSetDevice(g->device));
  RD_HIP(hipStreamSynchronize(g->st));      // jobs in flight were scored against the library as it was
  const PixFrame src = frame_on_device(m, who, L, planes, pitches, on_device);
  RD_HIP(hipMemcpyAsync(&m->d_quads[at], q, sizeof(*q), hipMemcpyHostToDevice, g->st));
  RD_HIP(hipMemsetAsync(m->d_tsums, 0, 2 * sizeof(int), g->st));
  rdk::match_signatures(g->st, m->d_tsig, m->d_tsums, format, src, &m->d_quads[at], 1, m->G, m->m);
  rdrt::check_launch("matched quads: a template's signature");
  RD_HIP(hipMemcpyAsync(m->h_tsums, m->d_tsums, 2 * sizeof(int), hipMemcpyDeviceToHost, g->st));
  RD_HIP(hipStreamSynchronize(g->st));
  const long long sb = m->h_tsums[0], sbb = m->h_tsums[1];
  if ((long long)m->D * sbb - sb * sb == 0) return -2;      // flat
  const int k = m->T;
  rdk::match_rotations(g->st, m->d_lib + (size_t)4 * k * m->D, m->d_tsig, m->G);
  rdrt::check_launch("matched quads: a template's rotations");
  for (int r = 0; r < 4; r++) { m->h_colsums[2 * (4 * k + r)] = (int)sb; m->h_colsums[2 * (4 * k + r) + 1] = (int)sbb; }
  RD_HIP(hipMemcpyAsync(m->d_colsums + 8 * (size_t)k, m->h_colsums + 8 * (size_t)k, 8 * sizeof(int), hipMemcpyHostToDevice, g->st));
  RD_HIP(hipStreamSynchronize(g->st));
  m->T = k + 1;
  return k;
}

int rd_matcher_signature(rd_matcher *m, int tmpl, int rot, int8_t *out, int32_t sums[2]) {
  Ring *g = ring_of(m, RD_MAGIC_MATCHER, "rd_matcher_signature");
  if (tmpl < 0 || tmpl >= m->T || rot < 0 || rot > 3) return -1;
  const int c = 4 * tmpl + rot;
  if (out) {
    RD_HIP(hipSetDevice(g->device));
    RD_HIP(hipMemcpyAsync(out, m->d_lib + (size_t)c * m->D, (size_t)m->D, hipMemcpyDeviceToHost, g->st));
    RD_HIP(hipStreamSynchronize(g->st));
  }
  if (sums) { sums[0] = m->h_colsums[2 * c]; sums[1] = m->h_colsums[2 * c + 1]; }
  return 0;
}

long rd_matcher_enqueue(rd_matcher *m, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device, const double *quads, int n, int flags) {
  static const char who[] = "rd_matcher_enqueue";
  Ring *g = ring_of(m, RD_MAGIC_MATCHER, who);
  // argument errors: -1, nothing enqueued
  PixLayout L;
  if (!frame_ok(format, planes, pitches, iw, ih, on_device, &L)) return -1;
  if ((flags & ~RD_MATCH_DOTS) || n < 0 || n > g->per_job || (n > 0 && !quads)) return -1;
  RD_HIP(hipSetDevice(g->device));
  const int slot = ring_claim(g, who, n);
  const int T = m->T, ncols = 4 * T;
  m->job_T[slot] = T; m->job_flags[slot] = flags;
  rdk::RectifyQuad *h_quads = m->h_quads + (size_t)slot * g->per_job, *d_quads = m->d_quads + (size_t)slot * g->per_job;
  for (int k = 0; k < n; k++) {
    rdk::RectifyQuad *q = &h_quads[k];
    q->pad = 0;
    rd_rectify_coefficients(quads + 8 * (size_t)k, q->c, &q->status);
  }
  if (n > 0) {      // (an empty job touches no frame)
    const PixFrame src = frame_on_device(m, who, L, planes, pitches, on_device);
    RD_HIP(hipMemcpyAsync(d_quads, h_quads, (size_t)n * sizeof(rdk::RectifyQuad), hipMemcpyHostToDevice, g->st));
    RD_HIP(hipMemsetAsync(m->d_sums, 0, (size_t)n * 2 * sizeof(int), g->st));
    rdk::match_signatures(g->st, m->d_sig, m->d_sums, format, src, d_quads, n, m->G, m->m);
    rdrt::check_launch("matched quads: signatures");
    rdk::match_dots(g->st, m->d_dots, m->cols, m->d_sig, n, m->d_lib, ncols, m->D);
    rdrt::check_launch("matched quads: dots");
    rdk::match_pick(g->st, m->d_recs, m->d_dots, m->cols, m->d_colsums, ncols, m->d_sums, d_quads, n, m->D);
    rdrt::check_launch("matched quads: records");
    RD_HIP(hipMemcpyAsync(m->h_recs + (size_t)slot * g->per_job, m->d_recs, (size_t)n * sizeof(rd_match), hipMemcpyDeviceToHost, g->st));
    if ((flags & RD_MATCH_DOTS) && ncols > 0) {
      if (!m->h_dots[slot]) RD_HIP(hipHostMalloc((void **)&m->h_dots[slot], (size_t)g->per_job * 4 * m->max_templates * sizeof(int), hipHostMallocDefault));      // (on first use)
      RD_HIP(hipMemcpy2DAsync(m->h_dots[slot], (size_t)ncols * sizeof(int), m->d_dots, (size_t)m->cols * sizeof(int), (size_t)ncols * sizeof(int), n, hipMemcpyDeviceToHost, g->st));
    }
  }
  return ring_record(g);
}

int rd_matcher_wait(rd_matcher *m, rd_match *out, int32_t *dots_out) {
  Ring *g = ring_of(m, RD_MAGIC_MATCHER, "rd_matcher_wait");
  const int slot = ring_wait(g);
  if (slot < 0) return -1;
  const int n = g->n[slot], ncols = 4 * m->job_T[slot];
  const rd_match *recs = m->h_recs + (size_t)slot * g->per_job;
  if (out)
    for (int k = 0; k < n; k++) {
      out[k] = recs[k];
      const int c = 4 * recs[k].tmpl + recs[k].rot, c2 = recs[k].tmpl2 >= 0 ? 4 * recs[k].tmpl2 + recs[k].rot2 : 0;      // (a record with status 1 names columns of the job's library)
      if (recs[k].status == 1) rd_match_score(&out[k], m->G, m->h_colsums[2 * c], m->h_colsums[2 * c + 1], m->h_colsums[2 * c2], m->h_colsums[2 * c2 + 1]);
      else rd_match_score(&out[k], m->G, 0, 0, 0, 0);
    }
  if (dots_out && (m->job_flags[slot] & RD_MATCH_DOTS) && ncols > 0 && n > 0) memcpy(dots_out, m->h_dots[slot], (size_t)n * ncols * sizeof(int));
  return n;
}

}  // extern "C"
