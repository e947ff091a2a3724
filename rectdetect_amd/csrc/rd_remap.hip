// rectdetect-mi355x: the remapper - lens-undistorted frames ahead of the detector (the contract: include/rectdetect_hip.h, "remapped frames"; the table:
// rd_remap_host.c; the kernel: rd_k_remap.hip; the jobs in flight, the frame's checks and its way to the device: rd_jobs.h).
#include "rd_jobs.h"
#include "rd_kernels.h"
#include "rd_remap_host.h"

using namespace rdjob;

struct rd_remapper {
  Ring ring;                  // (first: rd_jobs.h)
  int ow, oh, iw, ih, inside;
  int tpitch;                 // entries of a row of d_table (rdk::remap_table_pitch)
  int spitch;                 // bytes of a row of a staging frame: 3 * ow rounded up to 4
  int32_t *d_table;           // oh rows of tpitch entries, uploaded once
  uint8_t **d_out;            // per slot: a frame on its way to pinned host memory (allocated on first use)
  DevBuf frame;               // host and pinned frames travel through here
};

// host_table: malloc'd ow * oh entries, or NULL; tabulate fills it and returns the entries inside, or -1
template <class F> static rd_remapper *remapper_create(int device, int ow, int oh, int iw, int ih, int njobs, F &&tabulate) {
  if (!rd_remap_sizes_ok(ow, oh, iw, ih) || !ring_args_ok(device, njobs)) return NULL;
  int32_t *table = (int32_t *)malloc((size_t)ow * oh * 2 * sizeof(int32_t));
  if (!table) return NULL;
  const int inside = tabulate(table);
  if (inside < 0) { free(table); return NULL; }
  rd_remapper *r = (rd_remapper *)calloc(1, sizeof(*r));
  ring_create(&r->ring, RD_MAGIC_REMAPPER, device, 1, njobs);
  r->ow = ow; r->oh = oh; r->iw = iw; r->ih = ih; r->inside = inside;
  r->tpitch = rdk::remap_table_pitch(ow);
  r->spitch = (3 * ow + 3) & ~3;
  const size_t trow = (size_t)r->tpitch * 2 * sizeof(int32_t);
  RD_HIP(hipMalloc((void **)&r->d_table, trow * oh));
  RD_HIP(hipMemsetAsync(r->d_table, 0xff, trow * oh, r->ring.st));      // (the padding entries: -1, -1)
  RD_HIP(hipMemcpy2DAsync(r->d_table, trow, table, (size_t)ow * 2 * sizeof(int32_t), (size_t)ow * 2 * sizeof(int32_t), oh, hipMemcpyHostToDevice, r->ring.st));
  RD_HIP(hipStreamSynchronize(r->ring.st));
  free(table);
  r->d_out = (uint8_t **)calloc(njobs, sizeof(uint8_t *));
  return r;
}

extern "C" {

rd_remapper *rd_remapper_create_lens(int device, const rd_lens *lens, const rd_view *view, int ow, int oh, int iw, int ih, int njobs) {
  if (!lens || !view) return NULL;
  return remapper_create(device, ow, oh, iw, ih, njobs, [&](int32_t *table) { return rd_remap_table_lens(lens, view, ow, oh, iw, ih, table); });
}

rd_remapper *rd_remapper_create_map(int device, const float *mapx, const float *mapy, int ow, int oh, int iw, int ih, int njobs) {
  if (!mapx || !mapy) return NULL;
  return remapper_create(device, ow, oh, iw, ih, njobs, [&](int32_t *table) { return rd_remap_table_map(mapx, mapy, ow, oh, iw, ih, table); });
}

void rd_remapper_destroy(rd_remapper *r) {
  if (!r) return;
  Ring *g = ring_of(r, RD_MAGIC_REMAPPER, "rd_remapper_destroy");
  const int njobs = g->njobs;
  ring_destroy(g);
  for (int k = 0; k < njobs; k++) if (r->d_out[k]) RD_HIP(hipFree(r->d_out[k]));
  RD_HIP(hipFree(r->d_table));
  r->frame.release();
  free(r->d_out);
  free(r);
}

int rd_remapper_inside(const rd_remapper *r) { return r && r->ring.magic == RD_MAGIC_REMAPPER ? r->inside : -1; }

long rd_remapper_enqueue(rd_remapper *r, int format, const void *const planes[3], const int pitches[3], int on_device, uint32_t fill_bgr, void *out, int out_pitch,
                         int out_kind) {
  static const char who[] = "rd_remapper_enqueue";
  Ring *g = ring_of(r, RD_MAGIC_REMAPPER, who);
  // argument errors: -1, nothing enqueued
  PixLayout L;
  if (!frame_ok(format, planes, pitches, r->iw, r->ih, on_device, &L)) return -1;
  if ((out_kind != RD_FRAME_DEVICE && out_kind != RD_FRAME_HOST_PINNED) || !out || out_pitch < 3 * r->ow) return -1;
  RD_HIP(hipSetDevice(g->device));
  if (!is_kind(out, out_kind)) return -1;
  const int slot = ring_claim(g, who, 1);
  PixFrame src = planes_at(planes, pitches, L);      // a device frame: read where it lies
  if (on_device != RD_FRAME_DEVICE) {              // through the remapper's own buffer, one plane after the other
    r->frame.grow(g->st, L.bytes);
    src = r->frame.packed(L);
    bring(g->st, who, L, src, planes, pitches, on_device);
  }
  if (out_kind == RD_FRAME_DEVICE) {
    rdk::remap(g->st, (uint8_t *)out, out_pitch, format, src, r->d_table, r->ow, r->oh, fill_bgr);
    rdrt::check_launch("remapped frame");
  } else {      // (the copy engine writes the row bytes only: the caller's pitch padding stays as it is)
    if (!r->d_out[slot]) RD_HIP(hipMalloc((void **)&r->d_out[slot], (size_t)r->spitch * r->oh));      // (on first use: a remapper that writes to device memory only has none)
    rdk::remap(g->st, r->d_out[slot], r->spitch, format, src, r->d_table, r->ow, r->oh, fill_bgr);
    rdrt::check_launch("remapped frame");
    RD_HIP(hipMemcpy2DAsync(out, out_pitch, r->d_out[slot], r->spitch, (size_t)3 * r->ow, r->oh, hipMemcpyDeviceToHost, g->st));
  }
  return ring_record(g);
}

int rd_remapper_wait(rd_remapper *r) {
  Ring *g = ring_of(r, RD_MAGIC_REMAPPER, "rd_remapper_wait");
  return ring_wait(g) < 0 ? -1 : 0;
}

}  // extern "C"
