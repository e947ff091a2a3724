// rectdetect-mi355x: the compositor - colours and images written into the quads of a frame behind the detector's poll (the contract: include/rectdetect_hip.h,
// "composited quads"; the kernel: rd_k_composite.hip; the host's arithmetic: rd_comp_host.c).  Built like the annotator (rd_annotate.hip): one non-blocking stream of
// its own, one event per job in flight; no graphs, no threads, no environment switches.
//
// A job into another frame is the in-place job on a copy: the copy engine (or a blit) brings the source's rows to the destination on the stream, then the in-place
// launch runs there on the touched tiles only.  A pass over all tiles that reads the source and writes the destination would be a second kernel shape for the same
// bytes; the copy moves them at the memory system's rate and needs no code ("Composited quads").
#include "rd_internal.h"
#include "rd_comp.h"
#include "rectdetect_hip.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAGIC_COMPOSITOR 0x5244434fu

static_assert(sizeof(rd_comp_item) == 72 && sizeof(rd_comp_rec) == 96, "the layouts the header and the bindings state");

namespace {

struct Job {
  hipEvent_t done;
  // this job's block, pinned staging and device memory of `cap` bytes each: its n records and, right behind them, its touched tiles as pairs tx, ty - one block so
  // that ONE copy brings both to the device (a copy is a blit of 5 us on the stream, half the kernel's own time).  Allocated when the slot first takes a job and
  // grown when it takes one that needs more
  uint8_t *h_blk, *d_blk;
  size_t cap;
  int n;
};

// the planes a format uses, their row bytes and rows; a frame in the compositor's own buffer is packed with row strides rounded up to 4 bytes (rd_annotate.hip's)
struct Layout { int np, row[3], rows[3], pitch[3]; size_t off[3], bytes; };
Layout layout(int fmt, int iw, int ih) {
  Layout L;
  memset(&L, 0, sizeof(L));
  const int bpp = fmt == RD_PIX_BGR || fmt == RD_PIX_RGB ? 3 : 4;
  if (fmt <= RD_PIX_RGBA) { L.np = 1; L.row[0] = iw * bpp; L.rows[0] = ih; }
  else if (fmt == RD_PIX_NV12) { L.np = 2; L.row[0] = L.row[1] = iw; L.rows[0] = ih; L.rows[1] = ih / 2; }
  else { L.np = 3; L.row[0] = iw; L.rows[0] = ih; L.row[1] = L.row[2] = iw / 2; L.rows[1] = L.rows[2] = ih / 2; }
  for (int k = 0; k < L.np; k++) { L.pitch[k] = (L.row[k] + 3) & ~3; L.off[k] = L.bytes; L.bytes += (size_t)L.pitch[k] * L.rows[k]; }
  return L;
}

hipMemoryType memory_type(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return hipMemoryTypeUnregistered; }
  return at.type;
}

void ensure(uint8_t **buf, size_t *have, size_t want, hipStream_t st) {
  if (*have >= want) return;
  RD_HIP(hipStreamSynchronize(st));      // (jobs in flight use the old one)
  if (*buf) RD_HIP(hipFree(*buf));
  RD_HIP(hipMalloc((void **)buf, want));
  *have = want;
}

}  // namespace

struct rd_compositor {
  uint32_t magic;
  int device, pw, ph, max_items, njobs;
  size_t patch_bytes;
  hipStream_t st;
  Job *jobs;
  long next_enqueue, next_wait;
  // frames on their way to pinned host memory travel through `oframe`, patches from host or pinned memory through `patches` (both grow on demand; jobs follow one
  // another on st, so one buffer of each serves them all)
  uint8_t *oframe, *patches; size_t oframe_bytes, patches_bytes;
  uint8_t *mark; size_t mark_bytes;         // a byte per tile of the largest frame so far, all zero between jobs (rd_comp_tiles_of)
};

namespace rdrt {
int compositor_device(const rd_compositor *c) { return c && c->magic == MAGIC_COMPOSITOR ? c->device : -1; }
int compositor_max_items(const rd_compositor *c) { return c && c->magic == MAGIC_COMPOSITOR ? c->max_items : -1; }
}

extern "C" {

rd_compositor *rd_compositor_create(int device, int pw, int ph, int max_items, int njobs) {
  if (pw < 1 || ph < 1 || pw > 16384 || ph > 16384 || max_items < 1 || max_items > (1 << 20) || njobs < 1 || njobs > 1024) return NULL;
  if (device < 0 || device >= rd_device_count()) return NULL;
  RD_HIP(hipSetDevice(device));
  rd_compositor *c = (rd_compositor *)calloc(1, sizeof(*c));
  c->magic = MAGIC_COMPOSITOR;
  c->device = device; c->pw = pw; c->ph = ph; c->max_items = max_items; c->njobs = njobs;
  c->patch_bytes = (size_t)pw * ph * 3;
  RD_HIP(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
  c->jobs = (Job *)calloc(njobs, sizeof(Job));
  for (int k = 0; k < njobs; k++) RD_HIP(hipEventCreateWithFlags(&c->jobs[k].done, hipEventDisableTiming));
  return c;
}

void rd_compositor_destroy(rd_compositor *c) {
  if (!c) return;
  if (c->magic != MAGIC_COMPOSITOR) exitf(-1, "rd_compositor_destroy: bad handle\n");
  RD_HIP(hipSetDevice(c->device));
  RD_HIP(hipStreamSynchronize(c->st));
  for (int k = 0; k < c->njobs; k++) {
    RD_HIP(hipEventDestroy(c->jobs[k].done));
    if (c->jobs[k].h_blk) RD_HIP(hipHostFree(c->jobs[k].h_blk));
    if (c->jobs[k].d_blk) RD_HIP(hipFree(c->jobs[k].d_blk));
  }
  RD_HIP(hipStreamDestroy(c->st));
  if (c->oframe) RD_HIP(hipFree(c->oframe));
  if (c->patches) RD_HIP(hipFree(c->patches));
  free(c->mark);
  free(c->jobs);
  c->magic = 0;
  free(c);
}

long rd_compositor_enqueue(rd_compositor *c, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                           const rd_comp_item *items, int n, const void *patches, int npatches, int patches_kind,
                           void *const out_planes[3], const int out_pitches[3], int out_kind) {
  if (!c || c->magic != MAGIC_COMPOSITOR) exitf(-1, "rd_compositor_enqueue: bad handle\n");
  // argument errors: -1, nothing enqueued
  if (format < RD_PIX_BGR || format > RD_PIX_I420 || !planes || !pitches || iw < 1 || ih < 1 || iw > 65536 || ih > 65536) return -1;
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) return -1;
  if (format >= RD_PIX_NV12 && ((iw | ih) & 1)) return -1;
  const Layout L = layout(format, iw, ih);
  for (int k = 0; k < L.np; k++) if (!planes[k] || pitches[k] < L.row[k]) return -1;
  const bool inplace = out_planes == NULL;
  if (inplace) {
    if (on_device != RD_FRAME_DEVICE) return -1;
  } else {
    if ((out_kind != RD_FRAME_DEVICE && out_kind != RD_FRAME_HOST_PINNED) || !out_pitches) return -1;
    for (int k = 0; k < L.np; k++) if (!out_planes[k] || out_pitches[k] < L.row[k]) return -1;
  }
  if (n < 0 || n > c->max_items || (n > 0 && !items) || npatches < 0) return -1;
  bool pastes = false;
  for (int k = 0; k < n; k++) {
    if (items[k].patch < -1 || items[k].patch >= npatches) return -1;
    pastes = pastes || items[k].patch >= 0;
  }
  if (pastes && (!patches || (patches_kind != RD_FRAME_HOST && patches_kind != RD_FRAME_DEVICE && patches_kind != RD_FRAME_HOST_PINNED))) return -1;
  RD_HIP(hipSetDevice(c->device));
  if (!inplace)
    for (int k = 0; k < L.np; k++)
      if (memory_type(out_planes[k]) != (out_kind == RD_FRAME_DEVICE ? hipMemoryTypeDevice : hipMemoryTypeHost)) return -1;
  if (pastes && patches_kind == RD_FRAME_DEVICE && memory_type(patches) != hipMemoryTypeDevice) return -1;
  if (c->next_enqueue - c->next_wait >= c->njobs) exitf(-1, "rd_compositor_enqueue: %d jobs already in flight (wait first)\n", c->njobs);
  Job *j = &c->jobs[c->next_enqueue % c->njobs];
  j->n = n;
  // the items are taken here: the caller may reuse the array when the call returns
  const int gx = (iw + RD_COMP_TILE_W - 1) / RD_COMP_TILE_W, gy = (ih + RD_COMP_TILE_H - 1) / RD_COMP_TILE_H;
  // the block holds max_items records from its first job on; the tile list behind them may need more
  if (!j->h_blk) {
    j->cap = (size_t)c->max_items * sizeof(rd_comp_rec) + 4096 * 2 * sizeof(int32_t);
    RD_HIP(hipHostMalloc((void **)&j->h_blk, j->cap, hipHostMallocDefault));
    RD_HIP(hipMalloc((void **)&j->d_blk, j->cap));
  }
  rd_comp_rec *h_recs = (rd_comp_rec *)j->h_blk;
  size_t reach = 0;      // tiles the boxes reach, counted with repetition: an upper bound of the list's length, as is the number of tiles
  for (int k = 0; k < n; k++) {
    rd_comp_rec *r = &h_recs[k];
    rd_comp_make_rec(items[k].quad, iw, ih, r);
    r->patch = items[k].patch;
    r->col[0] = items[k].b; r->col[1] = items[k].g; r->col[2] = items[k].r;
    if (r->status && r->box[0] <= r->box[2] && r->box[1] <= r->box[3])
      reach += (size_t)(r->box[2] / RD_COMP_TILE_W - r->box[0] / RD_COMP_TILE_W + 1) * (size_t)(r->box[3] / RD_COMP_TILE_H - r->box[1] / RD_COMP_TILE_H + 1);
  }
  if (reach > (size_t)gx * gy) reach = (size_t)gx * gy;
  const size_t recs_bytes = (size_t)n * sizeof(rd_comp_rec), need = recs_bytes + reach * 2 * sizeof(int32_t);
  if (j->cap < need) {      // (the job that had this slot before has been waited for: nothing on the device uses its block)
    uint8_t *h_new;
    RD_HIP(hipHostMalloc((void **)&h_new, need, hipHostMallocDefault));
    memcpy(h_new, j->h_blk, recs_bytes);
    RD_HIP(hipHostFree(j->h_blk));
    RD_HIP(hipFree(j->d_blk));
    j->h_blk = h_new;
    RD_HIP(hipMalloc((void **)&j->d_blk, need));
    j->cap = need;
    h_recs = (rd_comp_rec *)j->h_blk;
  }
  int32_t *h_tiles = (int32_t *)(j->h_blk + recs_bytes);
  int ntiles = 0;
  if (reach > 0) {
    if (c->mark_bytes < (size_t)gx * gy) {
      free(c->mark);
      c->mark = (uint8_t *)calloc((size_t)gx * gy, 1);
      if (!c->mark) exitf(-1, "rd_compositor_enqueue: out of memory\n");
      c->mark_bytes = (size_t)gx * gy;
    }
    ntiles = rd_comp_tiles_of(h_recs, n, iw, ih, c->mark, h_tiles, (int)reach);
  }
  if (!(inplace && ntiles == 0)) {      // (that job has nothing to write)
    uint8_t *dst[3] = { NULL, NULL, NULL };
    int dpitch[3] = { 0, 0, 0 };
    if (inplace) {
      for (int k = 0; k < L.np; k++) { dst[k] = (uint8_t *)planes[k]; dpitch[k] = pitches[k]; }
    } else {
      if (out_kind == RD_FRAME_DEVICE) {
        for (int k = 0; k < L.np; k++) { dst[k] = (uint8_t *)out_planes[k]; dpitch[k] = out_pitches[k]; }
      } else {
        ensure(&c->oframe, &c->oframe_bytes, L.bytes, c->st);
        for (int k = 0; k < L.np; k++) { dst[k] = c->oframe + L.off[k]; dpitch[k] = L.pitch[k]; }
      }
      // the source's pixels, row bytes only (pitch padding is never written), straight to where the job runs
      if (on_device == RD_FRAME_HOST_PINNED)
        for (int k = 0; k < L.np; k++)
          if (memory_type(planes[k]) != hipMemoryTypeHost)
            exitf(-1, "rd_compositor_enqueue: RD_FRAME_HOST_PINNED needs pinned host memory (rd_host_alloc, allocatePinnedMemory, hipHostMalloc, hipHostRegister); plane %d at %p is not\n", k, planes[k]);
      for (int k = 0; k < L.np; k++)
        RD_HIP(hipMemcpy2DAsync(dst[k], dpitch[k], planes[k], pitches[k], L.row[k], L.rows[k], on_device == RD_FRAME_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->st));
      if (on_device == RD_FRAME_HOST) RD_HIP(hipStreamSynchronize(c->st));      // (pageable memory: the caller may reuse the buffer when this call returns)
    }
    if (ntiles > 0) {
      const uint8_t *dpatches = NULL;
      if (pastes) {
        if (patches_kind == RD_FRAME_DEVICE) dpatches = (const uint8_t *)patches;      // read where they lie
        else {
          if (patches_kind == RD_FRAME_HOST_PINNED && memory_type(patches) != hipMemoryTypeHost)
            exitf(-1, "rd_compositor_enqueue: patches of kind RD_FRAME_HOST_PINNED need pinned host memory; %p is not\n", patches);
          const size_t bytes = (size_t)npatches * c->patch_bytes;
          ensure(&c->patches, &c->patches_bytes, bytes, c->st);
          RD_HIP(hipMemcpyAsync(c->patches, patches, bytes, hipMemcpyHostToDevice, c->st));
          if (patches_kind == RD_FRAME_HOST) RD_HIP(hipStreamSynchronize(c->st));
          dpatches = c->patches;
        }
      }
      RD_HIP(hipMemcpyAsync(j->d_blk, j->h_blk, recs_bytes + (size_t)ntiles * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->st));
      rdk::composite(c->st, format, dst, dpitch, iw, ih, (const rd_comp_rec *)j->d_blk, n, (const int32_t *)(j->d_blk + recs_bytes), ntiles, dpatches, c->pw, c->ph);
      rdrt::check_launch("composited quads");
    }
    if (!inplace && out_kind == RD_FRAME_HOST_PINNED)
      for (int k = 0; k < L.np; k++)      // row bytes only: the caller's pitch padding stays as it is
        RD_HIP(hipMemcpy2DAsync(out_planes[k], out_pitches[k], dst[k], dpitch[k], L.row[k], L.rows[k], hipMemcpyDeviceToHost, c->st));
  }
  RD_HIP(hipEventRecord(j->done, c->st));
  return c->next_enqueue++;
}

int rd_compositor_wait(rd_compositor *c, uint8_t *status_out) {
  if (!c || c->magic != MAGIC_COMPOSITOR) exitf(-1, "rd_compositor_wait: bad handle\n");
  if (c->next_wait >= c->next_enqueue) return -1;
  RD_HIP(hipSetDevice(c->device));
  Job *j = &c->jobs[c->next_wait % c->njobs];
  RD_HIP(hipEventSynchronize(j->done));
  if (status_out) for (int k = 0; k < j->n; k++) status_out[k] = ((const rd_comp_rec *)j->h_blk)[k].status;
  c->next_wait++;
  return j->n;
}

}  // extern "C"
