// rectdetect-mi355x: the compositor - colours and images written into the quads of a frame behind the detector's poll (the contract: include/rectdetect_hip.h,
// "composited quads"; the kernel: rd_k_composite.hip; the host's arithmetic: rd_comp_host.c; the jobs in flight, the frame's checks and its ways: rd_jobs.h).
//
// A job into another frame is the in-place job on a copy: the copy engine (or a blit) brings the source's rows to the destination on the stream, then the in-place
// launch runs there on the touched tiles only.  A pass over all tiles that reads the source and writes the destination would be a second kernel shape for the same
// bytes; the copy moves them at the memory system's rate and needs no code ("Composited quads").
#include "rd_jobs.h"
#include "rd_comp.h"
#include <math.h>
#include <stdio.h>

using namespace rdjob;

static_assert(sizeof(rd_comp_item) == 72 && sizeof(rd_comp_rec) == 96, "the layouts the header and the bindings state");

namespace {

// a job's block, pinned staging and device memory of `cap` bytes each: its n records and, right behind them, its touched tiles as pairs tx, ty - one block so
// that ONE copy brings both to the device (a copy is a blit of 5 us on the stream, half the kernel's own time).  Allocated when the slot first takes a job and
// grown when it takes one that needs more
struct Block { uint8_t *h_blk, *d_blk; size_t cap; };

}  // namespace

struct rd_compositor {
  Ring ring;                                // (first: rd_jobs.h)
  int pw, ph;
  size_t patch_bytes;
  Block *jobs;                              // per slot
  DevBuf oframe, patches;                   // frames on their way to pinned host memory travel through `oframe`, patches from host or pinned memory through `patches`
  uint8_t *mark; size_t mark_bytes;         // a byte per tile of the largest frame so far, all zero between jobs (rd_comp_tiles_of)
};

extern "C" {

rd_compositor *rd_compositor_create(int device, int pw, int ph, int max_items, int njobs) {
  if (pw < 1 || ph < 1 || pw > 16384 || ph > 16384 || max_items < 1 || max_items > (1 << 20) || !ring_args_ok(device, njobs)) return NULL;
  rd_compositor *c = (rd_compositor *)calloc(1, sizeof(*c));
  ring_create(&c->ring, RD_MAGIC_COMPOSITOR, device, max_items, njobs);
  c->pw = pw; c->ph = ph;
  c->patch_bytes = (size_t)pw * ph * 3;
  c->jobs = (Block *)calloc(njobs, sizeof(Block));
  return c;
}

void rd_compositor_destroy(rd_compositor *c) {
  if (!c) return;
  Ring *g = ring_of(c, RD_MAGIC_COMPOSITOR, "rd_compositor_destroy");
  const int njobs = g->njobs;
  ring_destroy(g);
  for (int k = 0; k < njobs; k++) {
    if (c->jobs[k].h_blk) RD_HIP(hipHostFree(c->jobs[k].h_blk));
    if (c->jobs[k].d_blk) RD_HIP(hipFree(c->jobs[k].d_blk));
  }
  c->oframe.release();
  c->patches.release();
  free(c->mark);
  free(c->jobs);
  free(c);
}

long rd_compositor_enqueue(rd_compositor *c, int format, const void *const planes[3], const int pitches[3], int iw, int ih, int on_device,
                           const rd_comp_item *items, int n, const void *patches, int npatches, int patches_kind,
                           void *const out_planes[3], const int out_pitches[3], int out_kind) {
  static const char who[] = "rd_compositor_enqueue";
  Ring *g = ring_of(c, RD_MAGIC_COMPOSITOR, who);
  // argument errors: -1, nothing enqueued
  PixLayout L;
  if (!frame_ok(format, planes, pitches, iw, ih, on_device, &L) || !dest_ok(L, out_planes, out_pitches, out_kind, on_device)) return -1;
  if (n < 0 || n > g->per_job || (n > 0 && !items) || npatches < 0) return -1;
  bool pastes = false;
  for (int k = 0; k < n; k++) {
    if (items[k].patch < -1 || items[k].patch >= npatches) return -1;
    pastes = pastes || items[k].patch >= 0;
  }
  if (pastes && (!patches || (patches_kind != RD_FRAME_HOST && patches_kind != RD_FRAME_DEVICE && patches_kind != RD_FRAME_HOST_PINNED))) return -1;
  RD_HIP(hipSetDevice(g->device));
  if (!dest_memory_ok(L, out_planes, out_kind)) return -1;
  if (pastes && patches_kind == RD_FRAME_DEVICE && !is_kind(patches, RD_FRAME_DEVICE)) return -1;
  Block *j = &c->jobs[ring_claim(g, who, n)];
  // the items are taken here: the caller may reuse the array when the call returns
  const int gx = (iw + RD_COMP_TILE_W - 1) / RD_COMP_TILE_W, gy = (ih + RD_COMP_TILE_H - 1) / RD_COMP_TILE_H;
  // the block holds max_items records from its first job on; the tile list behind them may need more
  if (!j->h_blk) {
    j->cap = (size_t)g->per_job * sizeof(rd_comp_rec) + 4096 * 2 * sizeof(int32_t);
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
  const bool inplace = out_planes == NULL, to_pinned = !inplace && out_kind == RD_FRAME_HOST_PINNED;
  if (!(inplace && ntiles == 0)) {      // (that job has nothing to write)
    PixFrame dst = planes_at(planes, pitches, L);      // in place
    if (to_pinned) { c->oframe.grow(g->st, L.bytes); dst = c->oframe.packed(L); }
    else if (!inplace) dst = planes_at(out_planes, out_pitches, L);
    if (!inplace) bring(g->st, who, L, dst, planes, pitches, on_device);      // the source's pixels straight to where the job runs
    if (ntiles > 0) {
      const uint8_t *dpatches = NULL;
      if (pastes) {
        if (patches_kind == RD_FRAME_DEVICE) dpatches = (const uint8_t *)patches;      // read where they lie
        else {
          if (patches_kind == RD_FRAME_HOST_PINNED && memory_type(patches) != hipMemoryTypeHost)
            exitf(-1, "rd_compositor_enqueue: patches of kind RD_FRAME_HOST_PINNED need pinned host memory; %p is not\n", patches);
          const size_t bytes = (size_t)npatches * c->patch_bytes;
          c->patches.grow(g->st, bytes);
          RD_HIP(hipMemcpyAsync(c->patches.p, patches, bytes, hipMemcpyHostToDevice, g->st));
          if (patches_kind == RD_FRAME_HOST) RD_HIP(hipStreamSynchronize(g->st));
          dpatches = c->patches.p;
        }
      }
      RD_HIP(hipMemcpyAsync(j->d_blk, j->h_blk, recs_bytes + (size_t)ntiles * 2 * sizeof(int32_t), hipMemcpyHostToDevice, g->st));
      rdk::composite(g->st, format, dst, (const rd_comp_rec *)j->d_blk, n, (const int32_t *)(j->d_blk + recs_bytes), ntiles, dpatches, c->pw, c->ph);
      rdrt::check_launch("composited quads");
    }
    if (to_pinned) send(g->st, L, out_planes, out_pitches, dst);
  }
  return ring_record(g);
}

int rd_compositor_wait(rd_compositor *c, uint8_t *status_out) {
  Ring *g = ring_of(c, RD_MAGIC_COMPOSITOR, "rd_compositor_wait");
  const int slot = ring_wait(g);
  if (slot < 0) return -1;
  if (status_out) for (int k = 0; k < g->n[slot]; k++) status_out[k] = ((const rd_comp_rec *)c->jobs[slot].h_blk)[k].status;
  return g->n[slot];
}

}  // extern "C"
