// rectdetect-mi355x: the detector's objects - a slot's planes, streams and events, create / destroy of both kinds, counters, debug planes - and the reference's
// rectangle API (oclrect.h), a shim over a detector with two slots.  What a frame passes through lives in rd_frames.hip.
#include "rd_detector.h"
#include <sched.h>

extern "C" {
#include "rd_post.h"
}

#define RD_POLY_HANDOFF_DEFAULT 2048      // records handed off per frame: 112 KB of pinned memory per slot

// The device planes of a slot: the one list of them, both kinds, in layout order.  Every detector carves its slots out of one allocation (rd_detector::arena): slot k
// at arena + k * slot_pitch, its planes in the order of the rows its kind owns, each rounded up to 256 bytes.  The planes of slot k + z then lie a constant number
// of bytes behind those of slot k - a kernel of a group launch reaches frame z's planes as `pointer + blockIdx.z * pitch` - and a frame that is launched on its own
// runs on the layout the groups use: a kernel that runs past its plane lands in the neighbouring plane in every configuration.
// Offsets, the slot's size and the Slot's pointers all come from one walk of this list (slot_planes); nothing else names the planes.
#define PK_RECT 1
#define PK_POLY 2
#define PK_POLY_UNFUSED 4      // the polyline kind at frame sizes the fused front kernel's tiles do not cover (!front_is_fused): the three operators need their planes
#define PK_BOTH (PK_RECT | PK_POLY)
typedef size_t PlaneCount(const rd_detector *d);      // elements of a plane
static size_t pn_n(const rd_detector *d) { return (size_t)d->N; }
static size_t pn_2n(const rd_detector *d) { return (size_t)d->N * 2; }
static size_t pn_4n(const rd_detector *d) { return (size_t)d->N * 4; }
static size_t pn_16n(const rd_detector *d) { return (size_t)d->N * 16; }
static size_t pn_scratch2(const rd_detector *d) { return (size_t)d->N * 3 + 256; }      // region_merge: the initial forest, flags + allow bytes, the second label plane of the rounds
static size_t pn_d2(const rd_detector *d) { return RD_D2_SCRATCH_INTS(d->N); }
static size_t pn_bits(const rd_detector *d) { return (size_t)((d->iw + 63) / 64) * d->ih + 8; }      // a bit plane: ceil(iw / 64) words per row
static size_t pn_tails(const rd_detector *d) { const size_t a = rdk::iir_pass_scratch_floats(3, d->ih, d->iw), b = rdk::iir_pass_scratch_floats(3, d->iw, d->ih); return a > b ? a : b; }
static size_t pn_flags(const rd_detector *) { return 16; }
static size_t pn_probes(const rd_detector *d) { return (size_t)d->maxrec_dev * RD_PROBE_INTS; }
#define PLANE(field, count, kinds) { offsetof(Slot, field), sizeof(*((Slot *)0)->field), count, kinds }
#define BLUR_PLANES(k) PLANE(tr[k], pn_n, PK_BOTH), PLANE(fw[k], pn_n, PK_BOTH), PLANE(bw[k], pn_n, PK_BOTH), PLANE(hz[k], pn_n, PK_BOTH), PLANE(bl[k], pn_n, PK_BOTH)
static const struct { size_t field, elem; PlaneCount *count; int kinds; } kSlotPlanes[] = {
  PLANE(bgr, pn_4n, PK_BOTH),
  PLANE(plab0, pn_n, PK_BOTH),            // (polyline kind: the colour conversion's packed output is read by nothing but the debug plane)
  PLANE(plab1, pn_n, PK_RECT), PLANE(smooth, pn_n, PK_RECT), PLANE(quant, pn_n, PK_RECT),
  BLUR_PLANES(0), BLUR_PLANES(1), BLUR_PLANES(2),
  PLANE(plab1, pn_n, PK_POLY_UNFUSED),    // (the polyline kind has it behind the blur's planes: a second row, so that no plane of either kind moves)
  PLANE(vxy, pn_2n, PK_RECT | PK_POLY_UNFUSED), PLANE(strength, pn_n, PK_RECT | PK_POLY_UNFUSED),
  PLANE(nms, pn_n, PK_BOTH),
  PLANE(i0, pn_n, PK_RECT), PLANE(i1, pn_n, PK_RECT), PLANE(mask0, pn_n, PK_BOTH), PLANE(tidy, pn_n, PK_RECT), PLANE(label1, pn_n, PK_BOTH), PLANE(strsum, pn_n, PK_BOTH),
  PLANE(region, pn_n, PK_RECT), PLANE(rsize, pn_n, PK_RECT), PLANE(boundarysrc, pn_n, PK_RECT), PLANE(boundary, pn_n, PK_RECT), PLANE(lsid, pn_n, PK_BOTH), PLANE(region0, pn_n, PK_RECT),
  PLANE(scratch2, pn_scratch2, PK_RECT), PLANE(d2s, pn_d2, PK_RECT),
  PLANE(table, pn_4n, PK_RECT), PLANE(claim, pn_n, PK_RECT), PLANE(tlist, pn_n, PK_RECT),
  PLANE(e8, pn_n, PK_RECT),
  PLANE(strongbits, pn_bits, PK_BOTH),    // (polyline kind: the poly mask, what the polyline stage traces)
  PLANE(mmbits, pn_bits, PK_RECT),
  PLANE(ext, pn_n, PK_RECT),
  PLANE(tails, pn_tails, PK_BOTH), PLANE(flags, pn_flags, PK_BOTH),
  { offsetof(Slot, lslist), 1, pn_16n, PK_BOTH },      // (bytes: the list has the reference's capacity)
  PLANE(probes, pn_probes, PK_RECT),
};
#undef BLUR_PLANES
#undef PLANE

// The walk: the size of a slot of d's kind; with s != NULL also s's pointers, into the slot's range at `base`.
static size_t slot_planes(const rd_detector *d, Slot *s, char *base) {
  const int kind = d->kind == RD_KIND_POLY ? PK_POLY | (front_is_fused(d) ? 0 : PK_POLY_UNFUSED) : PK_RECT;
  size_t at = 0;
  for (const auto &r : kSlotPlanes) {
    if (!(r.kinds & kind)) continue;
    if (s) { char *p = base + at; memcpy((char *)s + r.field, &p, sizeof(p)); }
    at += (r.count(d) * r.elem + 255) & ~(size_t)255;
  }
  return at;
}

// Streams of the high-priority pool (see slot_alloc) are kept for the life of the process and handed to the next detector of the same device: a detector
// that is closed and another one opened (bench.py's side configurations after the headline) then runs on the same hardware queues instead of a second set.
static struct { pthread_mutex_t mu; hipStream_t st[64]; int dev[64]; int n; } stream_pool = { PTHREAD_MUTEX_INITIALIZER };
hipStream_t pooled_stream(int device) {
  hipStream_t st = NULL;
  pthread_mutex_lock(&stream_pool.mu);
  for (int i = 0; i < stream_pool.n; i++) if (stream_pool.dev[i] == device) { st = stream_pool.st[i]; stream_pool.st[i] = stream_pool.st[stream_pool.n - 1]; stream_pool.dev[i] = stream_pool.dev[stream_pool.n - 1]; stream_pool.n--; break; }
  pthread_mutex_unlock(&stream_pool.mu);
  if (st) {      // (handed back idle - its last user synchronised it; one that reports an error instead is not handed out again)
    const hipError_t e = hipStreamQuery(st);
    if (e == hipSuccess || e == hipErrorNotReady) return st;
    (void)hipGetLastError();
    (void)hipStreamDestroy(st);
  }
  int lo = 0, hi = 0;
  RD_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
  RD_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi));
  return st;
}
static void unpool_stream(int device, hipStream_t st) {
  pthread_mutex_lock(&stream_pool.mu);
  const bool room = stream_pool.n < 64;
  if (room) { stream_pool.st[stream_pool.n] = st; stream_pool.dev[stream_pool.n] = device; stream_pool.n++; }
  pthread_mutex_unlock(&stream_pool.mu);
  if (!room) RD_HIP(hipStreamDestroy(st));
}

// the pool's teardown, for a caller that wants the streams gone (they are otherwise kept until the process ends, at most 64 of them): destroys every pooled stream
// of `device` (-1: of every device); streams in use by a live detector are not in the pool and are not touched
extern "C" void rd_release_cached_streams(int device) {
  hipStream_t gone[64]; int dev[64]; int n = 0;
  pthread_mutex_lock(&stream_pool.mu);
  for (int i = 0; i < stream_pool.n;) {
    if (device < 0 || stream_pool.dev[i] == device) {
      gone[n] = stream_pool.st[i]; dev[n] = stream_pool.dev[i]; n++;
      stream_pool.st[i] = stream_pool.st[stream_pool.n - 1]; stream_pool.dev[i] = stream_pool.dev[stream_pool.n - 1]; stream_pool.n--;
    } else i++;
  }
  pthread_mutex_unlock(&stream_pool.mu);
  for (int i = 0; i < n; i++) { RD_HIP(hipSetDevice(dev[i])); RD_HIP(hipStreamSynchronize(gone[i])); RD_HIP(hipStreamDestroy(gone[i])); }
}

// A slot's stream for repeats and fetches (created on first use): from the runtime's high-priority pool of hardware queues.  As ordinary streams they share the
// four queues of the default pool with the four streams that carry the groups, so a repeat - the oldest frame in flight, the one the caller waits for - stood in a queue
// behind whole groups of later frames after all (the reason it has a stream of its own); with queues of their own: 2853 against 2776-2791 frames/s on one box
// (RD_REDO_STREAM_PRIORITY=0: ordinary streams).  The group streams themselves stay in the default pool: moved to the high-priority pool they gain as much at 1920x1080
// but a detector opened after another one was closed in the same process (bench.py's side configurations) then ran 10-16 % slower - not understood, not kept.
hipStream_t make_redo_stream() {
  static const int prio = RD_LAB_INT("RD_REDO_STREAM_PRIORITY", 1);
  hipStream_t st = NULL;
  if (prio) { int lo = 0, hi = 0; RD_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi)); RD_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi)); }
  else RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  return st;
}

// the events of a slot; ev_begin / ev_done carry timestamps (device time of the frame: rd_detector_counter 1)
static const struct { hipEvent_t Slot::*ev; bool timing; } kSlotEvents[] = {
  { &Slot::ev_fork, false }, { &Slot::ev_join, false }, { &Slot::ev_mm, false }, { &Slot::ev_begin, true }, { &Slot::ev_done, true },
  { &Slot::ev_strong, false }, { &Slot::ev_redo, false }, { &Slot::ev_upload, false }, { &Slot::ev_dense, false },
};

// share: the slot whose streams this one uses as well (NULL: own streams)
static void slot_alloc(rd_detector *d, Slot *s, Slot *share) {
  const size_t N = (size_t)d->N;
  s->shares_streams = share != NULL;
  if (share) { s->st = share->st; s->st2 = share->st2; }
  else {
    // One or two frames in flight: each frame spreads over two streams, and the four streams of two frames need four hardware queues of their own.  The
    // runtime hands its four queues per priority level to the streams in the order they first launch something, and the null stream (set-up copies) and the
    // caller's command queue hold two of them: the second frame's streams then land on the queues of the first frame's - its main chain behind the other's polyline
    // chain (traced: two frames in flight ran 1.18 times as fast as one).  The streams of such a detector therefore come from the pool of another priority
    // level, where nothing else lives.  (Raising the number of queues for everybody - GPU_MAX_HW_QUEUES=8 - does the same for this path, 1420 -> 1590 frames/s, but
    // costs the group path, whose four streams are best served by four queues, 9 %.)
    static const int fork_prio = RD_LAB_INT("RD_FORK_STREAM_PRIORITY", 1);
    const bool from_pool = fork_prio != 0;
    if (d->fork_poly && from_pool) {
      s->st = pooled_stream(d->device);
      s->st2 = pooled_stream(d->device);
      s->pooled_streams = 1;
    } else {
    RD_HIP(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
    RD_HIP(hipStreamCreateWithFlags(&s->st2, hipStreamNonBlocking));
    }
  }
  for (const auto &e : kSlotEvents) { if (e.timing) RD_HIP(hipEventCreate(&(s->*e.ev))); else RD_HIP(hipEventCreateWithFlags(&(s->*e.ev), hipEventDisableTiming)); }
  slot_planes(d, s, d->arena + (size_t)(s - d->slots) * d->slot_pitch);
  // what the planes must hold before the first frame: empty vote tables, the blur's flags at zero
  if (d->kind == RD_KIND_RECT) rdk::reduce_ls_init(s->st, s->table, s->claim, s->tlist, (int)(N * 4 / 5));
  RD_HIP(hipMemset(s->flags, 0, 16 * sizeof(int))); RD_HIP(hipStreamSynchronize(0));
  s->ps = rdk::poly_scratch_create(d->iw, d->ih);
  RD_HIP(hipHostMalloc(&s->h_bgr, N * 4, hipHostMallocDefault));
  // the hand-over block (rd_kernels.h: RD_PACK_*; poly kind: counters + records, no probes)
  const size_t pack_ints = d->kind == RD_KIND_POLY ? RD_PACK_RECORDS + (size_t)d->handoff_rec * RD_REC_INTS : RD_PACK_RECORDS + (size_t)RD_MAXREC * (RD_REC_INTS + RD_PROBE_INTS);
  RD_HIP(hipHostMalloc((void **)&s->h_pack, pack_ints * sizeof(int), hipHostMallocDefault)); memset(s->h_pack, 0, pack_ints * sizeof(int));
  RD_HIP(hipHostGetDevicePointer((void **)&s->h_pack_dev, s->h_pack, 0));
  s->h_ctr = s->h_pack; s->h_segs = s->h_pack + RD_PACK_RECORDS; s->h_probes = s->h_pack + RD_PACK_RECORDS + (size_t)RD_MAXREC * RD_REC_INTS;
  s->rounds = 20;
  s->seq = -1;
  if (d->device_post) {
    s->post_scratch = dnew<int>(rdk::post_scratch_ints());
    RD_HIP(hipHostMalloc((void **)&s->h_post, rdk::post_out_ints() * sizeof(int), hipHostMallocDefault)); memset(s->h_post, 0, rdk::post_out_ints() * sizeof(int));
    RD_HIP(hipHostGetDevicePointer((void **)&s->h_post_dev, s->h_post, 0));
  }
  // descriptor of the sparse stages
  s->frame = d->frames + (s - d->slots);
  rdk::PolyFrame &f = *s->frame;
  memset(&f, 0, sizeof(f));
  f.ps = *s->ps; f.in = NULL; f.in_bits = s->strongbits; f.ring_src = NULL; f.lslist = s->lslist; f.ids = s->lsid;
  f.boundary = s->boundary; f.table = s->table; f.claim = s->claim; f.tlist = s->tlist; f.probes = s->probes; f.pack = s->h_pack_dev; f.rflags = s->scratch2 ? s->scratch2 + N : NULL;
  f.post_scratch = s->post_scratch; f.post_out = s->h_post_dev;
}

static void slot_free(Slot *s, int device) {
  RD_HIP(hipStreamSynchronize(s->st));
  // (the planes: part of the detector's arena, freed with it)
  rdk::poly_scratch_destroy(s->ps);
  RD_HIP(hipHostFree(s->h_bgr)); RD_HIP(hipHostFree(s->h_pack));
  if (s->sc_bgr) RD_HIP(hipFree(s->sc_bgr));
  if (s->sc_h) RD_HIP(hipHostFree(s->sc_h));
  dfree(s->post_scratch); if (s->h_post) RD_HIP(hipHostFree(s->h_post));
  for (const auto &e : kSlotEvents) RD_HIP(hipEventDestroy(s->*e.ev));
  if (s->st_redo) RD_HIP(hipStreamDestroy(s->st_redo));
  dfree(s->big_probes);
  if (!s->shares_streams) {
    if (s->pooled_streams) { RD_HIP(hipStreamSynchronize(s->st2)); RD_HIP(hipStreamSynchronize(s->st)); unpool_stream(device, s->st2); unpool_stream(device, s->st); }
    else {
    RD_HIP(hipStreamDestroy(s->st2));
    RD_HIP(hipStreamDestroy(s->st));
    }
  }
}

// ---- detector set-up: what rd_detector_create and rd_polyline_detector_create share (the argument checks stay with their entry point)
static rd_detector *detector_new(int kind, int device, int iw, int ih, int nslots, int nworkers) {
  RD_HIP(hipSetDevice(device));
  rd_detector *d = (rd_detector *)calloc(1, sizeof(*d));
  d->magic = MAGIC_RECT; d->kind = kind; d->device = device; d->iw = iw; d->ih = ih; d->N = iw * ih; d->nslots = nslots; d->nworkers = nworkers;
  d->maxrec_dev = d->N * 16 / 56;
  if (d->maxrec_dev > 65536) d->maxrec_dev = 65536;      // the slots' probe buffers; frames with more records are probed again into a buffer that grows (slot_rectangles)
  { const int m = rd_env_int("RD_MAXREC_DEV", 0); if (m >= 16 && m < d->maxrec_dev) d->maxrec_dev = m; }      // (tests: exercise that path)
  d->use_graph = rd_env("RD_NO_GRAPH") ? 0 : 1;
  d->poly_mode = rd_env("RD_POLY_MULTILAUNCH") ? 0 : 1;      // (tests: the ~85-launch form for every frame)
  d->force_redo = (rd_env("RD_POLY_FORCE_REDO") ? 1 : 0) | (rd_env("RD_ABSORB_FORCE_SLOW") ? 2 : 0);   // tests: every frame also takes the polyline / absorption fallback
  // The single-block polyline kernel holds 16 384 live chain pixels; a 1920x1080 frame of the synthetic streams has ~11 000, frames of 3 megapixels and
  // more are beyond it as a rule: their streams start on the multi-launch form instead of overflowing - and being repeated - until the two-overflow rule
  // (slot_finish_device, rd_detector_poll_segments) finds that out (3840x2160: 12 of the first 16 frames).  Smaller frames that overflow anyway are still caught by that rule.
  d->poly_overflows = (long)iw * ih > 3000000L ? 1 : 0;
  d->batch = 1; d->deferred_slot = -1; d->last_polled_slot = -1;
  pthread_mutex_init(&d->tan_mu, NULL); pthread_cond_init(&d->tan_cv, NULL);
  pthread_mutex_init(&d->launch_mu, NULL);
  d->slots = (Slot *)calloc((size_t)nslots, sizeof(Slot));
  d->frames = (rdk::PolyFrame *)calloc((size_t)nslots, sizeof(rdk::PolyFrame));
  return d;
}

// streams, group mode, planes and slots, once the kind's own settings (fork_poly, batch) stand
static void detector_slots(rd_detector *d, int nstreams) {
  const int nslots = d->nslots;
  // One stream per frame: the frames beyond the fourth queue up behind earlier ones on the same four streams (slot i uses the
  // streams of slot i mod 4) - a stream of its own would be time-sliced onto the same four hardware queues and stall frames
  // that have nothing to do with each other, while a queued frame keeps its queue busy as soon as its predecessor is done
  // (the host's turn-around between "frame polled" and "next frame enqueued" otherwise idles a quarter of the device).
  d->nstreams = nstreams < nslots ? nstreams : nslots;
  // Group mode: four frames per launch from twelve frame slots on (three groups: one being filled, two in flight), two from six on, eight from 32 on
  // (640x480: 9100 frames/s with 16 slots in groups of four, 11700 with 32 in groups of eight; 1080p: no difference);
  // RD_ZBATCH=k overrides (k frames per launch, 2..8; 0 / 1: off).
  d->zb = nslots >= 32 ? 8 : (nslots >= 12 ? 4 : (nslots >= 6 ? 2 : 1));      // (always at least three or four groups: one being filled, the others in flight on the four streams)
  if ((long long)d->iw * d->ih > 1920ll * 1088) d->zb = 1;      // (launches of larger frames fill the device on their own: 3840x2160 measured 1 % slower in groups)
  if (rd_env("RD_ZBATCH")) { const int z = rd_env_int("RD_ZBATCH", 1); d->zb = z < 1 ? 1 : (z > RD_ZB_MAX ? RD_ZB_MAX : z); }
  if (d->fork_poly || d->zb > nslots) d->zb = 1;
  if (d->zb > 1) { d->batch = 1; d->defer = 0; }      // (a group's sparse stages follow its dense stages on the same stream)
  d->slot_pitch = slot_planes(d, NULL, NULL);
  d->arena = dnew<char>((size_t)nslots * d->slot_pitch);
  for (int i = 0; i < nslots; i++) {
    Slot *s = &d->slots[i];
    slot_alloc(d, s, (!d->fork_poly && i >= nstreams) ? &d->slots[i % nstreams] : NULL);
    s->owner = d;
    pthread_mutex_init(&s->mu, NULL); pthread_cond_init(&s->cv, NULL);
    if (d->nworkers > 0 && pthread_create(&s->th, NULL, slot_worker, s) != 0) exitf(-1, "rd_detector_create: cannot start worker thread\n");
  }
  if (d->kind == RD_KIND_RECT) rdk::quant_lut_init(d->slots[0].st);
  RD_HIP(hipDeviceSynchronize());
}

static void slot_destroy_graphs(Slot *s) {
  for (int g = 0; g < 2; g++) for (int k = 0; k < RD_NSEQ; k++) if (s->graphs[g][k]) { RD_HIP(hipGraphExecDestroy(s->graphs[g][k])); s->graphs[g][k] = NULL; }
}

extern "C" {

rd_detector *rd_detector_create(int device, int iw, int ih, int nslots, int nworkers) {
  if (rd_device_count() <= 0) exitf(-1, "rd_detector_create: no HIP device available - this library has no CPU path\n");
  if (iw < 16 || ih < 16) exitf(-1, "rd_detector_create: frame %dx%d too small\n", iw, ih);
  if ((long long)iw * ih >= (1ll << 25)) exitf(-1, "rd_detector_create: frame %dx%d too large (pixel indices are kept below 2^25: hash keys and marked label words rely on the spare bits)\n", iw, ih);
  if (nslots < 1) nslots = 1;
  rd_detector *d = detector_new(RD_KIND_RECT, device, iw, ih, nslots, nworkers);
  d->nring = nslots + 1;
  d->prev_ring = dnew<int8_t>((size_t)d->N * d->nring);
  RD_HIP(hipMemset(d->prev_ring, 0, (size_t)d->N * d->nring));
  // candidate funnel + pose estimation on the device (rd_k_post.hip) instead of on one worker thread per frame slot: RD_DEVICE_POST=0|1 decides;
  // otherwise the host path - 0.3 ms of CPU time per 1080p frame, i.e. 0.6 of a core at 2000 frames/s: measured 2050 frames/s on 8 cores
  // as on 256, against 1830 for the device path - unless this process may run on one or two cores only
  if (rd_env("RD_DEVICE_POST")) d->device_post = rd_env_int("RD_DEVICE_POST", 0) != 0;
  else {
    cpu_set_t set;
    const int ncpu = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 0;
    d->device_post = (nworkers > 0 && ncpu > 0 && ncpu <= 2) ? 1 : 0;
  }
  // The device runs four hardware queues side by side (more are time-sliced: measured 2x slower per frame).  With one or two
  // frames in flight a frame spreads over two streams (polyline chain beside the blur chain: shortest latency); from three
  // frames on every frame keeps to one stream, so that four frames occupy the four queues (highest throughput).
  d->fork_poly = nslots <= 2 ? 1 : 0;
  if (RD_LAB_INT("RD_FORK_POLY", 1) == 0) d->fork_poly = 0;      // (measurements: one stream per frame with one or two in flight as well)
  // One or two frames in flight and no worker threads = the reference's call sequence (executeOnce, enqueueTask / pollTask): the caller's thread runs the
  // post-process at the end of every frame's latency; helper threads share its pose estimations (rd_post.c), RD_POST_HELPERS=n overrides their number
  d->post_helpers = 0;
  if (nworkers == 0 && nslots <= 2) {
    cpu_set_t set;
    const int ncpu = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 0;
    d->post_helpers = rd_env_int("RD_POST_HELPERS", ncpu >= 16 ? 4 : (ncpu >= 8 ? 2 : (ncpu >= 4 ? 1 : 0)));      // (1 / 3 / 5 / 7 helpers: 1.19 / 1.14-1.20 / 1.11 / 1.12-1.20 ms per executeOnce against 1.28 without)
    if (d->post_helpers > 0) rd_post_helpers_configure(d->post_helpers);
  }
  // round budget of the region merge: what the last 64 frames needed + margin (8 / 12 / 16 / 20 launched rounds; the rounds after
  // the merge has settled are no-ops, but each still costs two launches of a thousand blocks), frames that turn out to need more
  // are repeated with all 20; RD_REGION_ROUNDS_FIXED=8|12|16|20 pins the budget (20: never repeat anything).
  d->fixed_rounds = 0;
  if (rd_env("RD_REGION_ROUNDS_FIXED")) { const int r = rd_env_int("RD_REGION_ROUNDS_FIXED", 20); d->fixed_rounds = (r >= 8 && r <= 20 && !(r & 1)) ? r : 20; }
  d->rounds_budget = 20;
  d->t_edge = 500; d->t_strong = 2500;      // oclrect.c:277-284, 307-313
  if (rd_env("RD_TEST_THRESHOLDS")) {      // tests only: other thresholds, so that many strength sums stand exactly one below one (where the mask of the frame before decides, H1)
    int a = 0, b = 0;
    if (sscanf(rd_env("RD_TEST_THRESHOLDS"), "%d,%d", &a, &b) == 2 && a > 0 && b >= a) { d->t_edge = a; d->t_strong = b; }
  }
  d->strong_by_frame = rd_env("RD_STRONG_BY_FRAME") ? 1 : 0;
  d->budget_cycle = rd_env_int("RD_BUDGET_CYCLE", 0);      // tests: the launch budget changes every so many frames (12, 14, .. 20, 12, ..)
  // frames per set of sparse-stage launches: 4 from twelve frames in flight on - the deferral by one group below needs a third group of
  // slots to keep the streams fed, and without it a batch is a barrier per group (measured 10 % slower than no batching) - else every
  // frame on its own; RD_BATCH=1..4 overrides (tests: batching with any slot count)
  d->batch = nslots >= 24 ? 8 : (nslots >= 12 ? 4 : 1);      // (these stages are latency-bound chains of gathers: eight frames take a launch as long as four)
  if (rd_env("RD_BATCH")) { const int b = rd_env_int("RD_BATCH", 1); d->batch = b < 1 ? 1 : (b > RD_MAXB ? RD_MAXB : b); }
  if (d->fork_poly || d->batch > nslots) d->batch = d->fork_poly ? 1 : nslots;
  d->defer = (d->batch > 1 && nslots >= 3 * d->batch) ? 1 : 0;       // needs a third group of slots to keep the streams fed meanwhile
  const int nstreams = RD_LAB_INT("RD_NSTREAMS", 4) < 1 ? 1 : (RD_LAB_INT("RD_NSTREAMS", 4) > 8 ? 8 : RD_LAB_INT("RD_NSTREAMS", 4));      // (measurements only - 3 / 5 / 6 streams: 2776-2786 / 2746-2753 / 2827-2847 frames/s against 2881-2889 with four, one box)
  detector_slots(d, nstreams);
  return d;
}

void rd_detector_destroy(rd_detector *d) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_destroy: bad handle\n");
  RD_HIP(hipSetDevice(d->device));
  RD_HIP(hipDeviceSynchronize());
  for (int i = d->nslots - 1; i >= 0; i--) {      // (slots that borrowed streams go before the slots that own them)
    Slot *s = &d->slots[i];
    if (d->nworkers > 0) {
      pthread_mutex_lock(&s->mu); s->quit = 1; pthread_cond_broadcast(&s->cv); pthread_mutex_unlock(&s->mu);
      pthread_mutex_lock(&d->tan_mu); pthread_cond_broadcast(&d->tan_cv); pthread_mutex_unlock(&d->tan_mu);
      pthread_join(s->th, NULL);
    }
    free(s->result); free(s->res_segs);
    slot_destroy_graphs(s);
    slot_free(s, d->device);
  }
  if (d->st_upload) { RD_HIP(hipStreamSynchronize(d->st_upload)); unpool_stream(d->device, d->st_upload); }
  free(d->slots);
  free(d->frames);
  dfree(d->prev_ring);
  dfree(d->arena);
  free(d->last_segs);
  d->magic = 0;
  free(d);
}

// The reference hands the aperture over with the poll, i.e. after the frame (oclrect_pollTask); whatever runs ahead of the poll - the
// worker threads' post-process, the rectangles on the device - uses the last one seen.  A caller that knows it beforehand says so here,
// and the first frames of a stream are treated like all later ones.
void rd_detector_set_aperture(rd_detector *d, double tanAOV) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_set_aperture: bad handle\n");
  pthread_mutex_lock(&d->tan_mu);
  d->tan_aov = tanAOV; d->have_tan = 1;
  pthread_cond_broadcast(&d->tan_cv);
  pthread_mutex_unlock(&d->tan_mu);
}

long rd_detector_counter(rd_detector *d, int which) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_counter: bad handle\n");
  if (which >= RD_CTR_BUDGET_FRAMES && which < RD_CTR_BUDGET_FRAMES + RD_NBUDGETS) return d->budget_count[which - RD_CTR_BUDGET_FRAMES];
  if (which >= RD_CTR_NEED_FRAMES && which <= RD_CTR_NEED_FRAMES + 20) return d->need_count[which - RD_CTR_NEED_FRAMES];
  switch (which) {      // (what each counts: include/rectdetect_hip.h, enum rd_counter)
  case RD_CTR_POLY_REDONE: return __atomic_load_n(&d->n_redo, __ATOMIC_RELAXED);
  case RD_CTR_DEVICE_US: return d->dev_us;
  case RD_CTR_DEVICE_FRAMES: return d->dev_frames;
  case RD_CTR_ENQUEUE_US: return d->host_enqueue_ns / 1000;
  case RD_CTR_REGION_REDONE: return __atomic_load_n(&d->n_redo_rounds, __ATOMIC_RELAXED);
  case RD_CTR_REGION_BUDGET: return __atomic_load_n(&d->rounds_budget, __ATOMIC_RELAXED);
  case RD_CTR_REGION_UNSETTLED: return __atomic_load_n(&d->n_unsettled, __ATOMIC_RELAXED);
  case RD_CTR_PROBES_REGROWN: return __atomic_load_n(&d->n_truncated, __ATOMIC_RELAXED);
  case RD_CTR_POST_DEVICE: return __atomic_load_n(&d->n_post_device, __ATOMIC_RELAXED);
  case RD_CTR_POST_HOST: return __atomic_load_n(&d->n_post_host, __ATOMIC_RELAXED);
  case RD_CTR_POST_HOST_US: return __atomic_load_n(&d->host_post_ns, __ATOMIC_RELAXED) / 1000;
  case RD_CTR_ABSORB_SLOW: return __atomic_load_n(&d->n_redo_absorb, __ATOMIC_RELAXED);
  case RD_CTR_FRAMES_PER_LAUNCH: return d->zb;
  case RD_CTR_STRONG_ONE_LAUNCH: return d->n_strong_group;
  case RD_CTR_STRONG_BY_FRAME: return d->n_strong_by_frame;
  case RD_CTR_FRAMES_PINNED: return d->n_frames_pinned;
  case RD_CTR_FRAMES_COPIED: return d->n_frames_copied;
  case RD_CTR_LONG_LISTS: return __atomic_load_n(&d->n_long_lists, __ATOMIC_RELAXED);
  case RD_CTR_SLOT_BYTES: return (long)d->slot_pitch;      // (the way the slots are carved: every plane rounded up to 256 bytes)
  case RD_CTR_HANDOFF_RECORDS: return d->kind == RD_KIND_POLY ? d->handoff_rec : RD_MAXREC;
  case RD_CTR_SCALED_STAGING_BYTES: { size_t b = 0; for (int i = 0; i < d->nslots; i++) if (d->slots[i].sc_bgr && d->slots[i].sc_bytes > b) b = d->slots[i].sc_bytes; return (long)b; }
  }
  return -1;
}

int rd_detector_last_segments(rd_detector *d, void *dst, int max_records) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_last_segments: bad handle\n");
  if (!d->last_segs) return -1;
  int m = d->last_nsegs + 1 < max_records ? d->last_nsegs + 1 : max_records;
  if (dst && m > 0) memcpy(dst, d->last_segs, (size_t)m * 56);
  return d->last_nsegs;
}

// A plane kept as bits on the device (ceil(iw / 64) words per row), handed out as an int plane.  junction: not the bits but the junction counts
// (oclrect.cl:74-95: on-pixels of the 3x3 block, 1 -> 0, frame border 0) evaluated from them.
static size_t bit_plane_as_ints(rd_detector *d, const void *bits, int junction, void *dst, size_t max_bytes) {
  const size_t n = (size_t)d->N * 4 <= max_bytes ? (size_t)d->N : max_bytes / 4;
  const int wpr = (d->iw + 63) / 64, iw = d->iw, ih = d->ih;
  unsigned long long *tmp = (unsigned long long *)malloc((size_t)wpr * ih * 8 + 8);
  if (!tmp) exitf(-1, "rd_detector_debug_plane: out of memory\n");
  RD_HIP(hipMemcpy(tmp, bits, (size_t)wpr * ih * 8, hipMemcpyDeviceToHost));
  auto bit = [&](int x, int y) { return (int)((tmp[(size_t)y * wpr + (x >> 6)] >> (x & 63)) & 1ull); };
  for (size_t k = 0; k < n; k++) {
    const int y = (int)(k / iw), x = (int)(k % iw);
    int v = bit(x, y);
    if (junction) {
      if (v && x > 0 && y > 0 && x < iw - 1 && y < ih - 1) { int c = 0; for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) c += bit(x + dx, y + dy); v = c == 1 ? 0 : c; }
      else v = 0;
    }
    ((int *)dst)[k] = v;
  }
  free(tmp);
  return n * 4;
}
// The debug planes of both kinds: the one table of them (include/rectdetect_hip.h lists the names).  A row: name, kinds, plane + byte offset, `bytes`, how the plane is
// viewed, what has to be launched before it can be looked at.  `bytes` is what the CALLER gets when max_bytes is ample, not what lies at the pointer: the rows of the int
// views say N * 4 where the device holds N bytes (edge500) or a bit plane (strong, junction, mergemask, polymask); a raw row's two sizes are the same.
enum { VIEW_RAW,          // as stored; a shorter buffer gets min(bytes, max_bytes)
       // int views - kept in another shape on the device, handed out as the reference's int planes; a shorter buffer gets max_bytes / 4 elements:
       VIEW_BITS,         // a bit plane (what the polyline stage traces / what the region stage reads; oclrect.c:307-321, poly.cpp:121)
       VIEW_JUNCTION,     // the junction counts evaluated from a bit plane
       VIEW_POSITIVE,     // `> 0` of a float plane (rect kind's mask0, oclrect.c:262-264: not stored on the frame path, derived from the suppressed strength)
       VIEW_INT8,         // bytes (the blur's mask; oclrect.c:277-284)
       VIEW_STRSUM };     // raw + the strong mask the frame read: the reference's plane holds the sums ON TOP of the previous frame's strong mask (H1)
enum { PREP_NONE,
       PREP_IDS,          // polyline_ids: the id plane is not part of the frame path, it is built from the compact state
       PREP_FLATTEN,      // a -DRD_BOUNDARY_FLATTEN=0 build leaves the boundary components as a forest (its few readers walk): flattened here, where the plane is looked at
       PREP_TAPS };       // plab1, vxy, strength never leave the chip where the front is fused: the same kernel again, writing them out (the blurred planes are intact)
size_t rd_detector_debug_plane(rd_detector *d, const char *name, void *dst, size_t max_bytes) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_debug_plane: bad handle\n");
  if (d->last_polled_slot < 0) return 0;
  RD_HIP(hipSetDevice(d->device));
  Slot *s = &d->slots[d->last_polled_slot];
  const size_t N = (size_t)d->N, NI = N * 4;
  const int kind = d->kind == RD_KIND_POLY ? PK_POLY : PK_RECT;
  const struct { const char *n; int kinds; const void *p; size_t off, bytes; int view, prep; } tab[] = {
    { "plab0", PK_BOTH, s->plab0, 0, NI, VIEW_RAW, PREP_NONE }, { "plab1", PK_RECT, s->plab1, 0, NI, VIEW_RAW, PREP_TAPS }, { "lblur", PK_BOTH, s->bl[0], 0, NI, VIEW_RAW, PREP_NONE },
    { "vxy", PK_RECT, s->vxy, 0, N * 8, VIEW_RAW, PREP_TAPS }, { "strength", PK_RECT, s->strength, 0, NI, VIEW_RAW, PREP_TAPS }, { "nms", PK_BOTH, s->nms, 0, NI, VIEW_RAW, PREP_NONE },
    { "mask0", PK_RECT, s->nms, 0, NI, VIEW_POSITIVE, PREP_NONE }, { "mask0", PK_POLY, s->mask0, 0, NI, VIEW_RAW, PREP_NONE }, { "tidy", PK_RECT, s->tidy, 0, NI, VIEW_RAW, PREP_NONE },
    { "label1", PK_BOTH, s->label1, 0, NI, VIEW_RAW, PREP_NONE }, { "strsum", PK_RECT, s->strsum, 0, NI, VIEW_STRSUM, PREP_NONE }, { "strsum", PK_POLY, s->strsum, 0, NI, VIEW_RAW, PREP_NONE },
    { "edge500", PK_RECT, s->e8, 0, NI, VIEW_INT8, PREP_NONE }, { "smooth", PK_RECT, s->smooth, 0, NI, VIEW_RAW, PREP_NONE }, { "quant", PK_RECT, s->quant, 0, NI, VIEW_RAW, PREP_NONE },
    { "strong", PK_RECT, s->strongbits, 0, NI, VIEW_BITS, PREP_NONE }, { "junction", PK_RECT, s->strongbits, 0, NI, VIEW_JUNCTION, PREP_NONE }, { "mergemask", PK_RECT, s->mmbits, 0, NI, VIEW_BITS, PREP_NONE },
    { "polymask", PK_POLY, s->strongbits, 0, NI, VIEW_BITS, PREP_NONE },
    { "region", PK_RECT, s->region, 0, NI, VIEW_RAW, PREP_NONE }, { "region0", PK_RECT, s->region0, 0, NI, VIEW_RAW, PREP_NONE }, { "rsize", PK_RECT, s->rsize, 0, NI, VIEW_RAW, PREP_NONE },
    { "boundarysrc", PK_RECT, s->boundarysrc, 0, NI, VIEW_RAW, PREP_NONE }, { "boundary", PK_RECT, s->boundary, 0, NI, VIEW_RAW, PREP_FLATTEN }, { "lsid", PK_BOTH, s->lsid, 0, NI, VIEW_RAW, PREP_IDS },
    { "table", PK_RECT, s->table, 0, (N * 4 / 5) * 5 * 4, VIEW_RAW, PREP_NONE }, { "lslist", PK_BOTH, s->lslist, 0, N * 16, VIEW_RAW, PREP_NONE },
    { "polyctr", PK_BOTH, rdk::poly_scratch_counters(s->ps), 0, 64 * 4, VIEW_RAW, PREP_NONE }, { "iirflags", PK_RECT, s->flags, 0, 16 * 4, VIEW_RAW, PREP_NONE },
    { "d2work", PK_RECT, s->d2s, NI, 16 * 4, VIEW_RAW, PREP_NONE }, { "absorb", PK_RECT, s->scratch2, (N + RD_REGION_STATUS_AT) * 4, 8 * 4, VIEW_RAW, PREP_NONE },
  };
  for (const auto &r : tab) {
    if (!(r.kinds & kind) || strcmp(r.n, name)) continue;
    const char *p = (const char *)r.p + r.off;
    // (launches of a test tap: under the lock that keeps launches out of another thread's graph capture)
    pthread_mutex_lock(&d->launch_mu);
    if (r.prep == PREP_IDS) rdk::polyline_ids(s->st, s->frame, 1, (int)N);
    if (r.prep == PREP_FLATTEN && !RD_BOUNDARY_FLATTEN) rdk::label8_flatten(s->st, s->boundary, (int)N);
    if (r.prep == PREP_TAPS && front_is_fused(d)) frames_grad_nms(d, s, s->st, 1, 0, 1);
    if (r.prep != PREP_NONE) rdrt::check_launch("debug plane");
    pthread_mutex_unlock(&d->launch_mu);
    RD_HIP(hipStreamSynchronize(s->st));
    if (r.view == VIEW_BITS || r.view == VIEW_JUNCTION) return bit_plane_as_ints(d, p, r.view == VIEW_JUNCTION, dst, max_bytes);
    if (r.view == VIEW_POSITIVE || r.view == VIEW_INT8) {
      const size_t n = NI <= max_bytes ? N : max_bytes / 4, eb = r.view == VIEW_INT8 ? 1 : 4;
      void *tmp = malloc(n ? n * eb : 4);
      if (!tmp) exitf(-1, "rd_detector_debug_plane: out of memory\n");
      RD_HIP(hipMemcpy(tmp, p, n * eb, hipMemcpyDeviceToHost));
      for (size_t k = 0; k < n; k++) ((int *)dst)[k] = r.view == VIEW_INT8 ? ((const int8_t *)tmp)[k] : (((const float *)tmp)[k] > 0.0f ? 1 : 0);
      free(tmp);
      return n * 4;
    }
    const size_t b = r.bytes < max_bytes ? r.bytes : max_bytes;
    RD_HIP(hipMemcpy(dst, p, b, hipMemcpyDeviceToHost));
    if (r.view == VIEW_STRSUM && s->prev_in) {
      const size_t n = b / 4;
      int8_t *tmp = (int8_t *)malloc(n ? n : 1);
      RD_HIP(hipMemcpy(tmp, s->prev_in, n, hipMemcpyDeviceToHost));
      for (size_t k = 0; k < n; k++) ((int *)dst)[k] += tmp[k];
      free(tmp);
    }
    return b;
  }
  return 0;
}

// ---- the polyline kind
rd_detector *rd_polyline_detector_create(int device, int iw, int ih, int nslots, int strength_thre, float minerror, int size_thre) {
  if (iw < 16 || ih < 16 || (long long)iw * ih >= (1ll << 25) || nslots < 1 || device < 0 || strength_thre < 0 || !(minerror > 0.0f) || size_thre < 0) return NULL;
  if (rd_device_count() <= 0) exitf(-1, "rd_polyline_detector_create: no HIP device available - this library has no CPU path\n");
  if (device >= rd_device_count()) return NULL;
  rd_detector *d = detector_new(RD_KIND_POLY, device, iw, ih, nslots, 0);
  d->p_thre = strength_thre; d->p_minerror = minerror; d->p_size = size_thre;
  d->handoff_rec = RD_POLY_HANDOFF_DEFAULT;
  { const int h = rd_env_int("RD_POLY_HANDOFF", 0); if (h >= 2) d->handoff_rec = h; }      // (tests: a small block, so that ordinary frames take the long-list path)
  detector_slots(d, 4);      // (streams and group launches as the rect kind's; no second stream per frame, no batches, no rectangles: fork_poly, defer and device_post stay 0)
  return d;
}

// ================================================================================================ oclrect (reference API)
struct oclrect_t { uint32_t magic; rd_detector *det; int iw, ih; };

struct oclrect_t *init_oclrect(struct oclimgutil_t *oclimgutil, struct oclpolyline_t *oclpolyline, cl_device_id device, cl_context context, cl_command_queue queue, int iw, int ih) {
  (void)oclimgutil; (void)oclpolyline; (void)context; (void)queue;
  struct oclrect_t *t = (struct oclrect_t *)calloc(1, sizeof(*t));
  t->magic = MAGIC_RECT; t->iw = iw; t->ih = ih;
  t->det = rd_detector_create(device ? device->ordinal : rdrt::current_device(), iw, ih, 2, RD_LAB_INT("RD_API_WORKERS", 0));   // two pages like oclrect.c:54
  return t;
}

void dispose_oclrect(struct oclrect_t *t) {
  if (!t || t->magic != MAGIC_RECT) exitf(-1, "dispose_oclrect: bad handle\n");
  rd_detector_destroy(t->det);
  t->magic = 0;
  free(t);
}

rect_t *oclrect_executeOnce(struct oclrect_t *t, uint8_t *imgData, int ws, const double tanAOV) {
  if (!t || t->magic != MAGIC_RECT) exitf(-1, "oclrect_executeOnce: bad handle\n");
  if (t->det->next_enqueue != t->det->next_poll) exitf(-1, "oclrect_executeOnce: a task is still pending (poll it first)\n");
  rd_detector_enqueue(t->det, imgData, ws, 0);
  return (rect_t *)rd_detector_poll(t->det, tanAOV);
}

void oclrect_enqueueTask(struct oclrect_t *t, uint8_t *imgData, int ws) {
  if (!t || t->magic != MAGIC_RECT) exitf(-1, "oclrect_enqueueTask: bad handle\n");
  rd_detector_enqueue(t->det, imgData, ws, 0);
}

rect_t *oclrect_pollTask(struct oclrect_t *t, const double tanAOV) {
  if (!t || t->magic != MAGIC_RECT) exitf(-1, "oclrect_pollTask: bad handle\n");
  return (rect_t *)rd_detector_poll(t->det, tanAOV);
}

}  // extern "C"
