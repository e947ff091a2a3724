// rectdetect-mi355x: what the units of the detector runtime share - rd_detector.hip (the objects: slots, planes, streams, create / destroy, counters, debug planes),
// rd_frames.hip (everything a frame passes through between its enqueue and the return of its poll), rd_taps.hip (the stages' test taps) and, for the device
// allocator and the handle magics alone, rd_ops.hip (the operator API).  A function that only one of them uses is static there and not named here.
#pragma once
#include "rd_internal.h"
#include "rd_kernels.h"
#include "rd_poly_scratch.h"
#include "rectdetect_hip.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>

extern "C" {
#include "vec234.h"
#include "oclrect.h"
}

// Environment switches.  A detector reads the ones include/rectdetect_hip.h lists ("Environment") when it is created - its behaviour never changes afterwards, and two
// detectors of one process may differ.  The switches of experiments whose variant was measured and NOT kept (profiles/NOTES_r0*.md) exist in tuning builds only
// (-DRD_TUNING, tools/variants.sh): in the product they are the constants below.
static inline const char *rd_env(const char *name) { const char *v = getenv(name); return (v && *v) ? v : NULL; }
static inline int rd_env_int(const char *name, int dflt) { const char *v = rd_env(name); return v ? atoi(v) : dflt; }
#ifdef RD_TUNING
#define RD_LAB_INT(name, dflt) rd_env_int(name, dflt)
#else
#define RD_LAB_INT(name, dflt) (dflt)
#endif

#define MAGIC_IMGUTIL 0xa640d893u
#define MAGIC_POLYLINE 0x808f3801u
#define MAGIC_RECT 0x808f3802u

template <typename T> static T *dnew(size_t n) { void *p = NULL; RD_HIP(hipMalloc(&p, (n ? n : 1) * sizeof(T))); return (T *)p; }
static inline void dfree(void *p) { if (p) RD_HIP(hipFree(p)); }

#define RD_NBUDGETS 7       // launch budgets of the region merge: 8, 10, .. 20 (kRoundBudgets)
#define RD_NSEQ (1 + 2 * RD_NBUDGETS)      // captured launch sequences of a frame or a group (Slot::graphs)
#define RD_MAXREC 512       // records copied back per frame without a second transfer (the copy runs at PCIe speed: 16 us for 2048)

struct Slot {
  hipStream_t st;
  hipStream_t st2;                        // second stream of the slot: polyline stage, parallel to the region stages
  int pooled_streams;                     // st / st2 come from the process-wide pool of high-priority streams and go back there
  int shares_streams;                     // st / st2 belong to another slot (see rd_detector_create)
  hipEvent_t ev_fork, ev_mm, ev_join;
  hipEvent_t ev_begin, ev_done, ev_strong;   // ev_begin/ev_done carry timestamps: device time of the frame (rd_detector_counter)
  hipEvent_t watch_begin, watch_done;        // the events that bracket the frame in flight: the slot's own, or - a frame of a group launch - the ones of the group's first slot
  hipEvent_t ev_redo;                        // end of a repeated part of the frame (slot_finish_device)
  hipEvent_t ev_upload;                      // one or two frames in flight: the copy engine has read a host frame it took straight from the caller's pinned buffer
  hipStream_t st_redo;                       // created on first use: the slow absorption path (frame_absorb_slow), fetches of long lists
  int *big_probes; int big_probes_cap;       // probes of a frame with more segments than `probes` holds (grows on demand)
  const int8_t *prev_in;                  // the strong mask this slot's frame read (plane of rd_detector::prev_ring)
  uint8_t *bgr;
  const uint8_t *src;                     // where the frame in flight is read from: bgr (uploaded) or the caller's device buffer
  uint32_t *plab0, *plab1, *smooth, *quant;
  float *tr[3], *fw[3], *bw[3], *hz[3], *bl[3], *vxy, *strength, *nms;
  int *i0, *i1, *mask0, *tidy, *label1, *strsum, *region, *rsize, *scratch2, *d2s, *boundarysrc, *boundary, *lsid, *table, *claim, *probes, *region0, *tlist;
  int8_t *e8;
  unsigned long long *mmbits;             // the merge mask (oclrect.c:315-321) as a bit plane
  unsigned long long *strongbits;         // this frame's strong mask as a bit plane (ceil(iw / 64) words per row): what the polyline stage traces
  uint16_t *ext;
  float *tails; int *flags;
  void *lslist;
  rdk::PolyScratch *ps;
  rdk::PolyFrame *frame;                  // this slot's descriptor for the sparse stages (element `slot index` of the detector's array)
  hipEvent_t ev_dense;                    // batched mode: the frame's dense stages are done (the batch's sparse stages wait for it)
  int pending_sparse;                     // batched mode: dense stages enqueued, sparse stages not launched yet
  int pending_dense;                      // group mode (rd_detector::zb > 1): frame handed over, nothing launched yet
  int group_n;                            // frames that ran between this frame's ev_begin and ev_done (1, or the group's size: the interval is shared)
  // rectangles on the device (RD_DEVICE_POST): scratch, result block in pinned host memory, whether this frame's block is valid and for which aperture
  int *post_scratch, *h_post, *h_post_dev;
  int post_mode; double post_tan;
  // host side
  void *h_bgr;            // pinned staging for host frames
  void *h_segs; int *h_probes; int *h_ctr;   // views into h_pack
  int *h_pack, *h_pack_dev;                // everything the host needs from a frame, assembled by the device in pinned host memory (host / device address)
  long seq;
  int ws;
  // the frame's pixel format (RD_PIX_*), its planes and their row strides (hand_over); src = pl[0] and ws = pitch[0]; a host frame's planes are packed into bgr
  int fmt;
  const uint8_t *pl[3]; int pitch[3];
  // rd_detector_enqueue_scaled: 1, or 2 - the planes hold a frame of 2 iw x 2 ih pixels, which the front kernel averages 2x2 as it reads.  A host frame of that size
  // (up to 16 bytes per detector pixel) does not fit bgr / h_bgr: it travels through a pair of staging buffers of its own, which a slot gets with its first such frame
  int scale;
  uint8_t *sc_bgr; void *sc_h; size_t sc_bytes;
  // Captured launch sequences: [0] this slot's frame on its own, [1] the group this slot leads (group mode); by sequence - 0: the dense stages up to the first
  // labelling, 1 + 2 * round budget index + polyline mode: everything after the strong masks (the polyline kind's one sequence: 1 + polyline mode).  None reads the
  // frame (the colour conversion runs in front of them, outside), so a change of format or row stride re-captures nothing.
  hipGraphExec_t graphs[2][RD_NSEQ];
  int poly_mode;                          // polyline mode of the frame in flight (1 = single block, 0 = multi-launch)
  int rounds;                             // region-merge round budget of the frame in flight
  // post-process worker
  pthread_t th; pthread_mutex_t mu; pthread_cond_t cv;
  int state;              // 0 idle, 1 submitted to the GPU, 2 result ready
  int quit;
  void *result; double result_tan; void *res_segs; int res_nsegs;
  struct rd_detector *owner;
};

struct rd_detector {
  uint32_t magic;
  int device, iw, ih, N, nslots, nworkers, maxrec_dev;
  // Sparse stages (polylines, votes, probes) of `batch` consecutive frame slots run as ONE set of launches (frame = blockIdx.z): they
  // are a chain of 20-odd latency-bound launches that keeps a hardware queue busy for ~0.4 ms without filling the chip, per
  // batch instead of per frame.  Slots [g * batch, (g + 1) * batch) form group g; 1 = every frame on its own (shortest latency).
  int batch; unsigned sparse_rot;
  int device_post;                        // candidate funnel + pose estimation on the device (rd_k_post.hip) instead of the host worker threads
  long n_post_device, n_post_host, host_post_ns;
  int defer, deferred_slot;               // batched mode: a complete group's sparse stages are launched only once the NEXT group's dense stages are enqueued (deferred_slot: a slot of the waiting group or -1)
  rdk::PolyFrame *frames;                 // nslots descriptors (host memory; they travel as kernel arguments), slot order
  Slot *slots;
  int nstreams;
  int zb;                 // frames per launch of the DENSE stages as well (groups of zb consecutive slots, frame = blockIdx.z): small frames, whose launches do not fill the device
  char *arena; size_t slot_pitch;      // all slots' planes in one allocation, slot k at arena + k * slot_pitch (kSlotPlanes; rd_detector_counter 31: the pitch)
  // strong-edge masks of the last frames (reference quirk H1: a frame's strength sums start from the mask of the frame before), one byte per
  // pixel: a ring of nslots + 1 planes - frame t reads plane t mod (nslots + 1) and writes the next one, so what a frame read stays intact as
  // long as its slot's planes do (debug plane "strsum")
  int8_t *prev_ring; int nring;
  int t_edge, t_strong;                   // thresholds of the strength sums (500, 2500; RD_TEST_THRESHOLDS)
  int strong_by_frame;                    // tests (RD_STRONG_BY_FRAME): the strong masks of a group frame by frame instead of in one launch
  long n_strong_group, n_strong_by_frame; // groups whose strong masks took one launch / one launch per frame (rd_detector_counter 16 / 17)
  hipEvent_t last_strong; int have_last_strong;
  long next_enqueue, next_poll;
  long done_seq;                          // one more than the highest sequence number whose device work a worker has seen finished
  int last_polled_slot;
  void *last_segs; int last_nsegs;
  int use_graph, poly_mode, force_redo, fork_poly, fixed_rounds, budget_cycle; long n_redo, n_redo_rounds, n_redo_absorb;
  int overflow_streak;
  int poly_overflows;                     // set once two frames in a row overflowed the single-launch polyline kernel: later frames go multi-launch
  int rounds_budget, need_hist[64]; unsigned need_pos; long budget_count[RD_NBUDGETS], need_count[21];
  hipStream_t st_upload;     // group mode, host frames: the stream the frames travel on (created on first use, from the pool of high-priority streams)
  int post_helpers;          // helper threads armed by every poll (rd_post.c), 0 = none
  long host_enqueue_ns;      // wall time the caller spent inside rd_detector_enqueue
  long dev_us, dev_frames;   // sum over polled frames of (last kernel end - first kernel start) on the frame's stream, HIP events
  double tan_aov; int have_tan;    // what the workers use ahead of the poll that asks for the result
  pthread_mutex_t tan_mu; pthread_cond_t tan_cv;
  // Slots share streams (slot i uses the streams of slot i mod 4) and a worker thread may repeat part of its slot's frame on such a
  // stream while the enqueueing thread captures another slot's launch sequence on it: a capture would record the foreign launches, and
  // a stream that is capturing must not be synchronised.  launch_mu serialises captures against the launches of a repeat; repeats wait
  // on an event of their own (ev_redo), never on the stream.
  pthread_mutex_t launch_mu;
  const void *pinned[4][2]; unsigned pinned_next;   // the last 4 ranges of caller memory that were verified to be pinned host memory (RD_FRAME_HOST_PINNED; a frame's planes may lie in allocations of their own)
  const void *probed[2]; int probed_pinned[2];      // RD_FRAME_HOST, one or two frames in flight: the last two frame pointers asked about (a loop alternates between its two pages) and the answer
  long n_frames_pinned, n_frames_copied;     // host frames that travelled straight from the caller's pinned memory / through the detector's own staging pages
  long n_unsettled;          // frames whose region merge was still changing after RD_REGION_MAX_LAUNCHES launches (none on any fixture)
  long n_truncated;          // frames with more segment records than the slots' probe buffers hold (maxrec_dev): probed again into a larger buffer
  // the polyline kind (rd_polyline_detector_create: poly.cpp / vidpoly.cpp per frame); a rectangle detector has kind RD_KIND_RECT and none of this
  int kind;
  int p_thre, p_size; float p_minerror;     // filterStrength threshold, sizeThre, minerror
  int handoff_rec;           // records (header included) each slot's pinned block receives at the end of a frame (RD_POLY_HANDOFF)
  long n_long_lists;         // frames whose list did not fit that block and was fetched by the poll (rd_detector_counter 30)
};
#define RD_KIND_RECT 0
#define RD_KIND_POLY 1

// ---- what crosses a seam (between the library's units only: hidden, so that the library exports what it exported as one unit)
#pragma GCC visibility push(hidden)
// rd_detector.hip, for the frame path: a stream of the process-wide high-priority pool (handed back by the detector's destroy); a slot's stream for repeats and fetches
hipStream_t pooled_stream(int device);
hipStream_t make_redo_stream();
// rd_frames.hip, for the detector's objects: a slot's worker thread (started with the slot); whether the fused front kernel covers the frame size (decides the polyline
// kind's planes) and the front's last stage with its taps (debug planes "plab1", "vxy", "strength")
void *slot_worker(void *arg);
bool front_is_fused(const rd_detector *d);
void frames_grad_nms(rd_detector *d, Slot *s, hipStream_t st, int nz, size_t zs, int taps = 0);
// rd_frames.hip, for the test taps: the list a poll returns from a result block of the device post-process
rect_t *post_block_rectangles(const int *h_post);

// The region stage (oclrect.c:325-342) on a set of planes: a slot's (the frame path) or the caller's (rd_region_planes_device).  All of N = iw * ih ints except where noted.
struct RegionPlanes {
  const int *quant; const unsigned long long *mmbits, *strongbits;      // in: quantised pixels, the merge mask and the strong mask as bit planes (ceil(iw / 64) words per row)
  int *region0, *rsize, *region;          // merged regions, their sizes by label, regions after the absorption of small ones
  int *scratch2, *d2s;                    // 3N + 256 ints (the merge's launch flags at [N], the absorption's status words at [N + RD_REGION_STATUS_AT]); RD_D2_SCRATCH_INTS(N)
  int *boundarysrc, *boundary;            // boundary marks, their components
  int *table, *claim, *tlist;             // the vote tables, whose previous entries the last launch undoes
};
// Regions with `launches` launches of the merge, their sizes, absorption of small ones, boundaries and boundary components of nz frames whose planes lie zs bytes apart.
// from_merge = 0: the second half alone - absorption and boundaries from region0 / rsize as they stand (the tap's stage 1; `launches` is not read).
void region_stage(hipStream_t st, const RegionPlanes &p, int iw, int ih, int launches, int nz, size_t zs, int from_merge = 1);
// The absorption the long way (status word != 0 after region_stage) and the boundaries again.  Its rounds synchronise st: not for a stream that is being captured.  Returns despeckle2_slow's launches of the rounds.
int region_absorb_slow(hipStream_t st, const RegionPlanes &p, int iw, int ih);
#pragma GCC visibility pop

// The ladder of a frame whose region merge was still changing in the last launch of its first budget: the region stages again with as many launches as it takes
// (32 first - the frames that exceed a budget of 12-14 need 13-20 as a rule, and every launch after the settling one still costs a dispatch of the whole grid -
// then 64, then the definition's limit of RD_REGION_MAX_LAUNCHES = 128: region_ladder_next).  still_after(budget) runs the stages with that budget and returns the
// flag of the budget's last launch.  The one decision of the frame path (slot_finish_device) and of the stage's test tap (rd_region_planes_device).
struct LadderEnd { int budget, settled; };      // the budget that was final; settled = 0: the frame keeps what RD_REGION_MAX_LAUNCHES launches made of it
template <typename F> static LadderEnd region_ladder(F still_after) {
  LadderEnd e = { 0, 0 };
  for (int budget = rdk::region_ladder_next(RD_REGION_FIRST_BUDGET); budget && !e.settled; budget = rdk::region_ladder_next(budget)) {
    e.budget = budget;
    e.settled = still_after(budget) == 0;
  }
  return e;
}
