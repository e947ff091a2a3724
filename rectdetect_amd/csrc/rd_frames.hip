// rectdetect-mi355x: everything a frame passes through between rd_detector_enqueue* and the return of its poll - the stage sequences and their captured graphs, group
// and batched launches, the hand-over of a frame with its upload, the end of a frame (repeats, rectangles, the worker threads), the polls and the services' entry
// points behind a poll.  One unit, so that the per-frame path (hand_over -> enqueue_launch -> launch_frames -> the segments; poll -> slot_finish_device ->
// slot_rectangles) stays open to the compiler's inlining.  The detector's objects: rd_detector.hip.
#include "rd_detector.h"
#include "rd_comp.h"
#include "rd_jobs.h"
#include <time.h>
#include <sched.h>

extern "C" {
#include "rd_post.h"
}

// The device part of one frame (reference oclrect.c:235-381), enqueued on the slot's stream in three segments: [0] up to
// the first labelling and [2] the rest, each captured into a hipGraph (frame_segment), and between them [1] the hand-over of the
// strong-edge mask to the next frame (quirk H1, needs an event wait before it and an event record after it: rect_frames).
// last part of a frame: polylines of the strong edges, votes, probes, transfers.  mode 1 uses the single-launch polyline
// stage, which reports frames that do not fit its on-chip tables in counter 25; slot_postprocess() then repeats this
// part with mode 0.  For the nb frames of consecutive slots whose descriptors start at `frames`.
static void frame_polyline(rd_detector *d, const rdk::PolyFrame *frames, int nb, hipStream_t st, int mode) {
  // frame ring of the bridging step is "non-zero" on this path (oclrect.c:361, H3); the dense id plane is only produced on request (debug plane)
  rdk::polyline(st, frames, nb, d->N * 16, 1, 4.0f, 20, d->iw, d->ih, mode);
}

// segment / boundary votes (oclrect.c:365-367) and the probes the host needs (oclrect.c:1066-1098) for nb consecutive slots.
// The block the host needs - counters + round flags, the first RD_MAXREC segment records, their probes - is assembled by the
// sampling kernel directly in pinned host memory (0.2 MB of posted writes; frames with more records fetch the rest on demand):
// no copy launch at the end of the frame.
// tables_are_clean: frame_regions() ran just before (its last kernel undoes the previous entries of the vote tables)
// with_post: also the rectangles on the device, for the aperture the caller polled with last (the reference hands the aperture over with
// the poll, after the frame: a frame polled with another one, or the first frames of a stream, are post-processed on the host)
static void frames_votes(rd_detector *d, const rdk::PolyFrame *frames, int nb, hipStream_t st, int tables_are_clean, int with_post, double tan_aov = 0.0) {
  const int nentry = d->N * 4 / 5;
  rdk::reduce_ls(st, frames, nb, d->iw, d->ih, nentry, tables_are_clean);
  rdk::sample_segments(st, frames, nb, d->maxrec_dev, d->iw, d->ih, nentry, RD_MAXREC);
  if (with_post) rdk::post_device(st, frames, nb, d->maxrec_dev, d->iw, d->ih, tan_aov);      // (the caller's snapshot of the aperture: what the frames are labelled with)
}
// the aperture the device post-process of frames launched now runs with (set by polls and rd_detector_set_aperture, possibly on another thread)
static int aperture_snapshot(rd_detector *d, double *tan_out) {
  pthread_mutex_lock(&d->tan_mu);
  const int have = d->have_tan; *tan_out = d->tan_aov;
  pthread_mutex_unlock(&d->tan_mu);
  return have;
}

static void frame_tail(rd_detector *d, Slot *s, int mode) {   // both, in order, on the slot's main stream (overflow redo)
  frame_polyline(d, s->frame, 1, s->st, mode);
  frames_votes(d, s->frame, 1, s->st, 0, 0);
}

// The region stage's launches (rd_detector.h): the ONE list of them, for a frame, a group, a repeat and the stage's test tap (rd_region_planes_device).
void region_stage(hipStream_t st, const RegionPlanes &p, int iw, int ih, int launches, int nz, size_t zs, int from_merge) {
  const int N = iw * ih;
  if (from_merge) {      // regions (oclrect.c:325-336)
    int marked = 0;
    rdk::region_merge(st, p.region0, p.scratch2, p.quant, p.mmbits, p.strongbits, iw, ih, launches,
                      p.rsize, &marked, nz, zs);   // H2: the sizes start from the junction counts (evaluated by the first kernel)
    rdk::region_size(st, p.rsize, p.region0, N, p.d2s + N, marked, nz, zs);      // (also strips the rounds' marks from the labels, and clears the absorption's count)
  }
  rdk::despeckle2(st, p.region, p.region0, p.d2s, p.rsize, RD_ABSORB_THRE, iw, ih, from_merge ? 1 : 0, p.scratch2 + N + RD_REGION_STATUS_AT, nz, zs);   // (status words: they travel to the host with the round flags)
  // region boundaries and their components (oclrect.c:340-342)
  rdk::label8_boundary(st, p.boundary, p.boundarysrc, p.region, iw, ih, p.table, p.claim, p.tlist, nz, zs, RD_BOUNDARY_FLATTEN);   // (also undoes the previous frame's vote-table entries)
}
int region_absorb_slow(hipStream_t st, const RegionPlanes &p, int iw, int ih) {
  const int launches = rdk::despeckle2_slow(st, p.region, p.region0, p.d2s, p.rsize, RD_ABSORB_THRE, iw, ih);
  rdk::label8_boundary(st, p.boundary, p.boundarysrc, p.region, iw, ih, p.table, p.claim, p.tlist, 1, 0, RD_BOUNDARY_FLATTEN);
  return launches;
}

static RegionPlanes slot_region_planes(const Slot *s) {
  return { (const int *)s->quant, s->mmbits, s->strongbits, s->region0, s->rsize, s->region, s->scratch2, s->d2s, s->boundarysrc, s->boundary, s->table, s->claim, s->tlist };
}
// regions, their sizes, absorption of small ones, boundaries and boundary components (oclrect.c:325-342) of nz frames.  Reads planes that
// nothing later in the frame modifies (quant, mergemask, label1, junction), so it can be repeated with a larger round budget.
static void frame_regions(rd_detector *d, Slot *s, hipStream_t st, int nz, size_t zs) {
  region_stage(st, slot_region_planes(s), d->iw, d->ih, s->rounds, nz, zs);
}

// votes and probes of a frame whose regions were computed again (a frame whose rectangles the device computes gets them again as well,
// from the new regions, for the aperture known now)
static void redo_votes(rd_detector *d, Slot *s, hipStream_t st) {
  int with_post = 0;
  if (s->post_mode) {
    pthread_mutex_lock(&d->tan_mu);
    with_post = d->have_tan; s->post_tan = d->tan_aov;
    pthread_mutex_unlock(&d->tan_mu);
  }
  frames_votes(d, s->frame, 1, st, 1, with_post, s->post_tan);
  s->post_mode = with_post;
}

// The absorption of small regions again for a frame the two fast launches could not finish (h_ctr[RD_PACK_STATUS] != 0: more undecided pixels than
// the single-block tail holds, or dependency chains that wind through more rows than it sweeps - frames that consist of small
// regions), by rounds over work lists until nothing changes, then everything downstream of it.  Runs on a stream of the slot's own
// that is never captured (the loop synchronises), after the frame's ev_done: nothing else touches the slot's planes.
static void frame_absorb_slow(rd_detector *d, Slot *s) {
  if (!s->st_redo) s->st_redo = make_redo_stream();
  hipStream_t st = s->st_redo;
  region_absorb_slow(st, slot_region_planes(s), d->iw, d->ih);
  redo_votes(d, s, st);
  RD_HIP(hipStreamSynchronize(st));
  s->h_ctr[RD_PACK_STATUS] = 0;
}

// The whole frame-to-frame dependency chain in ONE launch (not captured: its planes change from frame to frame): this frame's strong mask
// (what oclrect.c:307-313 derives from the strength sums) from the sums + the strong mask of the frame before (H1, oclrect.c:274-275: the
// reference starts the sums from that mask; here the mask's element is added where a sum is read).  The same pass yields the edge mask at
// 500 of oclrect.c:277-284 and filters the labels at 2500 (filtering once at 2500 equals filtering at 500 and then at 2500, and both
// masks come from the unfiltered labels).
static void frame_strong(rd_detector *d, Slot *s, hipStream_t st) {
  const size_t N = (size_t)d->N;
  const long t = s->seq;
  s->prev_in = d->prev_ring + (size_t)(t % d->nring) * N;
  int8_t *out = d->prev_ring + (size_t)((t + 1) % d->nring) * N;
  rdk::strength_masks(st, NULL, out, NULL, s->e8, s->label1, s->strsum, d->t_edge, d->t_strong, d->iw, d->ih, s->prev_in, s->strongbits);      // (the mask as bytes for the next frame, as bits for this frame's polylines; nobody reads it as ints)
}

// gradient direction, re-packed blurred Lab, strength, non-max suppression (oclrect.c:251-258) of nz frames: one tile kernel that keeps the three
// intermediate planes on the chip (rd_k_front.hip: k_grad_nms); frame sizes its tiles do not cover take the three operators' kernels.
// taps: the intermediate planes are written as well (debug planes "plab1", "vxy", "strength")
bool front_is_fused(const rd_detector *d) { return rdk::grad_nms_fits(d->iw, d->ih) != 0; }
void frames_grad_nms(rd_detector *d, Slot *s, hipStream_t st, int nz, size_t zs, int taps) {
  const int iw = d->iw, ih = d->ih;
  if (front_is_fused(d)) {
    if (taps) rdk::grad_nms(st, s->nms, s->bl, iw, ih, nz, zs, s->plab1, s->vxy, s->strength);
    else rdk::grad_nms(st, s->nms, s->bl, iw, ih, nz, zs);
    return;
  }
  rdk::edgevec(st, s->vxy, s->bl[0], iw, ih, s->plab1, s->bl[1], s->bl[2], nz, zs);
  rdk::edge_plab(st, s->strength, s->plab1, iw, ih, nz, zs);
  rdk::thinthres(st, s->nms, s->strength, s->vxy, iw, ih, nz, zs);
}

// the front both detector kinds share, for nz frames: sigma=1 blur of L, a, b -> blurred planes (oclrect.c:246-251), then gradient direction (+ the packing of the
// blurred Lab, oclrect.c:251, on the way), strength, non-max suppression (oclrect.c:253-258)
static void frames_front(rd_detector *d, Slot *s, hipStream_t st, int nz, size_t zs) {
  const int iw = d->iw, ih = d->ih;
  { const float *c[3] = { s->tr[0], s->tr[1], s->tr[2] }; rdk::iir_blur_pass(st, s->hz, c, s->fw, s->bw, 3, ih, iw, 1, s->tails, s->flags, 1, nz, zs); }        // along x (source: 16-bit fields)
  { const float *c[3] = { s->hz[0], s->hz[1], s->hz[2] }; rdk::iir_blur_pass(st, s->bl, c, s->fw, s->bw, 3, iw, ih, 0, s->tails, s->flags + 1, 0, nz, zs); }   // along y
  frames_grad_nms(d, s, st, nz, zs);
}

// Segment 0 or 2 of one frame (nz = 1, zs = 0) or of the nz frames of a group, whose first slot is s and whose planes lie zs bytes apart.
static void frame_segment(rd_detector *d, Slot *s, int seg, hipStream_t st, int nz, size_t zs) {
  const int iw = d->iw, ih = d->ih;
  if (seg == 0) {
  // (colour conversion, oclrect.c:245: launched by launch_frames in front of this segment, outside the recorded graph - its source is the
  //  caller's device buffer when the frame is resident in HBM: no copy of the frame)
  frames_front(d, s, st, nz, zs);
  // mask of positive responses and the rect-path tidy (oclrect.c:262-272)
  // components (background included) of the tidied mask; the tidy itself runs inside the labelling's tile kernel (and clears the
  // strength sums for the H1 segment); the walk to the roots happens in the first kernel of the next segment
  rdk::label8_tidy(st, s->label1, NULL, s->tidy, s->nms, s->strsum, iw, ih, 1, nz, zs);      // (the mask of positive responses, oclrect.c:262-264, is not stored: nothing reads it - debug plane "mask0" derives it from the responses)
  // strength sums per component (oclrect.c:274-275) - without the strong mask of the frame before (H1), which frame_strong() adds
  rdk::calc_strength(st, s->strsum, s->nms, s->label1, iw, ih, NULL, 1, nz, zs);
  return;
  }
  // Three chains leave this point and meet again before the region stage / the votes:
  //   main stream: edge-stopped blur x20 -> quantise -> despeckle                              (oclrect.c:286-303)
  //   2nd stream : junction counts of the filtered labels -> merge mask                      (oclrect.c:315-321)
  //                then the polyline stage, which needs nothing but the strong mask          (oclrect.c:361)
  // With one or two frames in flight (fork_poly: never a group) the second chain runs on the slot's second stream; else everything on the main stream, blur chain first.
  const bool fork = d->fork_poly != 0;
  if (fork) {
    RD_HIP(hipEventRecord(s->ev_fork, st));
    RD_HIP(hipStreamWaitEvent(s->st2, s->ev_fork, 0));
    rdk::junction_bits(s->st2, (unsigned long long *)s->scratch2, s->strongbits, iw, ih);
    rdk::merge_mask(s->st2, s->mmbits, (const unsigned long long *)s->scratch2, iw, ih);
    RD_HIP(hipEventRecord(s->ev_mm, s->st2));
  }

  // edge-preserving smoothing x10, quantise, despeckle (oclrect.c:286-303)
  rdk::blblur_extents(st, s->ext, s->e8, iw, ih, nz, zs);
  // (Two pairs per launch - halo of 8 cells, four passes through two LDS planes, with and without running sums - halve the launches and
  //  the HBM traffic of this stage and were measured 6 % SLOWER at full rate: 100 KB of LDS leave one 1024-thread block per CU and the
  //  extra barriers cost more than the saved traffic; the stage is bound by vector instructions, not by memory.  DESIGN.md.)
  { const uint32_t *src = s->plab0;     // ping-pong between i0 and smooth; the 10th pair lands in smooth
    for (int i = 0; i < 10; i++) { uint32_t *dst = (i & 1) ? s->smooth : (uint32_t *)s->i0; rdk::blblur_pair(st, dst, s->ext, src, iw, ih, nz, zs); src = dst; } }
  rdk::despeckle(st, s->quant, s->smooth, s->nms, iw, ih, 1, nz, zs);      // quantisation to 24 levels per field (oclrect.c:298) happens on the fly

  if (fork) RD_HIP(hipStreamWaitEvent(st, s->ev_mm, 0));
  else {
    rdk::junction_bits(st, (unsigned long long *)s->scratch2, s->strongbits, iw, ih, nz, zs);
    rdk::merge_mask(st, s->mmbits, (const unsigned long long *)s->scratch2, iw, ih, nz, zs);
  }

  frame_regions(d, s, st, nz, zs);
  if (fork) { frame_polyline(d, s->frame, 1, s->st2, s->poly_mode); RD_HIP(hipEventRecord(s->ev_join, s->st2)); }      // (the polyline chain's launches follow the region stage's: of the three places tried - first, before that stage, after it - the one kept)

  if (d->batch > 1) return;      // the sparse stages of the batch's frames follow in one set of launches (sparse_launch)
  if (fork) RD_HIP(hipStreamWaitEvent(st, s->ev_join, 0));
  else frame_polyline(d, s->frame, nz, st, s->poly_mode);
  frames_votes(d, s->frame, nz, st, 1, 0);
}

// The polyline kind (rd_polyline_detector_create): poly.cpp:104-123 / vidpoly.cpp:165-183 per frame, for nz frames as above.  The front of the rect kind, the
// components of nms > 0 (no tidy), the strength sums from zero (no H1 carry-over: poly.cpp:118 clears them), filterStrength + `label > 0` as a bit plane, the
// polyline stage with the frame ring at zero (the reference's tmp3 is a fresh, zeroed buffer: poly.cpp:93) and the hand-off of the list's first records into
// pinned host memory.  Nothing depends on the frame before: the whole frame is one captured sequence.
static void poly_segment(rd_detector *d, Slot *s, int nz, size_t zs, hipStream_t st, int mode) {
  const int iw = d->iw, ih = d->ih, N = d->N;
  frames_front(d, s, st, nz, zs);
  rdk::label8_positive(st, s->label1, s->mask0, s->nms, s->strsum, iw, ih, 1, nz, zs);      // (poly.cpp:115-118; the walk to the roots happens in the next kernel)
  rdk::calc_strength(st, s->strsum, s->nms, s->label1, iw, ih, NULL, 1, nz, zs);           // (poly.cpp:119)
  rdk::poly_mask_bits(st, s->strongbits, s->label1, s->strsum, d->p_thre, iw, ih, nz, zs);   // (poly.cpp:120-121)
  rdk::polyline(st, s->frame, nz, N * 16, 0, d->p_minerror, d->p_size, iw, ih, mode);      // (poly.cpp:123)
  rdk::polyline_handoff(st, s->frame, nz, d->handoff_rec);
}

// region-merge round budgets a frame can be launched with; the rounds stop changing anything after ~10 on typical frames
// and every launched round costs two dispatches even when it exits at once, so the budget follows what recent frames
// needed (+ margin).  A frame whose last launched round still changed something is repeated with the full budget
// (slot_postprocess), so the result never depends on the budget.
static const int kRoundBudgets[RD_NBUDGETS] = { 8, 10, 12, 14, 16, 18, 20 };
static int budget_index(int rounds) { for (int k = 0; k < RD_NBUDGETS; k++) if (kRoundBudgets[k] == rounds) return k; return RD_NBUDGETS - 1; }

// how the polyline stage of the next frame is launched: the single-block kernel (1) until two frames in a row overflowed its on-chip tables
// (e.g. 3840x2160), from then on the ~85-launch form (0), which is also what repeats a frame the single-block kernel gave up on.  (One
// cooperative launch of several blocks per frame was built in round 3 and measured slower than the 85 launches: profiles/NOTES_r03.md.)
static int current_poly_mode(const rd_detector *d) {
  if (d->poly_mode == 0) return 0;
  return __atomic_load_n(&d->poly_overflows, __ATOMIC_RELAXED) ? 0 : 1;
}

// Where slot s keeps the captured form of launch sequence `seq` for nz frames (Slot::graphs), or NULL where the sequence runs kernel by kernel: without graphs
// (RD_NO_GRAPH), and with one or two frames in flight - the captured graph of the forked segment starts its second branch 170 us late, and the front segment, a
// straight line of ten kernels, is no faster as a graph either: 1615-1623 against 1636-1652 frames/s two deep (profiles/NOTES_r05.md).
static hipGraphExec_t *slot_graph(rd_detector *d, Slot *s, int nz, int seq) {
  if (!d->use_graph || d->fork_poly) return NULL;
  return &s->graphs[nz > 1 ? 1 : 0][seq];
}

// Enqueues on st what `record` enqueues there: directly (ge == NULL), or as a graph that is captured from it on first use and kept in *ge.
template <typename F> static void launch_captured(rd_detector *d, hipGraphExec_t *ge, hipStream_t st, F record) {
  if (!ge) { record(); return; }
  if (!*ge) {
    hipGraph_t g = NULL;
    pthread_mutex_lock(&d->launch_mu);
    RD_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    record();
    RD_HIP(hipStreamEndCapture(st, &g));
    pthread_mutex_unlock(&d->launch_mu);
    RD_HIP(hipGraphInstantiate(ge, g, NULL, NULL, 0));
    RD_HIP(hipGraphDestroy(g));
  }
  RD_HIP(hipGraphLaunch(*ge, st));
}

// What the rect kind launches behind the front kernel of one frame (nz = 1) or of the full group that slot s leads.  What cannot be shared by a group is the short
// middle part - a frame's strength sums start from the strong mask of the frame before it (H1) - which runs between the two captured segments, on the same stream.
static void rect_frames(rd_detector *d, Slot *s, int nz, hipStream_t st) {
  const size_t zs = nz > 1 ? d->slot_pitch : 0;
  launch_captured(d, slot_graph(d, s, nz, 0), st, [&] { frame_segment(d, s, 0, st, nz, zs); });
  // the strong masks: each frame's on top of its predecessor's (H1) - one launch for a group where its planes allow 16-byte accesses (the mask of the frame before
  // only decides sums that stand one below a threshold, and is then evaluated on the spot: k_strength_masks_group), else frame by frame
  if (d->have_last_strong) RD_HIP(hipStreamWaitEvent(st, d->last_strong, 0));      // (only the first frame waits for the group before - another stream - and only the last is waited for)
  bool one_launch = nz > 1 && !d->strong_by_frame && (d->N & 3) == 0 && rdk::strength_masks_group_fits(d->iw, s->label1, d->prev_ring, s->e8, zs);
  for (int i = 1; i < nz; i++) one_launch = one_launch && s[i].seq == s->seq + i;
  if (one_launch) {
    for (int i = 0; i < nz; i++) s[i].prev_in = d->prev_ring + (size_t)(s[i].seq % d->nring) * (size_t)d->N;
    rdk::strength_masks_group(st, d->prev_ring, s->e8, s->label1, s->strsum, d->t_edge, d->t_strong, d->iw, d->ih, s->strongbits, s->seq, d->nring, nz, zs);
    d->n_strong_group++;
  } else {
    for (int i = 0; i < nz; i++) frame_strong(d, &s[i], st);
    if (nz > 1) d->n_strong_by_frame++;
  }
  RD_HIP(hipEventRecord(s[nz - 1].ev_strong, st));
  d->last_strong = s[nz - 1].ev_strong; d->have_last_strong = 1;
  int rounds = d->fixed_rounds ? d->fixed_rounds : __atomic_load_n(&d->rounds_budget, __ATOMIC_RELAXED);
  if (d->budget_cycle) rounds = kRoundBudgets[2 + (int)((s->seq / d->budget_cycle) % (RD_NBUDGETS - 2))];      // (tests: a new graph every few frames)
  const int pm = current_poly_mode(d), bi = budget_index(rounds);
  for (int i = 0; i < nz; i++) { s[i].rounds = rounds; s[i].poly_mode = pm; d->budget_count[bi]++; }
  launch_captured(d, slot_graph(d, s, nz, 1 + 2 * bi + (d->batch == 1 ? pm : 0)), st, [&] { frame_segment(d, s, 2, st, nz, zs); });
  if (d->batch > 1) return;      // (votes, probes and rectangles follow with the batch's sparse stages)
  double tn = 0;
  const int with_post = aperture_snapshot(d, &tn) && d->device_post;
  if (with_post) rdk::post_device(st, s->frame, nz, d->maxrec_dev, d->iw, d->ih, tn);      // (outside the captured graphs: the aperture is a launch argument)
  for (int i = 0; i < nz; i++) { s[i].post_mode = with_post; s[i].post_tan = tn; }
}

// the polyline kind's: its one sequence, captured per polyline mode
static void poly_frames(rd_detector *d, Slot *s, int nz, hipStream_t st) {
  const size_t zs = nz > 1 ? d->slot_pitch : 0;
  const int pm = current_poly_mode(d);
  for (int i = 0; i < nz; i++) s[i].poly_mode = pm;
  launch_captured(d, slot_graph(d, s, nz, 1 + pm), st, [&] { poly_segment(d, s, nz, zs, st, pm); });
}

// the frame is on its way: its worker thread may start waiting for ev_done (which has been recorded by now - an event that was never
// recorded counts as complete)
static void slot_submitted(rd_detector *d, Slot *s) {
  if (d->nworkers > 0) {
    pthread_mutex_lock(&s->mu);
    s->state = 1;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
  }
}

// All launches of one frame (nz = 1, st = its slot's stream) or of the full group that slot s leads, for either detector kind.
// Group mode (rd_detector::zb > 1): the frames of zb consecutive slots in ONE set of launches, dense stages included (frame = blockIdx.z; the
// slots' planes lie slot_pitch bytes apart).  For frames so small that a launch does not fill the device (a 640x480 plane is 75 tiles for
// 256 CUs): the frame rate is then set by the number of launches the four hardware queues get through, and a group needs as many as a
// single frame.
static void launch_frames(rd_detector *d, Slot *s, int nz, hipStream_t st) {
  // (ONE pair of events brackets a group - its frames start and end together -, not one per frame: every record is a release fence in the stream)
  RD_HIP(hipEventRecord(s->ev_begin, st));
  for (int i = 0; i < nz; i++) { s[i].pending_dense = 0; s[i].watch_begin = s->ev_begin; s[i].watch_done = s->ev_done; s[i].group_n = nz; }
  // the colour conversion, outside the captured sequences: its source changes from frame to frame
  if (s->scale == 2) {      // (rd_detector_enqueue_scaled: the frames share format, scale and pitches)
    const uint8_t *planes[RD_ZB_MAX][3];
    for (int i = 0; i < nz; i++) for (int k = 0; k < 3; k++) planes[i][k] = s[i].pl[k];
    rdk::pix2plab_half_transposed(st, s->fmt, s->plab0, s->tr, planes, s->pitch, d->iw, d->ih, nz, nz > 1 ? d->slot_pitch : 0);
  } else if (s->fmt != RD_PIX_BGR) {      // (rd_detector_enqueue_planes: the frames share format and pitches)
    const uint8_t *planes[RD_ZB_MAX][3];
    for (int i = 0; i < nz; i++) for (int k = 0; k < 3; k++) planes[i][k] = s[i].pl[k];
    rdk::pix2plab_transposed(st, s->fmt, s->plab0, s->tr, planes, s->pitch, d->iw, d->ih, nz, nz > 1 ? d->slot_pitch : 0);
  } else if (nz == 1) rdk::bgr2plab_transposed(st, s->plab0, s->tr, s->src, d->iw, d->ih, s->ws);
  else {
    const uint8_t *srcs[RD_ZB_MAX];
    for (int i = 0; i < nz; i++) srcs[i] = s[i].src;
    rdk::bgr2plab_transposed(st, s->plab0, s->tr, srcs, d->iw, d->ih, s->ws, nz, d->slot_pitch);
  }
  if (d->kind == RD_KIND_POLY) poly_frames(d, s, nz, st); else rect_frames(d, s, nz, st);
  if (d->batch > 1) { RD_HIP(hipEventRecord(s->ev_dense, st)); s->pending_sparse = 1; }      // (ev_done: behind the batch's sparse stages, sparse_launch)
  else RD_HIP(hipEventRecord(s->ev_done, st));
  rdrt::check_launch(d->kind == RD_KIND_POLY ? "polyline frames" : "rect frames");
  if (d->batch == 1) for (int i = 0; i < nz; i++) slot_submitted(d, &s[i]);
}

// may two frames of a group share one front launch?  (one format, one scale, one set of row strides)
static bool same_layout(const Slot *a, const Slot *b) {
  if (a->fmt != b->fmt || a->scale != b->scale || a->ws != b->ws) return false;
  return a->fmt == RD_PIX_BGR || (a->pitch[1] == b->pitch[1] && a->pitch[2] == b->pitch[2]);
}

static hipStream_t group_stream(rd_detector *d, int g0) { return d->slots[(g0 / d->zb) % (d->nstreams > 0 ? d->nstreams : 1)].st; }

// the frames waiting in the group that starts at slot g0: all zb of them with one layout -> one set of launches; anything else (a poll
// that wants a result before the group is full, the end of a stream) -> frame by frame, the way a detector without groups launches them
static void group_launch(rd_detector *d, int g0) {
  const int g1 = g0 + d->zb < d->nslots ? g0 + d->zb : d->nslots;
  int cnt = 0;
  bool same = true, travelled = false;
  for (int i = g0; i < g1; i++) {
    const Slot *s = &d->slots[i];
    if (!s->pending_dense) continue;
    cnt++;
    same = same && same_layout(s, &d->slots[g0]);
    travelled = travelled || s->src == s->bgr || (s->sc_bgr && s->src == s->sc_bgr);
  }
  if (cnt == 0) return;
  // Host frames travelled when they were handed over, one after the other on the detector's upload stream (hand_over).  The launching thread waits for that
  // stream here - at most for the transfer just issued, 0.1 ms, on a thread that has nothing else to do until the next group completes - and what the host has seen
  // complete needs no ordering on the device: no event.  Round 6 found the 7-8 % that host frames cost against frames resident in HBM in exactly two places: an event
  // recorded after every upload (a record is a system-scope release, a write-back of the device's caches, 2 900 times a second in the middle of everybody's kernels:
  // 2671-2698 frames/s with it, 2886-2901 without) and - pinned frames, whose hand-over takes microseconds - eight transfers queued on the copy engine at once
  // (2701-2723 against 2849-2884 with one at a time).  profiles/NOTES_r06.md.
  if (travelled) RD_HIP(hipStreamSynchronize(d->st_upload));
  if (cnt == d->zb && same) { launch_frames(d, &d->slots[g0], d->zb, group_stream(d, g0)); return; }
  for (int i = g0; i < g1; i++) if (d->slots[i].pending_dense) launch_frames(d, &d->slots[i], 1, d->slots[i].st);
}

// Batched mode: the sparse stages of slots a..b (consecutive slots of one group, dense stages enqueued) as one set of launches on
// the stream of one of them - a different one each time, so that the extra ~0.4 ms of queue time does not always delay the same
// stream's next frame - behind the dense stages of all of them.
static void sparse_launch(rd_detector *d, int a, int b) {
  const int nb = b - a + 1;
  Slot *host = &d->slots[a + (int)(d->sparse_rot++ % (unsigned)nb)];
  hipStream_t st = host->st;
  for (int i = a; i <= b; i++) if (d->slots[i].st != st) RD_HIP(hipStreamWaitEvent(st, d->slots[i].ev_dense, 0));
  const int pm = current_poly_mode(d);
  const rdk::PolyFrame *frames = d->frames + a;
  frame_polyline(d, frames, nb, st, pm);
  double tn = 0;
  const int with_post = aperture_snapshot(d, &tn) && d->device_post;
  frames_votes(d, frames, nb, st, 1, with_post, tn);
  for (int i = a; i <= b; i++) {
    Slot *s = &d->slots[i];
    s->post_mode = with_post; s->post_tan = tn;
    s->poly_mode = pm;
    RD_HIP(hipEventRecord(s->ev_done, st));
    s->watch_done = s->ev_done;
    s->pending_sparse = 0;
  }
  rdrt::check_launch("rect frames, sparse stages");
  for (int i = a; i <= b; i++) slot_submitted(d, &d->slots[i]);
}

// launches what is pending in the group of slot si (a poll needs one of its frames, or the detector is drained)
static void sparse_flush(rd_detector *d, int si) {
  const int g0 = si / d->batch * d->batch, g1 = g0 + d->batch - 1 < d->nslots - 1 ? g0 + d->batch - 1 : d->nslots - 1;
  int a = -1, b = -1;
  for (int i = g0; i <= g1; i++) if (d->slots[i].pending_sparse) { if (a < 0) a = i; b = i; }
  if (a >= 0) sparse_launch(d, a, b);
  if (d->deferred_slot >= g0 && d->deferred_slot <= g1) d->deferred_slot = -1;
}

static void wait_event_outside_captures(rd_detector *d, hipEvent_t ev);
static void slot_fetch(Slot *s, void *dst, const void *src, size_t bytes);

// What remains to be done on the device for a finished slot, once per frame (on the polling thread or on the slot's worker): the two
// rare repeats and the bookkeeping of the round budget.
static void slot_finish_device(rd_detector *d, Slot *s) {
  if (s->rounds <= RD_REGION_FIRST_BUDGET && s->h_ctr[RD_PACK_FLAGS + s->rounds - 1] != 0) {   // the region merge was still changing in its last launch: again with as many launches as it takes (region_ladder)
    // (on a stream of the slot's own: the slot's regular stream is one of the four that carry the groups, and the repeat would wait there behind a whole group of
    //  other frames; nothing but this frame's result depends on it - the frame is finished, ev_done has been waited for)
    static const bool redo_inline = RD_LAB_INT("RD_REDO_ON_MAIN_STREAM", 0) != 0;
    if (!s->st_redo && !redo_inline) s->st_redo = make_redo_stream();
    hipStream_t rst = redo_inline ? s->st : s->st_redo;
    const LadderEnd end = region_ladder([&](int budget) {
      s->rounds = budget;
      pthread_mutex_lock(&d->launch_mu);
      frame_regions(d, s, rst, 1, 0);
      redo_votes(d, s, rst);
      RD_HIP(hipEventRecord(s->ev_redo, rst));
      pthread_mutex_unlock(&d->launch_mu);
      wait_event_outside_captures(d, s->ev_redo);
      int still = 0;
      slot_fetch(s, &still, s->scratch2 + d->N + budget - 1, sizeof(int));      // the flag of the budget's last launch
      return still;
    });
    if (!end.settled) __atomic_add_fetch(&d->n_unsettled, 1, __ATOMIC_RELAXED);      // (the definition's limit: the frame keeps what that many launches made of it - counter 6)
    __atomic_add_fetch(&d->n_redo_rounds, 1, __ATOMIC_RELAXED);
  }
  if (s->h_ctr[RD_PACK_STATUS] != 0 || (d->force_redo & 2)) {   // the absorption's fast path gave up on this frame: finish it the long way
    frame_absorb_slow(d, s);
    __atomic_add_fetch(&d->n_redo_absorb, 1, __ATOMIC_RELAXED);
  }
  {   // budget for the frames to come (need = launches up to and including the first one that changed nothing)
    int need = 20;
    for (int r = 0; r < 20; r++) if (s->h_ctr[RD_PACK_FLAGS + r] == 0) { need = r + 1; break; }
    pthread_mutex_lock(&d->tan_mu);
    d->need_count[need]++;
    d->need_hist[d->need_pos++ & 63] = need;
    // what all but the three most demanding of the last 64 frames needed (a repeat costs a region stage, ~90 launches; a launch too many
    // costs 5 us in EVERY frame: on the bench stream 97 % of the frames need 9-11 launches, one in 150 needs 17 or more)
    int cnt[22] = { 0 }, seen = 0, mx = 20;
    for (int k = 0; k < 64; k++) cnt[d->need_hist[k] > 20 ? 20 : d->need_hist[k]]++;
    for (int v = 20; v >= 0; v--) { seen += cnt[v]; if (seen > 3) { mx = v; break; } }
    int b = 20;
    for (int k = RD_NBUDGETS - 1; k >= 0; k--) if (d->need_pos >= 8 && kRoundBudgets[k] >= mx + 1) b = kRoundBudgets[k];
    __atomic_store_n(&d->rounds_budget, b, __ATOMIC_RELAXED);
    pthread_mutex_unlock(&d->tan_mu);
  }
  // two overflows among the stream's recent frames (whichever slots they ran in): its frames do not fit the single-launch kernel (e.g. 4K) - stop trying
  if (s->poly_mode == 1 && s->h_ctr[RD_PACK_GAVE_UP] != 0 && __atomic_add_fetch(&d->overflow_streak, 1, __ATOMIC_RELAXED) >= 2) __atomic_store_n(&d->poly_overflows, 1, __ATOMIC_RELAXED);
  if (s->poly_mode == 1 && s->h_ctr[RD_PACK_GAVE_UP] == 0) __atomic_store_n(&d->overflow_streak, 0, __ATOMIC_RELAXED);
  if ((s->poly_mode && s->h_ctr[RD_PACK_GAVE_UP] != 0) || (d->force_redo & 1)) {   // the single-launch polyline stage overflowed: repeat the tail the long way
    s->post_mode = 0;
    pthread_mutex_lock(&d->launch_mu);
    frame_tail(d, s, 0);
    RD_HIP(hipEventRecord(s->ev_redo, s->st));
    pthread_mutex_unlock(&d->launch_mu);
    wait_event_outside_captures(d, s->ev_redo);
    __atomic_add_fetch(&d->n_redo, 1, __ATOMIC_RELAXED);
  }
}

// Waiting for an event from a thread that is not the enqueueing one.  Slots share streams, and the enqueueing thread records a new graph
// on a slot's stream whenever a (slot, launch budget) pair is used for the first time - in the middle of a run, since the budget of the
// region merge follows the stream.  HIP refuses hipEventSynchronize / hipEventQuery on an event whose stream is being captured ("operation
// not permitted on an event last recorded in a capturing stream"), so the wait is a poll whose queries exclude captures (launch_mu: held by
// launch_captured for the duration of a capture, a few hundred microseconds).
static void wait_event_outside_captures(rd_detector *d, hipEvent_t ev) {
  for (;;) {
    pthread_mutex_lock(&d->launch_mu);
    const hipError_t e = hipEventQuery(ev);
    pthread_mutex_unlock(&d->launch_mu);
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) { RD_HIP(e); }
    struct timespec ts = { 0, 30000 };
    nanosleep(&ts, NULL);
  }
}

// device -> host copy for a slot whose device work is complete, from any thread: on the slot's private stream (never the legacy stream -
// a plain hipMemcpy would make that depend on a stream another thread may be capturing a graph on)
static void slot_fetch(Slot *s, void *dst, const void *src, size_t bytes) {
  if (!s->st_redo) s->st_redo = make_redo_stream();
  RD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->st_redo));
  RD_HIP(hipStreamSynchronize(s->st_redo));
}

// the list a poll returns from a result block of the device post-process (rd_k_post.hip: PolyFrame::post_out) that did not overflow: the
// valid candidates' records in candidate order, element 0 the header.  (Also what the test tap rd_postprocess_planes_device returns.)
rect_t *post_block_rectangles(const int *h_post) {
  const int nc = h_post[0];
  const char *recs = (const char *)(h_post + 8 + RD_POST_MAXC);
  int nv = 0;
  for (int c = 0; c < nc; c++) nv += h_post[8 + c] != 0;
  rect_t *ret = (rect_t *)calloc((size_t)nv + 1, sizeof(rect_t));
  int at = 1;
  for (int c = 0; c < nc; c++) if (h_post[8 + c] != 0) memcpy(&ret[at++], recs + (size_t)c * sizeof(rect_t), sizeof(rect_t));
  ret[0].nItems = nv + 1;
  return ret;
}

// host post-process of a slot whose device work is complete: rectangles for the given aperture + a copy of the segment list
// (can run again for another aperture: touches nothing on the device but, for frames with very many segments, two copies)
static void *slot_rectangles(rd_detector *d, Slot *s, double tanAOV, void **segs_out, int *nsegs_out) {
  int n = ((int *)s->h_segs)[0];
  // the rectangles the device computed (rd_k_post.hip), if this frame has them for this aperture and nothing overflowed there:
  // the valid candidates' records in candidate order (= the reference's list order)
  if (s->post_mode && s->post_tan == tanAOV && s->h_post[1] == 0 && n + 1 <= d->maxrec_dev) {
    rect_t *ret = post_block_rectangles(s->h_post);
    // the segment list handed to rd_detector_last_segments: all n records, as on the host path - the pinned block holds the first
    // RD_MAXREC of them, a frame with more fetches the list from the device
    void *copy0 = malloc((size_t)(n + 1) * 56);
    if (n + 1 <= RD_MAXREC) memcpy(copy0, s->h_segs, (size_t)(n + 1) * 56);
    else slot_fetch(s, copy0, s->lslist, (size_t)(n + 1) * 56);
    *segs_out = copy0; *nsegs_out = n;
    __atomic_add_fetch(&d->n_post_device, 1, __ATOMIC_RELAXED);
    return ret;
  }
  __atomic_add_fetch(&d->n_post_host, 1, __ATOMIC_RELAXED);
  const void *segs = s->h_segs; const int *probes = s->h_probes;
  void *big_segs = NULL; int *big_probes = NULL;
  int maxrec = d->maxrec_dev < RD_MAXREC ? d->maxrec_dev : RD_MAXREC;
  if (n + 1 > maxrec) {   // rare: more segments than the fixed-size transfer covers
    const int *dev_probes = s->probes;
    if (n + 1 > d->maxrec_dev) {
      // more records than the slot's probe buffer holds (the list itself has the reference's capacity, 16N / 56 records, pl:456): the
      // probes of all of them are taken again into a buffer that grows on demand - nothing is ever dropped
      if (!s->st_redo) s->st_redo = make_redo_stream();
      if (s->big_probes_cap < n + 1) { dfree(s->big_probes); s->big_probes = dnew<int>((size_t)(n + 1) * RD_PROBE_INTS); s->big_probes_cap = n + 1; }
      rdk::PolyFrame f = *s->frame;
      f.probes = s->big_probes; f.pack = NULL;
      rdk::sample_segments(s->st_redo, &f, 1, n + 1, d->iw, d->ih, d->N * 4 / 5, 0);
      rdrt::check_launch("probes of a frame with very many segments");
      dev_probes = s->big_probes;
      __atomic_add_fetch(&d->n_truncated, 1, __ATOMIC_RELAXED);      // (counter 10: frames that took this path)
    }
    big_segs = malloc((size_t)(n + 1) * 56); big_probes = (int *)malloc((size_t)(n + 1) * RD_PROBE_INTS * sizeof(int));
    slot_fetch(s, big_segs, s->lslist, (size_t)(n + 1) * 56);
    slot_fetch(s, big_probes, dev_probes, (size_t)(n + 1) * RD_PROBE_INTS * sizeof(int));
    segs = big_segs; probes = big_probes; maxrec = n + 1;
  }
  // RD_DIAG_NO_POST (diagnostics only): an empty rectangle list instead of the host post-process, to see whether a run is host-bound
  struct timespec tp0, tp1;
  clock_gettime(CLOCK_MONOTONIC, &tp0);
  void *r = rd_post_run(segs, maxrec, probes, d->iw, d->ih, tanAOV);
  clock_gettime(CLOCK_MONOTONIC, &tp1);
  __atomic_add_fetch(&d->host_post_ns, (tp1.tv_sec - tp0.tv_sec) * 1000000000L + (tp1.tv_nsec - tp0.tv_nsec), __ATOMIC_RELAXED);
  const int ns = n < maxrec ? n : maxrec - 1;
  void *copy = malloc((size_t)(ns + 1) * 56);
  memcpy(copy, segs, (size_t)(ns + 1) * 56);
  free(big_segs); free(big_probes);
  *segs_out = copy; *nsegs_out = ns;
  return r;
}

void *slot_worker(void *arg) {
  Slot *s = (Slot *)arg;
  rd_detector *d = s->owner;
  RD_HIP(hipSetDevice(d->device));
  for (;;) {
    pthread_mutex_lock(&s->mu);
    while (s->state != 1 && !s->quit) pthread_cond_wait(&s->cv, &s->mu);
    if (s->quit) { pthread_mutex_unlock(&s->mu); return NULL; }
    pthread_mutex_unlock(&s->mu);
    // the aperture arrives with the poll (reference API); workers run ahead with the last one seen
    pthread_mutex_lock(&d->tan_mu);
    while (!d->have_tan && !s->quit) pthread_cond_wait(&d->tan_cv, &d->tan_mu);
    const double tan = d->tan_aov;
    pthread_mutex_unlock(&d->tan_mu);
    if (s->quit) return NULL;
    // Frames finish roughly in sequence order, and the caller collects them in that order: only the workers of the frames next in line watch their event
    // closely (a query every 30 us); the others - with 64 frames in flight, most of them, for most of the 25 ms their frame spends on the device - sleep in
    // longer steps until the front of finished frames comes within two groups of theirs.  (All of them polling was two million event queries a second
    // through the runtime's locks, next to the thread that launches.)
    {
      const long window = 2L * (d->zb > 1 ? d->zb : 4);
      while (!s->quit && s->seq >= __atomic_load_n(&d->done_seq, __ATOMIC_RELAXED) + window) { struct timespec ts = { 0, 250000 }; nanosleep(&ts, NULL); }
    }
    wait_event_outside_captures(d, s->watch_done);
    { long cur = __atomic_load_n(&d->done_seq, __ATOMIC_RELAXED); while (cur < s->seq + 1 && !__atomic_compare_exchange_n(&d->done_seq, &cur, s->seq + 1, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { } }
    void *segs = NULL; int ns = 0;
    slot_finish_device(d, s);
    void *r = slot_rectangles(d, s, tan, &segs, &ns);
    pthread_mutex_lock(&s->mu);
    s->result = r; s->result_tan = tan; s->res_segs = segs; s->res_nsegs = ns;
    s->state = 2;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
  }
}

extern "C" {

// ---- hand-over of a frame (rd_detector_enqueue, rd_detector_enqueue_planes)
// The planes a format uses and the layout of a host frame packed into a slot's buffers: rd_jobs.h.
using rdjob::PixLayout;
using rdjob::pix_layout;
// a BGR frame of rd_detector_enqueue keeps the caller's row stride on its way through the slot's buffers: one plane of ws * ih bytes
static PixLayout bgr_layout(int ws, int ih) {
  PixLayout L;
  memset(&L, 0, sizeof(L));
  L.np = 1; L.row[0] = L.pitch[0] = ws; L.rows[0] = ih; L.bytes = (size_t)ws * ih;
  return L;
}

// a pageable frame's way to the device: pieces (byte ranges of the packed layout) gathered from the caller's planes into pinned memory by the caller and whichever
// helper threads are awake, uploaded in order as they complete
struct UploadJob { PixLayout L; const uint8_t *src[3]; int spitch[3]; char *dst, *dev; size_t piece; hipStream_t st; int n, uploaded; int ready[16]; };
static void pack_range(const UploadJob *j, size_t o, size_t end) {
  for (int k = 0; k < j->L.np; k++) {
    const size_t p0 = j->L.off[k], pp = (size_t)j->L.pitch[k];
    const size_t a = o > p0 ? o : p0, b = end < p0 + pp * j->L.rows[k] ? end : p0 + pp * j->L.rows[k];
    if (a >= b) continue;
    if (j->spitch[k] == j->L.pitch[k] && j->L.row[k] == j->L.pitch[k]) { rd_copy_to_staging(j->dst + a, j->src[k] + (a - p0), b - a); continue; }      // (the caller's plane is laid out as the packed one - a BGR frame always: one copy)
    for (size_t r = (a - p0) / pp, at = a; at < b; r++) {      // rows of plane k that meet [a, b)
      const size_t rs = p0 + r * pp, re = rs + (size_t)j->L.row[k];
      const size_t c0 = at > rs ? at : rs, c1 = b < re ? b : re;
      if (c0 < c1) rd_copy_to_staging(j->dst + c0, j->src[k] + r * j->spitch[k] + (c0 - rs), c1 - c0);
      at = rs + pp;
    }
  }
}
static void pack_copy_piece(void *ctx, int i) {
  UploadJob *u = (UploadJob *)ctx;
  const size_t o = (size_t)i * u->piece, m = u->L.bytes - o < u->piece ? u->L.bytes - o : u->piece;
  pack_range(u, o, o + m);
  __atomic_store_n(&u->ready[i], 1, __ATOMIC_RELEASE);
}
static void upload_progress(void *ctx) {      // (caller's thread only)
  UploadJob *u = (UploadJob *)ctx;
  int e = u->uploaded;
  while (e < u->n && __atomic_load_n(&u->ready[e], __ATOMIC_ACQUIRE)) e++;
  if (e == u->uploaded) return;
  const size_t o = (size_t)u->uploaded * u->piece, end = (size_t)e * u->piece < u->L.bytes ? (size_t)e * u->piece : u->L.bytes;
  RD_HIP(hipMemcpyAsync(u->dev + o, u->dst + o, end - o, hipMemcpyHostToDevice, u->st));
  u->uploaded = e;
}

// is this host buffer page-locked (allocatePinnedMemory of oclhelper.h, rd_host_alloc, hipHostMalloc, hipHostRegister)?  One question to the runtime per buffer, not per frame.
static bool host_buffer_is_pinned(rd_detector *d, const void *frame) {
  for (int k = 0; k < 2; k++) if (d->probed[k] == frame) return d->probed_pinned[k] != 0;
  const bool pinned = rdjob::memory_type(frame) == hipMemoryTypeHost;
  d->probed[1] = d->probed[0]; d->probed_pinned[1] = d->probed_pinned[0];
  d->probed[0] = frame; d->probed_pinned[0] = pinned ? 1 : 0;
  return pinned;
}

// what follows the hand-over of a frame: its launches - now, or with its group - and the caller's wait for the copy engine
static long enqueue_launch(rd_detector *d, Slot *s, Slot *wait_upload, struct timespec ts0) {
  const int si = (int)(s - d->slots);
  if (d->zb > 1) {      // group mode: launched together with the other frames of its group, once that is full (or a poll needs one of them)
    s->pending_dense = 1;
    // (the last group of slots may be short - nslots need not be a multiple of zb - and is launched when ITS last slot is filled: every group
    //  is launched the moment its last frame arrives, so frames reach the device in sequence order and at most one group is ever waiting)
    if (si % d->zb == d->zb - 1 || si == d->nslots - 1) group_launch(d, si / d->zb * d->zb);
  } else {
    launch_frames(d, s, 1, s->st);
    if (d->batch > 1 && (si % d->batch == d->batch - 1 || si == d->nslots - 1)) {      // the batch is complete
      // Launched right away, the sparse stages would sit in their stream between this group's dense stages and the next one's, waiting
      // for the slowest of the group's four streams: a barrier per group (measured: 10 % slower than no batching).  One group later,
      // everything they wait for is long done and the stream they land on has the next group's dense work queued in front of them.
      if (d->defer) {
        const int prev = d->deferred_slot;
        d->deferred_slot = si;
        if (prev >= 0) sparse_flush(d, prev);
      } else sparse_flush(d, si);
    }
  }
  if (wait_upload) RD_HIP(hipEventSynchronize(wait_upload->ev_upload));      // (the caller may touch its buffer again)
  { struct timespec ts1; clock_gettime(CLOCK_MONOTONIC, &ts1); d->host_enqueue_ns += (ts1.tv_sec - ts0.tv_sec) * 1000000000L + (ts1.tv_nsec - ts0.tv_nsec); }
  return d->next_enqueue++;
}

// The next slot takes a frame - format, planes and row strides as the entry point `who` checked them; L: the layout a host frame is packed into - and launches it.
// The BGR frames of rd_detector_enqueue and the frames of the other formats differ in three places, each a condition on fmt below; none of them has been measured the other way.
// scale 2 (rd_detector_enqueue_scaled): planes, pitches and L describe the source frame of 2 iw x 2 ih pixels; a host frame then travels through the slot's
// scaled-source staging (sc_h / sc_bgr, allocated here with the slot's first such frame - the slot is idle: its last frame has been polled) on the same paths.
static long hand_over(rd_detector *d, const char *who, int fmt, const void *const planes[3], const int pitches[3], const PixLayout &L, int on_device, int scale = 1) {
  if (d->next_enqueue - d->next_poll >= d->nslots) exitf(-1, "%s: %d frames already in flight (poll first)\n", who, d->nslots);
  RD_HIP(hipSetDevice(d->device));
  struct timespec ts0; clock_gettime(CLOCK_MONOTONIC, &ts0);
  Slot *s = &d->slots[d->next_enqueue % d->nslots];
  s->seq = d->next_enqueue; s->fmt = fmt; s->scale = scale;
  for (int k = 0; k < 3; k++) { s->pl[k] = NULL; s->pitch[k] = 0; }
  if (scale == 2 && on_device != RD_FRAME_DEVICE && !s->sc_bgr) {
    s->sc_bytes = pix_layout(RD_PIX_BGRA, 2 * d->iw, 2 * d->ih).bytes;      // (16 bytes per detector pixel: the largest of the six layouts)
    RD_HIP(hipMalloc((void **)&s->sc_bgr, s->sc_bytes));
    RD_HIP(hipHostMalloc(&s->sc_h, s->sc_bytes, hipHostMallocDefault));
  }
  uint8_t *const dbuf = scale == 2 ? s->sc_bgr : s->bgr;      // a host frame's way: pinned staging hbuf (pageable frames only), device copy dbuf
  void *const hbuf = scale == 2 ? s->sc_h : s->h_bgr;
  Slot *wait_upload = NULL;
  const bool group = d->zb > 1;
  if (on_device == RD_FRAME_DEVICE) {      // read where they lie (the caller keeps them valid until the frame's poll returned)
    for (int k = 0; k < L.np; k++) { s->pl[k] = (const uint8_t *)planes[k]; s->pitch[k] = pitches[k]; }
  } else {      // host frames: through the slot's buffers, one plane after the other
    for (int k = 0; k < L.np; k++) { s->pl[k] = dbuf + L.off[k]; s->pitch[k] = L.pitch[k]; }
    // Group mode: the frame travels NOW, on a stream of the detector's own (high-priority pool: a hardware queue nobody computes on), not when its group is launched:
    // eight uploads in front of a group's kernels kept that group's stream - a quarter of the device's queues - waiting for the copy engine for 1.6 of its 10.8 ms; and
    // an ordinary stream shares a hardware queue with a group's: 2786-2796 frames/s, the caller waiting 0.35 ms per frame.  No event: group_launch waits for the stream.
    hipStream_t ust = s->st;
    if (group) { if (!d->st_upload) d->st_upload = pooled_stream(d->device); ust = d->st_upload; }
    if (on_device == RD_FRAME_HOST_PINNED) {
      // The caller's planes are page-locked and stay as they are until the frame's poll: the copy engine takes them from there.  (The reference copies every frame into its own
      // pinned page first, oclrect.c:1256 - 6 MB per 1920x1080 frame by the caller's thread, 16 GB/s at full rate on the thread that also launches everything.)
      for (int k = 0; k < L.np; k++) {
        const void *lo = planes[k], *hi = (const char *)planes[k] + (size_t)pitches[k] * (L.rows[k] - 1) + L.row[k];
        bool known = false;      // (one look per range, not per frame: a capture loop reuses its pages)
        for (int e = 0; e < 4 && !known; e++) known = lo >= d->pinned[e][0] && hi <= d->pinned[e][1];
        if (known) continue;
        if (rdjob::memory_type(planes[k]) != hipMemoryTypeHost) { exitf(-1, "%s: RD_FRAME_HOST_PINNED needs pinned host memory (rd_host_alloc, allocatePinnedMemory, hipHostMalloc, hipHostRegister); plane %d at %p is not\n", who, k, planes[k]); }
        const unsigned e = d->pinned_next++ & 3;
        d->pinned[e][0] = lo; d->pinned[e][1] = hi;
      }
      // (The colour conversion reading the pinned buffer over PCIe itself, without the copy engine: 1985-2009 frames/s against 2656-2659 - the kernel then runs at the link's
      //  rate, a millisecond per group, with its blocks resident all the while.  profiles/NOTES_r06.md.)
      if (group) RD_HIP(hipStreamSynchronize(ust));      // (one transfer in the copy engine's queue at a time: the caller waits for the frame before - 0.1 ms where it used to copy for 0.16 - see group_launch)
      for (int k = 0; k < L.np; k++) {
        if (pitches[k] == L.row[k] && L.row[k] == L.pitch[k]) RD_HIP(hipMemcpyAsync(dbuf + L.off[k], planes[k], (size_t)L.row[k] * L.rows[k], hipMemcpyHostToDevice, ust));
        else RD_HIP(hipMemcpy2DAsync(dbuf + L.off[k], L.pitch[k], planes[k], pitches[k], L.row[k], L.rows[k], hipMemcpyHostToDevice, ust));
      }
      d->n_frames_pinned++;
    } else if (!group && fmt == RD_PIX_BGR && scale == 1 && host_buffer_is_pinned(d, planes[0])) {      // (only rd_detector_enqueue's frames ask)
      // The reference's call shape (oclrect_enqueueTask / executeOnce) on a buffer that happens to be page-locked - allocatePinnedMemory of oclhelper.h hands such memory out
      // (oclhelper.c:837-851, poly.cpp:68-69): the copy engine reads it in place, nothing is copied by the caller's thread, and the frame's kernels are launched behind the
      // transfer at once.  The reference's contract - the caller may reuse the buffer as soon as the call returns (oclrect.c:1256 copies it) - is kept by returning only when
      // the engine has read it: waited for at the END of this call (enqueue_launch), after the frame's ~45 launches, by which time it has long happened (6 MB in 0.12 ms).
      RD_HIP(hipMemcpyAsync(s->bgr, planes[0], L.bytes, hipMemcpyHostToDevice, s->st));
      RD_HIP(hipEventRecord(s->ev_upload, s->st));
      wait_upload = s;
      d->n_frames_pinned++;
    } else {
      d->n_frames_copied++;
      UploadJob u;
      u.L = L; u.dst = (char *)hbuf; u.dev = (char *)dbuf; u.st = ust; u.uploaded = 0;
      for (int k = 0; k < 3; k++) { u.src[k] = (const uint8_t *)planes[k]; u.spitch[k] = pitches[k]; }
      if (group) {      // the caller's thread packs, then the frame travels at once
        pack_range(&u, 0, L.bytes);
        if (fmt != RD_PIX_BGR || scale != 1) RD_HIP(hipStreamSynchronize(ust));      // (one transfer queued at a time, as the pinned frames'; a BGR frame's upload is queued behind the one before without this wait)
        RD_HIP(hipMemcpyAsync(dbuf, hbuf, L.bytes, hipMemcpyHostToDevice, ust));
      } else {
        // a single frame: the copy into pinned memory and the upload in pieces, so that a piece travels while the next is being copied (6 MB at 1920x1080:
        // the copy alone takes a fifth of a millisecond of the caller's latency).  With helper threads (armed here: the call that hands a frame over is followed by
        // the poll that waits for one) the pieces are copied side by side and uploaded in order as they complete.
        const bool helpers = d->post_helpers > 0;
        if (helpers) rd_post_helpers_arm();
        const int npieces = helpers ? 16 : 4;
        u.piece = ((L.bytes + npieces - 1) / npieces + 4095) & ~(size_t)4095;
        u.n = (int)((L.bytes + u.piece - 1) / u.piece);      // (<= npieces)
        for (int i = 0; i < u.n; i++) u.ready[i] = 0;
        rd_helpers_run(pack_copy_piece, &u, u.n, upload_progress);
        upload_progress(&u);
        if (u.uploaded != u.n) exitf(-1, "%s: internal error (pieces of the frame left behind)\n", who);
      }
    }
  }
  s->src = s->pl[0]; s->ws = s->pitch[0];
  return enqueue_launch(d, s, wait_upload, ts0);
}

long rd_detector_enqueue(rd_detector *d, const void *frame, int ws, int on_device) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_enqueue: bad handle\n");
  if ((size_t)ws * d->ih > (size_t)d->N * 4) exitf(-1, "rd_detector_enqueue: row stride %d too large for a %dx%d frame\n", ws, d->iw, d->ih);
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) exitf(-1, "rd_detector_enqueue: on_device = %d (0: host memory, 1: device memory, 2: pinned host memory)\n", on_device);
  const void *const planes[3] = { frame, NULL, NULL };
  const int pitches[3] = { ws, 0, 0 };
  return hand_over(d, "rd_detector_enqueue", RD_PIX_BGR, planes, pitches, bgr_layout(ws, d->ih), on_device);
}

long rd_detector_enqueue_planes(rd_detector *d, int format, const void *const planes[3], const int pitches[3], int on_device) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_enqueue_planes: bad handle\n");
  // argument errors: -1, nothing enqueued
  if (format < RD_PIX_BGR || format > RD_PIX_I420 || !planes || !pitches) return -1;
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) return -1;
  if (rdpix::is_yuv(format) && ((d->iw | d->ih) & 1)) return -1;
  const PixLayout L = pix_layout(format, d->iw, d->ih);
  for (int k = 0; k < L.np; k++) if (!planes[k] || pitches[k] < L.row[k]) return -1;
  if (format == RD_PIX_BGR) return rd_detector_enqueue(d, planes[0], pitches[0], on_device);
  return hand_over(d, "rd_detector_enqueue_planes", format, planes, pitches, L, on_device);
}

long rd_detector_enqueue_scaled(rd_detector *d, int format, const void *const planes[3], const int pitches[3], int scale, int on_device) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_enqueue_scaled: bad handle\n");
  if (scale == 1) return rd_detector_enqueue_planes(d, format, planes, pitches, on_device);
  // argument errors: -1, nothing enqueued
  if (scale != 2) return -1;
  if (format < RD_PIX_BGR || format > RD_PIX_I420 || !planes || !pitches) return -1;
  if (on_device != RD_FRAME_HOST && on_device != RD_FRAME_DEVICE && on_device != RD_FRAME_HOST_PINNED) return -1;
  const PixLayout L = pix_layout(format, 2 * d->iw, 2 * d->ih);      // (the source frame: even in both directions, whatever iw and ih are)
  for (int k = 0; k < L.np; k++) if (!planes[k] || pitches[k] < L.row[k]) return -1;
  return hand_over(d, "rd_detector_enqueue_scaled", format, planes, pitches, L, on_device, 2);
}

// device time of a polled frame (counters 1 and 2): the interval its events bracket - a group's is shared by its frames: each counts its part
static void count_device_time(rd_detector *d, const Slot *s) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, s->watch_begin, s->watch_done) == hipSuccess) { d->dev_us += (long)(ms * 1000.0f) / (s->group_n > 0 ? s->group_n : 1); d->dev_frames++; }
}

void *rd_detector_poll(rd_detector *d, double tanAOV) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_poll: bad handle\n");
  if (d->kind == RD_KIND_POLY) exitf(-1, "rd_detector_poll: this is a polyline detector (rd_polyline_detector_create) - its results come from rd_detector_poll_segments\n");
  if (d->next_poll >= d->next_enqueue) exitf(-1, "rd_detector_poll: nothing enqueued\n");
  RD_HIP(hipSetDevice(d->device));
  const int si = (int)(d->next_poll % d->nslots);
  Slot *s = &d->slots[si];
  void *r = NULL, *segs = NULL; int ns = 0;
  if (s->pending_sparse) sparse_flush(d, si);       // (an incomplete group: the caller wants a result before handing over more frames)
  if (s->pending_dense) group_launch(d, si / d->zb * d->zb);
  pthread_mutex_lock(&d->tan_mu);
  d->tan_aov = tanAOV; d->have_tan = 1;            // what workers and the device post-process of later frames run ahead with
  pthread_cond_broadcast(&d->tan_cv);
  pthread_mutex_unlock(&d->tan_mu);
  if (d->nworkers > 0) {
    pthread_mutex_lock(&s->mu);
    while (s->state != 2) pthread_cond_wait(&s->cv, &s->mu);
    r = s->result; segs = s->res_segs; ns = s->res_nsegs;
    const double used = s->result_tan;
    s->result = NULL; s->res_segs = NULL; s->state = 0;
    pthread_mutex_unlock(&s->mu);
    if (used != tanAOV) {      // the worker ran ahead with another aperture: redo with the requested one
      free(r); free(segs);
      r = slot_rectangles(d, s, tanAOV, &segs, &ns);
    }
  } else {
    if (d->post_helpers && !(s->post_mode && s->post_tan == tanAOV)) rd_post_helpers_arm();      // (they wake while the device is still busy with the frame: rd_post.c; not for a frame whose rectangles the device computes)
    static const int trace_poll = RD_LAB_INT("RD_TRACE_POLL", 0);      // (1: timings, 2: wait by querying instead of hipEventSynchronize)
    struct timespec t0, t1, t2, t3; clock_gettime(CLOCK_MONOTONIC, &t0);
    if (trace_poll == 2) { while (hipEventQuery(s->watch_done) == hipErrorNotReady) sched_yield(); }
    else RD_HIP(hipEventSynchronize(s->watch_done));
    clock_gettime(CLOCK_MONOTONIC, &t1);
    slot_finish_device(d, s);
    clock_gettime(CLOCK_MONOTONIC, &t2);
    r = slot_rectangles(d, s, tanAOV, &segs, &ns);
    clock_gettime(CLOCK_MONOTONIC, &t3);
    if (trace_poll) {
      static double a, b, c; static int n;
      a += (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3; b += (t2.tv_sec - t1.tv_sec) * 1e6 + (t2.tv_nsec - t1.tv_nsec) * 1e-3; c += (t3.tv_sec - t2.tv_sec) * 1e6 + (t3.tv_nsec - t2.tv_nsec) * 1e-3;
      if (++n % 100 == 0) { fprintf(stderr, "poll: wait %.1f us, finish %.1f us, rectangles %.1f us (average of 100)\n", a / 100, b / 100, c / 100); a = b = c = 0; }
    }
  }
  count_device_time(d, s);
  free(d->last_segs);
  d->last_segs = segs; d->last_nsegs = ns;
  d->last_polled_slot = si;
  d->next_poll++;
  return r;
}

// The frame of the most recently polled slot as a job of a service takes it (rd_rectify.hip, rd_annotate.hip, rd_composite.hip, rd_match.hip): format, planes and row strides as
// hand_over left them - device pointers in every case, which a service's stream may read at once: the poll has waited for the frame's last kernel - at the size it
// came in.  own: a host or pinned frame's copy in the slot's own buffer (bgr, or sc_bgr at scale 2), which the next frame of this slot overwrites and no job may write.
// false: nothing polled yet, or `service` is no live service of this kind on the detector's device; cap: the most items one of its jobs takes.
struct PolledFrame { int fmt, iw, ih, scale, cap; const void *planes[3]; const int *pitch; bool own; };
static bool polled_frame(rd_detector *d, const char *who, const void *service, uint32_t magic, PolledFrame *f) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "%s: bad handle\n", who);
  f->cap = rdjob::service_capacity(service, magic, d->device);
  if (d->last_polled_slot < 0 || f->cap < 0) return false;
  const Slot *s = &d->slots[d->last_polled_slot];
  f->fmt = s->fmt; f->scale = s->scale; f->iw = s->scale * d->iw; f->ih = s->scale * d->ih; f->pitch = s->pitch;
  for (int k = 0; k < 3; k++) f->planes[k] = s->pl[k];
  f->own = s->pl[0] == s->bgr || (s->sc_bgr && s->pl[0] == s->sc_bgr);
  return true;
}
// A frame that came in at scale 2 takes quads in detector coordinates: a copy of the job's n items (`size` bytes each, a quad's 8 doubles first), each corner mapped to
// the source's (pixel centres at integers: detector pixel x covers source pixels 2x and 2x+1, centre 2x + 0.5), to be freed behind the enqueue - which takes what it
// needs before it returns.  NULL: the job takes the caller's items (scale 1, or arguments that the service will refuse)
static_assert(offsetof(rd_comp_item, quad) == 0, "an item begins with its quad");
static void *mapped_to_source(const PolledFrame *f, const char *who, const void *items, int n, size_t size) {
  if (f->scale != 2 || !items || n < 1 || n > f->cap) return NULL;
  char *m = (char *)malloc((size_t)n * size);
  if (!m) exitf(-1, "%s: out of memory\n", who);
  memcpy(m, items, (size_t)n * size);
  for (int k = 0; k < n; k++) {
    double *q = (double *)(m + k * size);
    for (int i = 0; i < 8; i++) q[i] = q[i] * 2.0 + 0.5;
  }
  return m;
}
// Rectified patches from the polled frame; nothing of the slot is written.
long rd_detector_rectify_polled(rd_detector *d, rd_rectifier *r, const double *quads, int n, void *out, int out_kind) {
  PolledFrame f;
  if (!polled_frame(d, "rd_detector_rectify_polled", r, RD_MAGIC_RECTIFIER, &f)) return -1;
  void *m = mapped_to_source(&f, "rd_detector_rectify_polled", quads, n, 8 * sizeof(double));
  const long q = rd_rectifier_enqueue(r, f.fmt, f.planes, f.pitch, f.iw, f.ih, RD_FRAME_DEVICE, m ? (const double *)m : quads, n, out, out_kind);
  free(m);
  return q;
}
// Matched quads of the polled frame; nothing of the slot is written.
long rd_detector_match_polled(rd_detector *d, rd_matcher *m, const double *quads, int n, int flags) {
  PolledFrame f;
  if (!polled_frame(d, "rd_detector_match_polled", m, RD_MAGIC_MATCHER, &f)) return -1;
  void *mq = mapped_to_source(&f, "rd_detector_match_polled", quads, n, 8 * sizeof(double));
  const long q = rd_matcher_enqueue(m, f.fmt, f.planes, f.pitch, f.iw, f.ih, RD_FRAME_DEVICE, mq ? (const double *)mq : quads, n, flags);
  free(mq);
  return q;
}
// Annotated frames: a caller's device frame may be drawn into in place; the slot's own copy needs a destination.
long rd_detector_annotate_polled(rd_detector *d, rd_annotator *a, const rd_annot_prim *prims, int n, int flags, void *const out_planes[3], const int out_pitches[3], int out_kind) {
  PolledFrame f;
  if (!polled_frame(d, "rd_detector_annotate_polled", a, RD_MAGIC_ANNOTATOR, &f) || (f.own && !out_planes)) return -1;
  return rd_annotator_enqueue(a, f.fmt, f.planes, f.pitch, f.iw, f.ih, RD_FRAME_DEVICE, prims, n, flags, out_planes, out_pitches, out_kind);
}
// Composited quads: in place or into a destination by the annotator's rule.
long rd_detector_composite_polled(rd_detector *d, rd_compositor *c, const rd_comp_item *items, int n, const void *patches, int npatches, int patches_kind,
                                  void *const out_planes[3], const int out_pitches[3], int out_kind) {
  PolledFrame f;
  if (!polled_frame(d, "rd_detector_composite_polled", c, RD_MAGIC_COMPOSITOR, &f) || (f.own && !out_planes)) return -1;
  void *m = mapped_to_source(&f, "rd_detector_composite_polled", items, n, sizeof(rd_comp_item));
  const long q = rd_compositor_enqueue(c, f.fmt, f.planes, f.pitch, f.iw, f.ih, RD_FRAME_DEVICE, m ? (const rd_comp_item *)m : items, n, patches, npatches, patches_kind, out_planes, out_pitches, out_kind);
  free(m);
  return q;
}

void rd_detector_drain(rd_detector *d) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_drain: bad handle\n");
  RD_HIP(hipSetDevice(d->device));
  if (d->batch > 1) for (int i = 0; i < d->nslots; i += d->batch) sparse_flush(d, i);
  if (d->zb > 1) for (long q = d->next_poll; q < d->next_enqueue; q++) {      // (sequence order)
    const int si = (int)(q % d->nslots);
    if (d->slots[si].pending_dense) group_launch(d, si / d->zb * d->zb);
  }
  for (int i = 0; i < d->nslots; i++) RD_HIP(hipStreamSynchronize(d->slots[i].st));
}

void *rd_detector_poll_segments(rd_detector *d, int32_t *ids_out) {
  if (!d || d->magic != MAGIC_RECT) exitf(-1, "rd_detector_poll_segments: bad handle\n");
  if (d->kind != RD_KIND_POLY) exitf(-1, "rd_detector_poll_segments: this is a rectangle detector (rd_detector_create) - its results come from rd_detector_poll\n");
  if (d->next_poll >= d->next_enqueue) exitf(-1, "rd_detector_poll_segments: nothing enqueued\n");
  RD_HIP(hipSetDevice(d->device));
  const int si = (int)(d->next_poll % d->nslots);
  Slot *s = &d->slots[si];
  const size_t N = (size_t)d->N;
  if (s->pending_dense) group_launch(d, si / d->zb * d->zb);      // (an incomplete group: the caller wants a result before handing over more frames)
  RD_HIP(hipEventSynchronize(s->watch_done));
  // the single-block polyline kernel gave up on this frame (on-chip tables too small): the stage again in multi-launch form, on the slot's own stream (the
  // frame is finished; its slot is not reused before this poll returns); two such frames in a row send the stream's later frames to the multi-launch form
  const bool over = s->poly_mode == 1 && s->h_pack[RD_PACK_GAVE_UP] != 0;
  if (s->poly_mode == 1) { if (over) { if (++d->overflow_streak >= 2) d->poly_overflows = 1; } else d->overflow_streak = 0; }
  if (!s->st_redo) s->st_redo = make_redo_stream();
  if (over || (d->force_redo & 1)) {
    rdk::polyline(s->st_redo, s->frame, 1, d->N * 16, 0, d->p_minerror, d->p_size, d->iw, d->ih, 0);
    rdk::polyline_handoff(s->st_redo, s->frame, 1, d->handoff_rec);
    rdrt::check_launch("polyline frame, multi-launch repeat");
    RD_HIP(hipStreamSynchronize(s->st_redo));
    d->n_redo++;
  }
  const int n = s->h_pack[RD_PACK_RECORDS];
  void *out = malloc((size_t)(n + 1) * 56);
  if (!out) exitf(-1, "rd_detector_poll_segments: out of memory\n");
  if (n + 1 <= d->handoff_rec) memcpy(out, s->h_pack + RD_PACK_RECORDS, (size_t)(n + 1) * 56);
  else { slot_fetch(s, out, s->lslist, (size_t)(n + 1) * 56); d->n_long_lists++; }      // (nothing is dropped: the rest of a long list comes from the device)
  if (ids_out) {      // the dense id plane, only on request: from the slot's compact scratch
    rdk::polyline_ids(s->st_redo, s->frame, 1, (int)N);
    RD_HIP(hipMemcpyAsync(ids_out, s->lsid, N * 4, hipMemcpyDeviceToHost, s->st_redo));
    RD_HIP(hipStreamSynchronize(s->st_redo));
  }
  count_device_time(d, s);
  d->last_polled_slot = si;
  d->next_poll++;
  return out;
}

}  // extern "C"
