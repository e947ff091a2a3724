// rectdetect-mi355x: the stages' test taps - the device post-process, the polyline stage, the region stage and the vote stage on inputs of the caller, each on a stream and
// buffers of its own.  None touches a detector; what a tap shares with the frame path it calls (rd_detector.h), it does not restate.
#include "rd_detector.h"

extern "C" {

// ---- test taps of the device post-process (neither is on the frame path)
void rd_post_device_limits(int32_t out[8]) { rdk::post_limits(out); }

// rd_postprocess_planes' device twin: the caller's list, boundary plane and vote table through k_sample_segments and the three launches of
// rdk::post_device, once, on a stream, scratch and result block of its own; the result block is packed by the code a poll uses.
// The caller's plane holds a component id per pixel, as the default build's frame path leaves it.  A -DRD_BOUNDARY_FLATTEN=0 build reads
// the plane as a forest of pixel indices and would follow the caller's ids as links: the tap refuses to run there.
void *rd_postprocess_planes_device(int device, const void *segs, const int32_t *boundary, const int32_t *table, int iw, int ih, double tanAOV, int32_t info[8]) {
  if (!RD_BOUNDARY_FLATTEN) exitf(-1, "rd_postprocess_planes_device: needs a build with RD_BOUNDARY_FLATTEN=1 (the plane holds ids, not links)\n");
  RD_HIP(hipSetDevice(device));
  int n = ((const int *)segs)[0];
  if (n < 0) n = 0;
  const size_t N = (size_t)iw * ih;
  const int nentry = iw * ih * 4 / 5;
  char *d_ls = dnew<char>((size_t)(n + 1) * 56);
  int *d_boundary = dnew<int>(N), *d_table = dnew<int>((size_t)nentry * 5), *d_probes = dnew<int>((size_t)(n + 1) * RD_PROBE_INTS);
  int *d_scratch = dnew<int>(rdk::post_scratch_ints());
  int *h_post = NULL, *h_post_dev = NULL;
  const size_t out_bytes = rdk::post_out_ints() * sizeof(int);
  RD_HIP(hipHostMalloc((void **)&h_post, out_bytes, hipHostMallocDefault)); memset(h_post, 0, out_bytes);
  RD_HIP(hipHostGetDevicePointer((void **)&h_post_dev, h_post, 0));
  hipStream_t st = NULL;
  RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  RD_HIP(hipMemcpyAsync(d_ls, segs, (size_t)(n + 1) * 56, hipMemcpyHostToDevice, st));
  RD_HIP(hipMemcpyAsync(d_boundary, boundary, N * sizeof(int), hipMemcpyHostToDevice, st));
  RD_HIP(hipMemcpyAsync(d_table, table, (size_t)nentry * 5 * sizeof(int), hipMemcpyHostToDevice, st));
  RD_HIP(hipMemsetAsync(d_probes, 0, (size_t)(n + 1) * RD_PROBE_INTS * sizeof(int), st));
  rdk::PolyFrame f;
  memset(&f, 0, sizeof(f));
  f.lslist = d_ls; f.boundary = d_boundary; f.table = d_table; f.probes = d_probes; f.pack = NULL;
  f.post_scratch = d_scratch; f.post_out = h_post_dev;
  rdk::sample_segments(st, &f, 1, n + 1, iw, ih, nentry, 0);
  rdk::post_device(st, &f, 1, n + 1, iw, ih, tanAOV);
  rdrt::check_launch("rd_postprocess_planes_device");
  RD_HIP(hipStreamSynchronize(st));
  if (info) { for (int i = 0; i < 8; i++) info[i] = 0; info[0] = h_post[0]; info[1] = h_post[1]; }
  void *ret = h_post[1] == 0 ? (void *)post_block_rectangles(h_post) : NULL;
  RD_HIP(hipStreamDestroy(st));
  RD_HIP(hipHostFree(h_post));
  dfree(d_scratch); dfree(d_probes); dfree(d_table); dfree(d_boundary); dfree(d_ls);
  return ret;
}

// ---- test taps of the polyline stage (neither is on the frame path)
void rd_polyline_limits(int32_t out[4]) { rdk::poly_limits(out); }

// oclpolyline_execute's twin with the form of the stage chosen by the caller: the caller's 0/1 plane through rdk::polyline and rdk::polyline_ids,
// once, on a stream and scratch of its own.  form 1 is the single-block kernel alone: where it gives up (ctr_out[25]) nothing repeats the stage,
// the caller sees the flag and whatever list the kernel left.
int rd_polyline_planes_device(int device, const int32_t *mask, int iw, int ih, int ring_nonzero, float minerror, int size_thre, int lslist_bytes, int form,
                              void *lslist_out, int32_t *ids_out, int32_t ctr_out[64]) {
  // (the stage's scratch is sized for lists of up to 16 bytes per pixel, what every caller in the reference passes; two records are the least a list holds)
  if (!mask || !lslist_out || !ids_out || !ctr_out || iw < 5 || ih < 5 || iw > 0xffff || ih > 0x7fff || (form != 0 && form != 1) || size_thre < 0 ||
      lslist_bytes < 2 * 56 || (long long)lslist_bytes > (long long)iw * ih * 16) return -1;
  RD_HIP(hipSetDevice(device));
  const size_t N = (size_t)iw * ih;
  int *d_mask = dnew<int>(N), *d_ids = dnew<int>(N);
  char *d_ls = dnew<char>((size_t)lslist_bytes + 56);
  rdk::PolyScratch *ps = rdk::poly_scratch_create(iw, ih);
  hipStream_t st = NULL;
  RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  RD_HIP(hipMemcpyAsync(d_mask, mask, N * sizeof(int), hipMemcpyHostToDevice, st));
  RD_HIP(hipMemsetAsync(d_ls, 0, (size_t)lslist_bytes + 56, st));
  rdk::PolyFrame f;
  memset(&f, 0, sizeof(f));
  f.ps = *ps; f.in = d_mask; f.lslist = d_ls; f.ids = d_ids;
  rdk::polyline(st, &f, 1, lslist_bytes, ring_nonzero ? 1 : 0, minerror, size_thre, iw, ih, form);
  rdk::polyline_ids(st, &f, 1, (int)N);
  rdrt::check_launch("rd_polyline_planes_device");
  RD_HIP(hipMemcpyAsync(lslist_out, d_ls, (size_t)lslist_bytes, hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(ids_out, d_ids, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(ctr_out, rdk::poly_scratch_counters(ps), 64 * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  RD_HIP(hipStreamDestroy(st));
  rdk::poly_scratch_destroy(ps);
  dfree(d_ls); dfree(d_ids); dfree(d_mask);
  return 0;
}

// ---- test taps of the region stage (neither is on the frame path)
void rd_region_limits(int iw, int ih, int32_t out[32]) { rdk::region_limits(iw, ih, out); }

// an int plane (non-zero / positive = set) as the bit plane the region kernels read: ceil(iw / 64) words per row, bits beyond the row's end clear
static void pack_bit_plane(unsigned long long *bits, const int32_t *plane, int iw, int ih, int positive_only) {
  const int wpr = (iw + 63) / 64;
  memset(bits, 0, ((size_t)wpr * ih + 8) * sizeof(*bits));
  for (int y = 0; y < ih; y++)
    for (int x = 0; x < iw; x++) {
      const int v = plane[(size_t)y * iw + x];
      if (positive_only ? v > 0 : v != 0) bits[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
    }
}

// The frame path's region stage on planes of the caller: stage 0 = region_stage (what frame_regions calls) from the merge's inputs, with a budget of the caller's or
// (launches = 0) the frame path's - RD_REGION_FIRST_BUDGET launches, then region_ladder -; stage 1 = its second half, from the absorption's inputs.  Either way
// region_absorb_slow (what frame_absorb_slow calls) where the status word asks for it or the caller forces it.  Once, on a stream, planes and scratch of its own.
int rd_region_planes_device(int device, int stage, int iw, int ih, const int32_t *pix, const int32_t *mask, const int32_t *edge, int launches,
                            const int32_t *region0_in, const int32_t *rsize_in, int force_slow,
                            int32_t *region0_out, int32_t *rsize_out, int32_t *region_out, int32_t *boundarysrc_out, int32_t *boundary_out, int32_t info[RD_REGION_INFO_INTS]) {
  if (!region0_out || !rsize_out || !region_out || !boundarysrc_out || !boundary_out || !info || (stage != 0 && stage != 1)) return -1;
  if (iw < 16 || ih < 16 || (long long)iw * ih >= (1ll << 25)) return -1;      // (rd_detector_create's limits)
  const size_t N = (size_t)iw * ih;
  if (stage == 0) {
    if (!pix || !mask || !edge || launches < 0 || (launches & 1) || launches == 1 || launches > RD_REGION_MAX_LAUNCHES) return -1;
  } else {
    if (!region0_in || !rsize_in) return -1;
    for (size_t p = 0; p < N; p++)
      if (region0_in[p] < 0 || (size_t)region0_in[p] >= N || rsize_in[p] < 0 || rsize_in[p] >= (1 << 26)) return -1;      // (labels index the size table; the tail's words hold sizes in 26 bits)
  }
  RD_HIP(hipSetDevice(device));
  const int n = (int)N, nentry = n * 4 / 5;
  const size_t nbits = (size_t)((iw + 63) / 64) * ih + 8;
  int *d_pix = dnew<int>(N), *d_region0 = dnew<int>(N), *d_rsize = dnew<int>(N), *d_region = dnew<int>(N), *d_bsrc = dnew<int>(N), *d_boundary = dnew<int>(N);
  int *d_scratch2 = dnew<int>(N * 3 + 256), *d_d2s = dnew<int>(RD_D2_SCRATCH_INTS(N)), *d_table = dnew<int>(N * 4), *d_claim = dnew<int>(N), *d_tlist = dnew<int>(N);
  unsigned long long *d_mm = dnew<unsigned long long>(nbits), *d_sb = dnew<unsigned long long>(nbits);
  int *flags = d_scratch2 + N, *status = flags + RD_REGION_STATUS_AT;
  const RegionPlanes planes = { d_pix, d_mm, d_sb, d_region0, d_rsize, d_region, d_scratch2, d_d2s, d_bsrc, d_boundary, d_table, d_claim, d_tlist };
  hipStream_t st = NULL;
  RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  rdk::reduce_ls_init(st, d_table, d_claim, d_tlist, nentry);
  RD_HIP(hipMemsetAsync(flags, 0, 256 * sizeof(int), st));
  for (int i = 0; i < RD_REGION_INFO_INTS; i++) info[i] = 0;
  int budget = 0, settled = 1;
  if (stage == 0) {
    unsigned long long *h_bits = (unsigned long long *)malloc(nbits * sizeof(*h_bits));
    if (!h_bits) exitf(-1, "rd_region_planes_device: out of memory\n");
    RD_HIP(hipMemcpyAsync(d_pix, pix, N * sizeof(int), hipMemcpyHostToDevice, st));
    pack_bit_plane(h_bits, mask, iw, ih, 0);
    RD_HIP(hipMemcpyAsync(d_mm, h_bits, nbits * sizeof(*h_bits), hipMemcpyHostToDevice, st));
    RD_HIP(hipStreamSynchronize(st));      // (the one host buffer packs both planes)
    pack_bit_plane(h_bits, edge, iw, ih, 1);
    RD_HIP(hipMemcpyAsync(d_sb, h_bits, nbits * sizeof(*h_bits), hipMemcpyHostToDevice, st));
    RD_HIP(hipStreamSynchronize(st));
    free(h_bits);
    auto still_after = [&](int b) {      // the stage with b launches of the merge; the flag of the last one
      int still = 0;
      region_stage(st, planes, iw, ih, b, 1, 0);
      rdrt::check_launch("rd_region_planes_device");
      RD_HIP(hipMemcpyAsync(&still, flags + b - 1, sizeof(int), hipMemcpyDeviceToHost, st));
      RD_HIP(hipStreamSynchronize(st));
      return still;
    };
    budget = launches ? launches : RD_REGION_FIRST_BUDGET;
    settled = still_after(budget) == 0;
    if (!launches && !settled) { const LadderEnd e = region_ladder(still_after); budget = e.budget; settled = e.settled; }
  } else {
    RD_HIP(hipMemcpyAsync(d_region0, region0_in, N * sizeof(int), hipMemcpyHostToDevice, st));
    RD_HIP(hipMemcpyAsync(d_rsize, rsize_in, N * sizeof(int), hipMemcpyHostToDevice, st));
    region_stage(st, planes, iw, ih, 0, 1, 0, 0);      // (not from the merge: the absorption's count word is not known to be zero)
    rdrt::check_launch("rd_region_planes_device");
  }
  RD_HIP(hipMemcpyAsync(info, flags, (size_t)RD_REGION_MAX_LAUNCHES * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(info + RD_REGION_MAX_LAUNCHES + 2, status, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  info[RD_REGION_MAX_LAUNCHES] = budget; info[RD_REGION_MAX_LAUNCHES + 1] = settled;
  if (info[RD_REGION_MAX_LAUNCHES + 2] != 0 || force_slow) {      // as frame_absorb_slow
    info[RD_REGION_MAX_LAUNCHES + 7] = region_absorb_slow(st, planes, iw, ih);
    rdrt::check_launch("rd_region_planes_device, slow absorption");
    info[RD_REGION_MAX_LAUNCHES + 6] = 1;
  }
  if (!RD_BOUNDARY_FLATTEN) rdk::label8_flatten(st, d_boundary, n);      // (a tuning build leaves the components as a forest, as on the frame path: flattened where the plane is looked at)
  RD_HIP(hipMemcpyAsync(region0_out, d_region0, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(rsize_out, d_rsize, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(region_out, d_region, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(boundarysrc_out, d_bsrc, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(boundary_out, d_boundary, N * sizeof(int), hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  RD_HIP(hipStreamDestroy(st));
  dfree(d_sb); dfree(d_mm); dfree(d_tlist); dfree(d_claim); dfree(d_table); dfree(d_d2s); dfree(d_scratch2);
  dfree(d_boundary); dfree(d_bsrc); dfree(d_region); dfree(d_rsize); dfree(d_region0); dfree(d_pix);
  return 0;
}

// ---- test taps of the vote stage (neither is on the frame path)
void rd_votes_limits(int32_t out[RD_VOTES_LIMITS_INTS]) { rdk::votes_limits(out); }

// The frame path's sparse tail on masks and boundary planes of the caller: per step rdk::polyline, rdk::polyline_ids, rdk::reduce_ls and rdk::sample_segments, one set of
// launches for the step's nb frames.  Frame z keeps its scratch, list, table, claim and tlist from step to step, as a slot does from frame to frame; how a step undoes
// the one before is the caller's choice (clean).  The planes hold ids, not links: refused in a -DRD_BOUNDARY_FLATTEN=0 build, as rd_postprocess_planes_device is.
int rd_votes_planes_device(int device, int iw, int ih, int nsteps, int nb, const int32_t *masks, const int32_t *boundaries,
                           const int32_t *ring_nonzero, const float *minerror, const int32_t *size_thre, const int32_t *form, int clean,
                           int max_records, int pack_records, const int32_t *rflags, int32_t guard, int probes_ints, int pack_ints,
                           int32_t *ids_out, void *lslist_out, int32_t *ctr_out, int32_t *table_out, int32_t *tlist_out, int32_t *claim_out, int32_t *probes_out, int32_t *pack_out) {
  if (!RD_BOUNDARY_FLATTEN) exitf(-1, "rd_votes_planes_device: needs a build with RD_BOUNDARY_FLATTEN=1 (the plane holds ids, not links)\n");
  if (!masks || !boundaries || !ring_nonzero || !minerror || !size_thre || !form || !rflags || !ids_out || !lslist_out || !ctr_out || !table_out || !tlist_out || !claim_out ||
      !probes_out || !pack_out) return -1;
  if (iw < 16 || ih < 16 || (long long)iw * ih >= (1ll << 25) || nsteps < 1 || nb < 1 || nb > RD_MAXB || (clean != 0 && clean != 1)) return -1;      // (rd_detector_create's limits)
  // the sampling kernel's first RD_PACK_STATUS + RD_PACK_STATUS_INTS threads write the block's counters, flags, status words and header record, and the launch is sized by
  // max_records * 15 threads: four records' threads cover them without counting on the launch's rounding to whole blocks, the tap asks for one more; the header record
  // needs room in the block
  if (max_records < 5 || pack_records < 1 || (long long)probes_ints < (long long)max_records * RD_PROBE_INTS ||
      (long long)pack_ints < RD_PACK_RECORDS + (long long)pack_records * (RD_REC_INTS + RD_PROBE_INTS)) return -1;
  for (int s = 0; s < nsteps; s++)
    if ((form[s] != 0 && form[s] != 1) || size_thre[s] < 0) return -1;
  RD_HIP(hipSetDevice(device));
  const size_t N = (size_t)iw * ih;
  const int n = (int)N, nentry = n * 4 / 5;
  const size_t ls_bytes = N * 16;
  // what frame z keeps: a scratch region plane with its marks and components (the planes of the labelling call whose last kernel undoes the tables), table, claim, tlist -
  // one allocation, frame z's part z * zs bytes behind frame 0's, as a slot's planes lie
  const size_t keep_ints = ((3 * N + (size_t)nentry * 7 + 1) + 63) / 64 * 64, zs = keep_ints * sizeof(int);
  int *d_keep = dnew<int>(keep_ints * nb);
  int *k_region = d_keep, *k_marks = k_region + N, *k_label = k_marks + N, *k_table = k_label + N, *k_claim = k_table + (size_t)nentry * 5, *k_tlist = k_claim + nentry;
  int *d_rflags = dnew<int>((size_t)nb * 256);
  hipStream_t st = NULL;
  RD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  RD_HIP(hipMemsetAsync(d_keep, 0, keep_ints * nb * sizeof(int), st));
  RD_HIP(hipMemcpyAsync(d_rflags, rflags, (size_t)nb * 256 * sizeof(int), hipMemcpyHostToDevice, st));
  rdk::PolyScratch *ps[RD_MAXB];
  rdk::PolyFrame f[RD_MAXB];
  int *d_mask[RD_MAXB], *d_boundary[RD_MAXB], *d_ids[RD_MAXB], *d_probes[RD_MAXB], *h_pack[RD_MAXB];
  char *d_ls[RD_MAXB];
  for (int z = 0; z < nb; z++) {
    ps[z] = rdk::poly_scratch_create(iw, ih);
    d_mask[z] = dnew<int>(N); d_boundary[z] = dnew<int>(N); d_ids[z] = dnew<int>(N); d_probes[z] = dnew<int>((size_t)probes_ints);
    d_ls[z] = dnew<char>(ls_bytes + 56);
    RD_HIP(hipMemsetAsync(d_ls[z], 0, ls_bytes + 56, st));
    int *pack_dev = NULL;
    RD_HIP(hipHostMalloc((void **)&h_pack[z], (size_t)pack_ints * sizeof(int), hipHostMallocDefault));
    RD_HIP(hipHostGetDevicePointer((void **)&pack_dev, h_pack[z], 0));
    memset(&f[z], 0, sizeof(f[z]));
    f[z].ps = *ps[z]; f[z].in = d_mask[z]; f[z].lslist = d_ls[z]; f[z].ids = d_ids[z]; f[z].boundary = d_boundary[z];
    f[z].table = k_table + z * keep_ints; f[z].claim = k_claim + z * keep_ints; f[z].tlist = k_tlist + z * keep_ints;
    f[z].probes = d_probes[z]; f[z].pack = pack_dev; f[z].rflags = d_rflags + (size_t)z * 256;
    rdk::reduce_ls_init(st, f[z].table, f[z].claim, f[z].tlist, nentry);
  }
  for (int s = 0; s < nsteps; s++) {
    for (int z = 0; z < nb; z++) {
      const size_t at = (size_t)s * nb + z;
      RD_HIP(hipMemcpyAsync(d_mask[z], masks + at * N, N * sizeof(int), hipMemcpyHostToDevice, st));
      RD_HIP(hipMemcpyAsync(d_boundary[z], boundaries + at * N, N * sizeof(int), hipMemcpyHostToDevice, st));
      RD_HIP(hipMemsetD32Async((hipDeviceptr_t)d_probes[z], guard, (size_t)probes_ints, st));
      for (int i = 0; i < pack_ints; i++) h_pack[z][i] = guard;      // (the step before has been waited for)
    }
    // clean 1: the frame path's order - the boundary labelling, whose last kernel undoes the tables' entries, then votes that are told so
    if (clean) rdk::label8_boundary(st, k_label, k_marks, k_region, iw, ih, k_table, k_claim, k_tlist, nb, zs, RD_BOUNDARY_FLATTEN);
    rdk::polyline(st, f, nb, (int)ls_bytes, ring_nonzero[s] ? 1 : 0, minerror[s], size_thre[s], iw, ih, form[s]);
    rdk::polyline_ids(st, f, nb, n);
    rdk::reduce_ls(st, f, nb, iw, ih, nentry, clean);
    rdk::sample_segments(st, f, nb, max_records, iw, ih, nentry, pack_records);
    rdrt::check_launch("rd_votes_planes_device");
    for (int z = 0; z < nb; z++) {
      const size_t at = (size_t)s * nb + z;
      RD_HIP(hipMemcpyAsync(ids_out + at * N, d_ids[z], N * sizeof(int), hipMemcpyDeviceToHost, st));
      RD_HIP(hipMemcpyAsync((char *)lslist_out + at * ls_bytes, d_ls[z], ls_bytes, hipMemcpyDeviceToHost, st));
      RD_HIP(hipMemcpyAsync(ctr_out + at * 64, rdk::poly_scratch_counters(ps[z]), 64 * sizeof(int), hipMemcpyDeviceToHost, st));
      RD_HIP(hipMemcpyAsync(table_out + at * nentry * 5, f[z].table, (size_t)nentry * 5 * sizeof(int), hipMemcpyDeviceToHost, st));
      RD_HIP(hipMemcpyAsync(claim_out + at * nentry, f[z].claim, (size_t)nentry * sizeof(int), hipMemcpyDeviceToHost, st));
      RD_HIP(hipMemcpyAsync(tlist_out + at * (nentry + 1), f[z].tlist, ((size_t)nentry + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
      RD_HIP(hipMemcpyAsync(probes_out + at * probes_ints, d_probes[z], (size_t)probes_ints * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    RD_HIP(hipStreamSynchronize(st));
    for (int z = 0; z < nb; z++) memcpy(pack_out + ((size_t)s * nb + z) * pack_ints, h_pack[z], (size_t)pack_ints * sizeof(int));
  }
  RD_HIP(hipStreamDestroy(st));
  for (int z = 0; z < nb; z++) {
    RD_HIP(hipHostFree(h_pack[z]));
    dfree(d_ls[z]); dfree(d_probes[z]); dfree(d_ids[z]); dfree(d_boundary[z]); dfree(d_mask[z]);
    rdk::poly_scratch_destroy(ps[z]);
  }
  dfree(d_rflags); dfree(d_keep);
  return 0;
}

}  // extern "C"
