// rectdetect-mi355x: decoded quads for gfx950 - the second launch of a code job: from the G plane the tensor kernel wrote (rd_k_tensor.hip, { U8, NHWC, GRAY, m }) to
// one rd_code per quad.  The arithmetic is the contract in include/rectdetect_hip.h ("decoded quads").
//
// Launch shape: one block of 16 waves per quad, everything after the G plane in this one launch; no global atomics, nothing for the stream to zero - the record is
// written whole by one lane (an invalid quad's 48 zero bytes by six).  A job is a handful of blocks, so what a block costs is the number of trips to memory one after
// the other, not the work: the first form - a wave per cell, lanes striding over the cell's rectangle, shuffles - made 16 cells x 3 rows of DEPENDENT byte loads per
// wave and took 31 us for ten 128 x 128 quads (profiles/NOTES_code.md); this one makes one trip for a patch of up to 128 x 128.
//   A. cell sums.  The quad's plane is read as 16-byte words from the 16-byte boundary at or below its first byte, one word per thread and pass (1024 threads:
//      16 KB a pass), bytes in front of the plane and behind it skipped.  A thread walks its 16 pixels in raster order - x, y and the two cell coordinates kept
//      incrementally, one division where the walk starts and one per row it enters; f = (2i+1)*C - 2*pw*cx is the contract's fx - and adds a run of counted pixels
//      of one cell as cnt << 32 | sg with ONE 64-bit LDS atomic when the cell changes (sg <= 205 * 205 * 255 < 2^32: no carry into cnt).  Integer sums: any order
//      gives the same bits.
//   B. decision in wave 0.  M = 256 * sg / cnt (unsigned), lo, hi and margin by shuffles over the at most 144 cells (three per lane); the payload word is one 64-lane
//      ballot with lane = r*n + c (n = 8 uses bit 63), the ring count the popcounts of three more; the rotations are three more ballots, each lane picking its bit
//      out of the word before - a wave-uniform register, no table needed.
//   C. search.  All 1024 threads stride over the dictionary (4 entries each at most); a thread keeps the smallest key dist << 14 | id << 2 | k - which makes the tie
//      rule free - and the smallest dist among the ids that are not its best one.  Two threads never hold the same id, so merging two such pairs is exact: the
//      loser's best is a candidate for `second`.  Shuffles, then sixteen pairs through LDS.
#include "rd_device.h"
#include "rd_kernels.h"
#include "rectdetect_hip.h"
#include "rd_code_tile.h"

namespace {

constexpr int WAVES = RD_CODE_WAVES, NT = RD_WAVE * WAVES, MAXCELLS = RD_CODE_MAX_CELLS, NONE = RD_CODE_NONE, WORD = RD_CODE_PLANE_PAD;
constexpr uint32_t KEY_NONE = (uint32_t)NONE << 14 | 0x3fffu;      // no entry: its dist reads NONE
static_assert(sizeof(rd_code) == 48 && RD_CODE_MAX_DICT <= 1 << 12 && RD_CODE_MAX_N * RD_CODE_MAX_N == RD_WAVE, "the key's fields; a payload bit per lane");
static_assert((RD_CODE_MAX_N + 2 * RD_CODE_MAX_BORDER) * (RD_CODE_MAX_N + 2 * RD_CODE_MAX_BORDER) == MAXCELLS && MAXCELLS <= 3 * RD_WAVE, "three cells per lane of wave 0");
static_assert(WORD == sizeof(uint4) && NT <= 1024, "a thread reads one uint4 a pass");

// merges the pair (key, second) of another holder of DIFFERENT ids into this one
__device__ __forceinline__ void merge(uint32_t &key, int &sec, uint32_t okey, int osec) {
  const uint32_t loser = max(key, okey);
  key = min(key, okey);
  sec = min(min(sec, osec), (int)(loser >> 14));
}

// step 2 for one axis at pixel i of p: the cell and f (the contract's fx, fy)
__device__ __forceinline__ void axis_at(int i, int C, int p, int &c, int &f) {
  const int a = (2 * i + 1) * C;      // at most 2047 * 12
  c = a / (2 * p);
  f = a - c * (2 * p);
}

__device__ __forceinline__ bool counted(int f, int p, int inset) { return inset * p <= 4 * f && 4 * f <= (8 - inset) * p; }

__global__ __launch_bounds__(NT) void k_code(rd_code *out, const uint8_t *plane, const rdk::RectifyQuad *quads, int pw, int ph, rd_code_spec spec, const uint64_t *dict, int ndict) {
  __shared__ unsigned long long sums[MAXCELLS];      // cnt << 32 | sg
  __shared__ uint64_t rots[4];
  __shared__ int dec[4];                             // lo, hi, margin, border_errors
  __shared__ uint32_t wkey[WAVES];
  __shared__ int wsec[WAVES];
  const int lane = threadIdx.x, wave = rd::rd_ty(), tid = wave * RD_WAVE + lane;
  uint64_t *rec = (uint64_t *)(out + blockIdx.x);
  if (!quads[blockIdx.x].status) {      // (the whole block)
    if (tid < 6) rec[tid] = 0;
    return;
  }
  const int total = pw * ph;            // at most 2^20
  const uint8_t *src = plane + (size_t)blockIdx.x * (size_t)total;
  const int n = spec.n, border = spec.border, C = n + 2 * border, ncells = C * C, inset = spec.inset;
  if (tid < MAXCELLS) sums[tid] = 0;
  __syncthreads();

  // A. the cells' sums
  const int mis = (int)((uintptr_t)src & (WORD - 1));      // bytes of the first word that lie in front of the plane
  const uint4 *words = (const uint4 *)(src - mis);
  const int nwords = (mis + total + WORD - 1) / WORD;      // (the last word may reach up to 15 bytes behind the plane: RD_CODE_PLANE_PAD)
  for (int w = tid; w < nwords; w += NT) {
    const uint4 v = words[w];
    const uint32_t word[4] = { v.x, v.y, v.z, v.w };
    const int p0 = w * WORD - mis, first = max(p0, 0);
    int y = first / pw, x = first - y * pw, cx, fx, cy, fy;
    axis_at(x, C, pw, cx, fx);
    axis_at(y, C, ph, cy, fy);
    bool rowok = counted(fy, ph, inset);
    int cur = -1;
    unsigned long long acc = 0;
#pragma unroll
    for (int b = 0; b < WORD; b++) {
      const int p = p0 + b;
      if (p >= 0 && p < total) {
        if (rowok && counted(fx, pw, inset)) {
          const int cell = cy * C + cx;
          if (cell != cur) {
            if (cur >= 0) atomicAdd(&sums[cur], acc);
            cur = cell; acc = 0;
          }
          acc += (1ull << 32) | ((word[b >> 2] >> (8 * (b & 3))) & 255u);
        }
        fx += 2 * C;                                           // the next pixel: 2C <= 2pw, one cell further at most
        if (fx >= 2 * pw) { fx -= 2 * pw; cx++; }
        if (++x == pw) {                                       // the next row
          x = 0; cx = 0; fx = C; y++;
          axis_at(y, C, ph, cy, fy);
          rowok = counted(fy, ph, inset);
        }
      }
    }
    if (cur >= 0) atomicAdd(&sums[cur], acc);
  }
  __syncthreads();

  // B. means, threshold, ring, payload and its rotations
  if (wave == 0) {
    int m[3], lo = 0x7fffffff, hi = 0;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int cell = lane + q * RD_WAVE;
      m[q] = -1;
      if (cell < ncells) {
        const unsigned long long s = sums[cell];
        const uint32_t cnt = (uint32_t)(s >> 32), sg = (uint32_t)s;
        m[q] = cnt ? (int)((256u * sg) / cnt) : 0;      // (cnt > 0 for a legal spec; 256 * sg <= 2 743 392 000: unsigned)
        lo = min(lo, m[q]); hi = max(hi, m[q]);
      }
    }
#pragma unroll
    for (int o = RD_WAVE / 2; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, RD_WAVE)); hi = max(hi, __shfl_xor(hi, o, RD_WAVE)); }
    const int mid = lo + hi;
    const bool flip = spec.polarity != 0;
    int margin = 0x7fffffff, errors = 0;
    bool light[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int cell = lane + q * RD_WAVE, cy = cell / C, cx = cell - cy * C;
      const bool in = m[q] >= 0, ring = cx < border || cx >= C - border || cy < border || cy >= C - border;
      light[q] = 2 * m[q] > mid;
      if (in) margin = min(margin, abs(2 * m[q] - mid));
      errors += __popcll(__ballot(in && ring && (light[q] != flip)));
    }
#pragma unroll
    for (int o = RD_WAVE / 2; o > 0; o >>= 1) margin = min(margin, __shfl_xor(margin, o, RD_WAVE));
    // the payload: lane r*n + c wants cell (border + r) * C + border + c, which lane `from` holds in slot `from >> 6`
    const int r = lane / n, c = lane - r * n;
    const bool pay = lane < n * n;
    const int want = pay ? (r + border) * C + c + border : 0;
    bool bit = false;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const unsigned long long held = __ballot(light[q]);      // cells 64q .. 64q + 63
      if ((want >> 6) == q) bit = (held >> (want & 63)) & 1;
    }
    uint64_t word = __ballot(pay && (bit != flip));
    if (lane == 0) { rots[0] = word; dec[0] = lo; dec[1] = hi; dec[2] = margin; dec[3] = errors; }
    for (int k = 1; k < 4; k++) {
      word = __ballot(pay && ((word >> ((n - 1 - c) * n + r)) & 1));
      if (lane == 0) rots[k] = word;
    }
  }
  __syncthreads();

  // C. the dictionary
  const uint64_t r0 = rots[0], r1 = rots[1], r2 = rots[2], r3 = rots[3];
  uint32_t key = KEY_NONE;
  int sec = NONE;
  for (int id = tid; id < ndict; id += NT) {
    const uint64_t d = dict[id];
    const uint32_t base = (uint32_t)id << 2;
    const uint32_t k = min(min((uint32_t)__popcll(r0 ^ d) << 14 | base, (uint32_t)__popcll(r1 ^ d) << 14 | base | 1u),
                           min((uint32_t)__popcll(r2 ^ d) << 14 | base | 2u, (uint32_t)__popcll(r3 ^ d) << 14 | base | 3u));
    merge(key, sec, k, NONE);
  }
#pragma unroll
  for (int o = RD_WAVE / 2; o > 0; o >>= 1) {
    const uint32_t okey = __shfl_xor(key, o, RD_WAVE);
    const int osec = __shfl_xor(sec, o, RD_WAVE);
    merge(key, sec, okey, osec);
  }
  if (lane == 0) { wkey[wave] = key; wsec[wave] = sec; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < WAVES; w++) merge(key, sec, wkey[w], wsec[w]);
    const int lo = dec[0], hi = dec[1], errors = dec[3];
    const int id = ndict ? (int)(key >> 2 & 0xfffu) : -1, rot = ndict ? (int)(key & 3u) : 0, hamming = (int)(key >> 14);
    const int ok = hi - lo >= 256 * spec.contrast && errors <= spec.max_border && (ndict == 0 || hamming <= spec.max_hamming);
    rec[0] = r0;
    rec[1] = (uint64_t)(uint32_t)id | (uint64_t)(uint32_t)rot << 32;
    rec[2] = (uint64_t)(uint32_t)hamming | (uint64_t)(uint32_t)sec << 32;
    rec[3] = (uint64_t)(uint32_t)errors | (uint64_t)(uint32_t)lo << 32;
    rec[4] = (uint64_t)(uint32_t)hi | (uint64_t)(uint32_t)dec[2] << 32;
    rec[5] = (uint64_t)(uint32_t)ok;      // (reserved = 0)
  }
}

}  // namespace

namespace rdk {

void code(hipStream_t s, uint8_t *out, const uint8_t *plane, size_t plane_bytes, const RectifyQuad *quads, int n, int pw, int ph, const rd_code_spec &spec, const uint64_t *dict, int ndict) {
  if (n <= 0) return;
  if (!rd_code_spec_ok(&spec, pw, ph) || ndict < 0 || ndict > RD_CODE_MAX_DICT) { fprintf(stderr, "rdk::code: not a legal code spec for %d x %d\n", pw, ph); abort(); }      // (rd_rectifier_create_code refuses it first)
  // the kernel reads whole 16-byte words: from the plane's first byte (aligned, so nothing in front of it) to at most 15 bytes behind the last quad's
  if (((uintptr_t)plane & (RD_CODE_PLANE_PAD - 1)) || plane_bytes < (size_t)n * pw * ph + RD_CODE_PLANE_PAD) {
    fprintf(stderr, "rdk::code: the planes of %d quads of %d x %d need %zu readable bytes on a 16-byte boundary, not %zu\n", n, pw, ph, (size_t)n * pw * ph + RD_CODE_PLANE_PAD, plane_bytes);
    abort();
  }
  hipLaunchKernelGGL(k_code, dim3(n), dim3(RD_WAVE, WAVES), 0, s, (rd_code *)out, plane, quads, pw, ph, spec, dict, ndict);
}

}  // namespace rdk
