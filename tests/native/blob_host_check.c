/* rectdetect-mi355x: rd_blob_host.c as a plain process, for the sanitizers (tests/test_cpu_blobs.py compiles both files with -fsanitize=address,undefined).
 * In-program masks with known answers: the bounds of a spec, the sizes, an empty page, a checkerboard under both connectivities, the capacity rule, pad bits, a
 * comb whose teeth join late, and the full 2048 x 2048 page whose coordinate sums do not fit int32.  Every output lies between guard bytes. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rectdetect_hip.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "blob_host_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)
#define GUARD 64

static rd_blob_spec spec_of(int connectivity, int min_area, int max_area, int max_blobs, int page) {
  rd_blob_spec s;
  memset(&s, 0, sizeof(s));
  s.radius = 15; s.k = 26; s.oversample = 1; s.connectivity = connectivity; s.min_area = min_area; s.max_area = max_area; s.max_blobs = max_blobs; s.page = page;
  return s;
}

static uint8_t *pack(const uint8_t *mask, int pw, int ph, int set_pad) {
  const int rb = (pw + 7) >> 3;
  uint8_t *bits = (uint8_t *)calloc((size_t)rb * ph, 1);
  CHECK(bits);
  for (int j = 0; j < ph; j++) {
    for (int i = 0; i < pw; i++) if (mask[(size_t)j * pw + i]) bits[(size_t)j * rb + (i >> 3)] |= (uint8_t)(0x80 >> (i & 7));
    if (set_pad) for (int i = pw; i < 8 * rb; i++) bits[(size_t)j * rb + (i >> 3)] |= (uint8_t)(0x80 >> (i & 7));
  }
  return bits;
}

/* runs rd_blob_page_host between guards; the caller frees the result (its first byte is the output's) */
static uint8_t *run(const uint8_t *bits, int pw, int ph, const rd_blob_spec *s) {
  const size_t n = rd_blob_bytes(s, pw, ph);
  CHECK(n > 0 && n % 8 == 0);
  uint8_t *buf = (uint8_t *)malloc(n + 2 * GUARD);
  CHECK(buf && ((uintptr_t)buf & 7) == 0);
  memset(buf, 0xA5, n + 2 * GUARD);
  CHECK(rd_blob_page_host(bits, pw, ph, s, buf + GUARD) == 1);
  for (int k = 0; k < GUARD; k++) CHECK(buf[k] == 0xA5 && buf[GUARD + n + k] == 0xA5);
  memmove(buf, buf + GUARD, n);
  return buf;
}

int main(void) {
  rd_blob_spec s = spec_of(8, 1, 0, 16, 1);
  CHECK(sizeof(rd_blob_spec) == 48 && sizeof(rd_blob_head) == 32 && sizeof(rd_blob) == 40);
  CHECK(rd_blob_spec_ok(&s, 2048, 2048) && !rd_blob_spec_ok(&s, 2049, 2048) && !rd_blob_spec_ok(NULL, 8, 8) && !rd_blob_spec_ok(&s, 0, 8));
  CHECK(rd_blob_bytes(&s, 9, 5) == 32 + 40 * 16 + 16 && rd_blob_bytes(&s, 8, 8) == 32 + 40 * 16 + 8);
  s.page = 0; CHECK(rd_blob_bytes(&s, 9, 5) == 32 + 40 * 16);
  s.connectivity = 6; CHECK(!rd_blob_spec_ok(&s, 8, 8) && rd_blob_bytes(&s, 8, 8) == 0);
  int32_t lim[10];
  for (int k = 0; k < 10; k++) lim[k] = -7;
  rd_blob_limits(lim + 1);
  CHECK(lim[0] == -7 && lim[9] == -7 && lim[1] == (1 << 4 | 1 << 8) && lim[2] == 7 && lim[3] == 63 && lim[4] == 4096 && lim[5] == 1 << 22 && lim[6] % 64 == 0 && lim[7] >= 1 && lim[8] == 0);

  { /* refusals write nothing */
    uint8_t bits[8] = { 0xff, 0, 0, 0, 0, 0, 0, 0 };
    uint64_t out[64];
    memset(out, 0xA5, sizeof(out));
    s = spec_of(4, 1, 0, 1, 0);
    CHECK(rd_blob_page_host(NULL, 8, 1, &s, out) == 0 && rd_blob_page_host(bits, 8, 1, NULL, out) == 0 && rd_blob_page_host(bits, 8, 1, &s, NULL) == 0);
    CHECK(rd_blob_page_host(bits, 8, 1, &s, (uint8_t *)out + 4) == 0 && rd_blob_page_host(bits, 0, 1, &s, out) == 0);
    s.max_blobs = 0; CHECK(rd_blob_page_host(bits, 8, 1, &s, out) == 0);
    for (size_t k = 0; k < sizeof(out); k++) CHECK(((uint8_t *)out)[k] == 0xA5);
  }
  { /* an empty page, and one whose only ink is its pad bits */
    uint8_t mask[5 * 9];
    memset(mask, 0, sizeof(mask));
    s = spec_of(8, 1, 0, 4, 1);
    for (int pad = 0; pad < 2; pad++) {
      uint8_t *bits = pack(mask, 9, 5, pad), *out = run(bits, 9, 5, &s);
      for (size_t k = 0; k < rd_blob_bytes(&s, 9, 5); k++) CHECK(out[k] == 0);
      free(out); free(bits);
    }
  }
  { /* a 9 x 7 checkerboard: 32 components under 4, the first 5 in raster order survive a max_blobs of 5; one component under 8 */
    uint8_t mask[7 * 9];
    for (int j = 0; j < 7; j++) for (int i = 0; i < 9; i++) mask[j * 9 + i] = (uint8_t)(((i + j) & 1) == 0);
    uint8_t *bits = pack(mask, 9, 7, 1);
    s = spec_of(4, 1, 0, 5, 1);
    uint8_t *out = run(bits, 9, 7, &s);
    const rd_blob_head *h = (const rd_blob_head *)out;
    const rd_blob *r = (const rd_blob *)(h + 1);
    CHECK(h->ink == 32 && h->all == 32 && h->found == 32 && h->written == 5 && h->ink_kept == 32 && h->largest == 1 && h->flags == RD_BLOB_OVERFLOW && h->reserved == 0);
    for (int k = 0; k < 5; k++) CHECK(r[k].first == 2 * k && r[k].area == 1 && r[k].x0 == 2 * k && r[k].x1 == 2 * k && r[k].y0 == 0 && r[k].y1 == 0 && r[k].sx == 2 * k && r[k].sy == 0);
    const uint8_t *page = out + 32 + 40 * 5;
    for (int j = 0; j < 7; j++) CHECK(page[2 * j] == ((j & 1) ? 0x55 : 0xAA) && page[2 * j + 1] == ((j & 1) ? 0x00 : 0x80));      /* (pad bits 0) */
    CHECK(page[14] == 0 && page[15] == 0);
    free(out);
    s = spec_of(8, 1, 0, 5, 0);
    out = run(bits, 9, 7, &s);
    h = (const rd_blob_head *)out; r = (const rd_blob *)(h + 1);
    CHECK(h->all == 1 && h->found == 1 && h->written == 1 && h->flags == 0 && h->largest == 32);
    CHECK(r[0].first == 0 && r[0].area == 32 && r[0].x0 == 0 && r[0].y0 == 0 && r[0].x1 == 8 && r[0].y1 == 6 && r[0].sx == 128 && r[0].sy == 96 && r[1].area == 0 && r[1].first == 0);
    free(out); free(bits);
  }
  { /* a comb joined at the bottom: the teeth are separate until the last row, the root is still pixel 0; the filter drops it and keeps a lone square */
    enum { W = 70, H = 40 };
    uint8_t *mask = (uint8_t *)calloc(W * H, 1);
    CHECK(mask);
    for (int j = 0; j < H - 4; j++) for (int i = 0; i < W; i += 2) mask[j * W + i] = 1;
    for (int i = 0; i < W; i++) mask[(H - 5) * W + i] = 1;
    mask[(H - 2) * W + 3] = mask[(H - 2) * W + 4] = mask[(H - 1) * W + 3] = mask[(H - 1) * W + 4] = 1;
    uint8_t *bits = pack(mask, W, H, 0);
    s = spec_of(4, 1, 0, 4, 0);
    uint8_t *out = run(bits, W, H, &s);
    const rd_blob_head *h = (const rd_blob_head *)out;
    const rd_blob *r = (const rd_blob *)(h + 1);
    const int comb_area = 35 * (H - 5) + W;
    CHECK(h->all == 2 && h->found == 2 && h->largest == comb_area && r[0].first == 0 && r[0].area == comb_area && r[0].x1 == W - 1 && r[0].y1 == H - 5);
    CHECK(r[1].first == (H - 2) * W + 3 && r[1].area == 4 && r[1].sx == 14 && r[1].sy == 2 * (H - 2) + 2 * (H - 1));
    free(out);
    s = spec_of(4, 4, 4, 4, 1);
    out = run(bits, W, H, &s);
    h = (const rd_blob_head *)out; r = (const rd_blob *)(h + 1);
    CHECK(h->all == 2 && h->found == 1 && h->ink_kept == 4 && h->largest == comb_area && r[0].area == 4);
    const uint8_t *page = out + 32 + 40 * 4;
    int set = 0;
    for (int k = 0; k < ((W + 7) >> 3) * H; k++) for (int b = 0; b < 8; b++) set += page[k] >> b & 1;
    CHECK(set == 4);
    free(out); free(bits); free(mask);
  }
  { /* the full 2048 x 2048 page: sums that need 64 bits */
    enum { S = 2048 };
    uint8_t *bits = (uint8_t *)malloc((size_t)S * S / 8);
    CHECK(bits);
    memset(bits, 0xff, (size_t)S * S / 8);
    s = spec_of(4, 1, 1 << 22, 1, 1);
    uint8_t *out = run(bits, S, S, &s);
    const rd_blob_head *h = (const rd_blob_head *)out;
    const rd_blob *r = (const rd_blob *)(h + 1);
    CHECK(h->ink == 1 << 22 && h->all == 1 && h->found == 1 && h->largest == 1 << 22 && r->area == 1 << 22 && r->sx == 4292870144ll && r->sy == 4292870144ll && r->x1 == S - 1 && r->y1 == S - 1);
    CHECK(memcmp(out + 32 + 40, bits, (size_t)S * S / 8) == 0);
    free(out); free(bits);
  }
  printf("blob_host_check: ok\n");
  return 0;
}
