// rectdetect-mi355x: page components - what rd_k_blob.hip and rd_blob_host.c (rd_blob_limits) share: the tile of pixels a block of the tile kernel labels in LDS, and the bounds of a spec
#pragma once
#define RD_BLOB_TILE_W 64
#define RD_BLOB_TILE_H 32
#define RD_BLOB_MAX_RADIUS 63
#define RD_BLOB_MAX_BLOBS 4096
#define RD_BLOB_MAX_PIXELS (1 << 22)      /* pw * ph of a page; the largest area */
#define RD_BLOB_MAX_SLOT_PIXELS ((size_t)1 << 27)      /* max_quads * pw * ph of a rectifier: 1 GiB of scratch per slot at most */
