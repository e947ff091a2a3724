/* rectdetect-mi355x: scanned pages - what the kernel (rd_k_scan.hip) and the host's rd_scan_limits (rd_scan_host.c) must agree on.  Plain C. */
#ifndef RD_SCAN_TILE_H_INCLUDED
#define RD_SCAN_TILE_H_INCLUDED

#define RD_SCAN_MAX_RADIUS 63
#define RD_SCAN_TILE_W 64      /* output pixels of a block: one wave row is 64 consecutive pixels - one ballot, eight bytes of a bit row */
#define RD_SCAN_TILE_H 16      /* four waves, four rows each */

#endif
