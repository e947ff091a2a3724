// rectdetect-mi355x: composited quads - what the kernel (rd_k_composite.hip), the runtime (rd_composite.hip) and the entry point behind the poll (rd_frames.hip) share.
// The records and the host's arithmetic: rd_comp_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rd_comp_host.h"
#include "rd_pix.h"

namespace rdk {
// n items composited IN PLACE into one frame in format fmt (RD_PIX_*), one launch of ntiles one-wave blocks: tiles holds the pairs tx, ty of the tiles the
// valid items' boxes reach (rd_comp_tiles_of), recs, tiles and patches are device memory; patches: images of pw x ph BGR pixels (may be NULL when no item pastes).
void composite(hipStream_t s, int fmt, const rdpix::PixFrame &frame, const rd_comp_rec *recs, int n, const int32_t *tiles, int ntiles, const uint8_t *patches, int pw, int ph);
}  // namespace rdk
