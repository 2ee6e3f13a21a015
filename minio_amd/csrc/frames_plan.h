/* Host planner for mec_encode_frames_batch_var*: batch encode straight into
 * the on-disk [hash||shard] frames of streamingBitrotWriter
 * (cmd/bitrot-streaming.go:44-75), one block length per item.
 *
 * The input is mec_encode_batch_var's packed rows (var_plan.h).  The output
 * layout is defined by the lengths alone.  With S_i = ceil(len_i/d) and
 * total = d+p:
 *   F_0 = 0, F_{i+1} = F_i + 32 + S_i,
 *   frames is total*F_n bytes, row s's stream is [s*F_n, (s+1)*F_n),
 *   in it item i's frame at F_i: the 32-byte digest of the S_i shard bytes
 *   that follow it.
 * No stride, no padding: consecutive blocks of one object passed as
 * consecutive items make [F_first, F_last+1) of row s that object's shard
 * file for logical row s.
 *
 * Pure host code, no HIP includes: linked into the library and into the
 * stand-alone checker tools/frames_plan_check.cpp.
 */
#ifndef MEC_FRAMES_PLAN_H
#define MEC_FRAMES_PLAN_H

#include <cstdint>
#include <vector>

#include "var_plan.h"

namespace mec {

/* F_0..F_n into frame_off (n+1 entries).  False, with nothing written, when
 * d <= 0, block_size <= 0, n <= 0, a pointer is null, a length is outside
 * [1, block_size] or F_n would overflow int64. */
bool frame_offsets(int d, int64_t block_size, int64_t n, const int64_t *lens,
                   int64_t *frame_off);

struct FramesPlan {
    std::vector<int64_t> frame_off; /* n+1: F_0..F_n, strictly increasing */
    int64_t frames_bytes = 0;       /* total * F_n */
};

/* build_var_plan's checks and tables into *var, the F prefix into *out.
 * False, with both unspecified, where build_var_plan refuses or total*F_n
 * (plus a granule of slack) would overflow int64. */
bool build_frames_plan(int d, int total, int64_t block_size, int64_t n,
                       const int64_t *lens, VarPlan *var, FramesPlan *out);

} // namespace mec
#endif
