/* Host planner for mec_encode_frames_batch_var* (see frames_plan.h). */
#include "frames_plan.h"

#include <cstddef>

namespace mec {

bool frame_offsets(int d, int64_t block_size, int64_t n, const int64_t *lens,
                   int64_t *frame_off) {
    if (d <= 0 || block_size <= 0 || n <= 0 || !lens || !frame_off)
        return false;
    /* first pass checks, second writes: a refusal leaves frame_off alone */
    int64_t F = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t len = lens[i];
        if (len < 1 || len > block_size) return false;
        const int64_t S = len / d + (len % d != 0);
        if (S > INT64_MAX - 32 - F) return false;
        F += 32 + S;
    }
    F = 0;
    for (int64_t i = 0; i < n; i++) {
        frame_off[i] = F;
        F += 32 + lens[i] / d + (lens[i] % d != 0);
    }
    frame_off[n] = F;
    return true;
}

bool build_frames_plan(int d, int total, int64_t block_size, int64_t n,
                       const int64_t *lens, VarPlan *var, FramesPlan *out) {
    if (!build_var_plan(d, total, block_size, n, lens, var)) return false;
    /* sum S_i <= R_n and total*R_n fits (build_var_plan); 32*n is below 2^37 */
    const int64_t Fn = var->shards_total + 32 * n;
    if (Fn > (INT64_MAX - 64) / total) return false;
    out->frame_off.resize((size_t)n + 1);
    int64_t F = 0;
    for (int64_t i = 0; i < n; i++) {
        out->frame_off[(size_t)i] = F;
        F += 32 + var->items[(size_t)i].shard_len;
    }
    out->frame_off[(size_t)n] = F;
    out->frames_bytes = (int64_t)total * F;
    return true;
}

} // namespace mec
