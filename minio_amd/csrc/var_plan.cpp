/* Host planner for mec_encode_batch_var* (see var_plan.h). */
#include "var_plan.h"

#include <algorithm>

namespace mec {

bool build_var_plan(int d, int total, int64_t block_size, int64_t n,
                    const int64_t *lens, VarPlan *out, int64_t max_cols) {
    if (d <= 0 || total < d || block_size <= 0 || n <= 0 || !lens)
        return false;
    /* chain id item*total+row must fit in 32 bits */
    if (n > (int64_t)UINT32_MAX / total) return false;
    /* total*R_n is the largest byte count a caller derives from the plan */
    const int64_t max_rows = INT64_MAX / total;

    out->items.resize((size_t)n);
    out->col_off.resize((size_t)n + 1);
    out->order.resize((size_t)n);
    int64_t R = 0, C = 0, bytes = 0, shards = 0;
    bool sorted = true; /* already descending: the order is the identity */
    for (int64_t i = 0; i < n; i++) {
        const int64_t len = lens[i];
        if (len < 1 || len > block_size) return false;
        const int64_t S = len / d + (len % d != 0);
        /* keeps R + align64(S) <= max_rows, so nothing below overflows */
        if (S > max_rows - R - 63) return false;
        const int64_t cols = S / 32 + (S % 32 != 0);
        if (cols > max_cols - C) return false;
        out->items[(size_t)i] = VarItem{R, S};
        out->col_off[(size_t)i] = C;
        out->order[(size_t)i] = (uint32_t)i;
        if (i && S > out->items[(size_t)i - 1].shard_len) sorted = false;
        R += (S + 63) & ~int64_t(63);
        C += cols;
        bytes += len; /* len <= d*S, so bytes <= d*R <= INT64_MAX */
        shards += S;
    }
    out->col_off[(size_t)n] = C;
    out->rows_total = R;
    out->cols_total = C;
    out->bytes_total = bytes;
    out->shards_total = shards;
    if (!sorted) {
        /* stable LSD radix sort of the identity order by key = max S - S,
         * 11 bits a pass: two passes for shards up to 4 MiB, O(n) each (a
         * comparison sort was most of the planner's time at n = 16384) */
        const VarItem *it = out->items.data();
        int64_t s_max = it[0].shard_len, s_min = s_max;
        for (int64_t i = 1; i < n; i++) {
            s_max = std::max(s_max, it[i].shard_len);
            s_min = std::min(s_min, it[i].shard_len);
        }
        const uint64_t range = (uint64_t)(s_max - s_min);
        constexpr int kBits = 11;
        out->scratch.resize((size_t)n);
        uint32_t *src = out->order.data(), *dst = out->scratch.data();
        for (int shift = 0; shift < 64 && (range >> shift) != 0;
             shift += kBits) {
            size_t count[(1 << kBits) + 1] = {0};
            for (int64_t k = 0; k < n; k++)
                count[(((uint64_t)(s_max - it[src[k]].shard_len) >> shift) &
                       ((1u << kBits) - 1)) + 1]++;
            for (int b = 0; b < (1 << kBits); b++) count[b + 1] += count[b];
            for (int64_t k = 0; k < n; k++) {
                const uint32_t i = src[k];
                dst[count[((uint64_t)(s_max - it[i].shard_len) >> shift) &
                          ((1u << kBits) - 1)]++] = i;
            }
            std::swap(src, dst);
        }
        if (src != out->order.data()) out->order.swap(out->scratch);
    }
    return true;
}

} // namespace mec
