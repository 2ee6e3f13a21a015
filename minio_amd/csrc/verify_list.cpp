/* Host list builder for mec_verify_reconstruct_batch* (see verify_list.h).
 *
 * The reference does the same bookkeeping per object: parallelReader marks
 * a row whose ReadAt returned errFileCorrupt as missing and triggers
 * another read (cmd/erasure-decode.go:192-212); Decode/Heal reconstruct
 * from the rest, and Erasure.Heal writes each rebuilt row through a bitrot
 * writer, which hashes it (cmd/erasure-decode.go:317-364,
 * cmd/bitrot-streaming.go:57-75).
 */
#include "verify_list.h"

namespace mec {

bool verify_chain_count(int64_t n, int total, uint32_t *count) {
    if (n < 0 || total <= 0) return false;
    /* n <= INT64_MAX / total keeps the product itself from overflowing */
    if (n > (int64_t)UINT32_MAX / total) return false;
    *count = (uint32_t)(n * total);
    return true;
}

bool build_verify_list(int64_t n, int total, const uint8_t *read_mask,
                       std::vector<uint32_t> *list) {
    uint32_t count;
    list->clear();
    if (!verify_chain_count(n, total, &count)) return false;
    for (uint32_t c = 0; c < count; c++)
        if (read_mask[c]) list->push_back(c);
    return true;
}

void merge_verified(uint32_t count, const uint8_t *read_mask,
                    const uint8_t *ok, uint8_t *present) {
    for (uint32_t c = 0; c < count; c++)
        present[c] = (read_mask[c] && ok[c]) ? 1 : 0;
}

void build_rehash_list(const ReconPlan &pl, int d, int p, int64_t n,
                       const uint8_t *present, int data_only,
                       std::vector<uint32_t> *list) {
    const int total = d + p;
    const int scope = data_only ? d : total;
    list->clear();
    for (int64_t i = 0; i < n; i++) {
        if (pl.status[(size_t)i] != kPlanOk) continue;
        const uint8_t *pr = present + (size_t)i * total;
        for (int s = 0; s < scope; s++)
            if (!pr[s]) list->push_back((uint32_t)(i * total + s));
    }
}

} // namespace mec
