/* Host planner for mec_bitrot_verify_files* (see scrub_plan.h). */
#include "scrub_plan.h"

#include <algorithm>

namespace mec {

int64_t scrub_shard_file_size(int64_t part, int64_t shard) {
    const int64_t frames = part / shard + (part % shard != 0);
    if (frames > (INT64_MAX - part) / kScrubHashBytes) return -1;
    return frames * kScrubHashBytes + part;
}

bool scrub_file_offsets(int n, const int64_t *sizes, int64_t *off) {
    if (n <= 0 || !sizes || !off) return false;
    int64_t F = 0;
    for (int f = 0; f < n; f++) {
        if (sizes[f] < 0 || sizes[f] > INT64_MAX - 63) return false;
        const int64_t step = (sizes[f] + 63) & ~int64_t(63);
        if (step > INT64_MAX - F) return false;
        F += step;
    }
    F = 0;
    for (int f = 0; f < n; f++) {
        off[f] = F;
        F += (sizes[f] + 63) & ~int64_t(63);
    }
    off[n] = F;
    return true;
}

/* message bytes of one chain */
static inline int64_t chain_len(const ScrubPlan &pl, const ScrubChain &c) {
    const ScrubFile &sf = pl.files[c.file];
    return c.frame + 1 == sf.frames ? sf.last : sf.shard;
}

bool build_scrub_plan(int n, const int64_t *file_off,
                      const int64_t *file_sizes, const int64_t *part_sizes,
                      const int64_t *shard_sizes, int64_t files_bytes,
                      unsigned base_mod8, ScrubPlan *pl,
                      uint64_t max_frames) {
    if (n <= 0 || !file_off || !file_sizes || !part_sizes || !shard_sizes ||
        !pl || files_bytes < 0)
        return false;
    uint64_t total = 0;
    for (int f = 0; f < n; f++) {
        if (file_off[f] < 0 || file_sizes[f] < 0 || part_sizes[f] < 0 ||
            shard_sizes[f] < 1)
            return false;
        if (file_off[f] > files_bytes ||
            file_sizes[f] > files_bytes - file_off[f])
            return false;
        if (file_sizes[f] !=
            scrub_shard_file_size(part_sizes[f], shard_sizes[f]))
            continue;
        /* every frame takes more than 32 of the file's bytes, so the count
         * is far below 2^63 and the sum cannot wrap */
        const int64_t S = shard_sizes[f], part = part_sizes[f];
        total += (uint64_t)(part / S + (part % S != 0));
        if (total > max_frames) return false;
    }

    pl->files.assign((size_t)n, ScrubFile{});
    pl->early.assign((size_t)n, kScrubHashed);
    pl->aligned.clear();
    pl->sheared.clear();
    for (int f = 0; f < n; f++) {
        ScrubFile &sf = pl->files[(size_t)f];
        const int64_t S = shard_sizes[f], part = part_sizes[f];
        sf.off = file_off[f];
        sf.shard = S;
        if (file_sizes[f] != scrub_shard_file_size(part, S)) {
            pl->early[(size_t)f] = kScrubBadSize;
            continue;
        }
        if (part == 0) {
            pl->early[(size_t)f] = kScrubEmpty;
            continue;
        }
        const int64_t frames = part / S + (part % S != 0);
        sf.frames = (uint32_t)frames;
        sf.last = part - (frames - 1) * S;
        /* only the address modulo 8 matters, and it advances by the pitch
         * modulo 8 from frame to frame */
        const unsigned step = (unsigned)((kScrubHashBytes + S) & 7);
        unsigned phase = (base_mod8 + (unsigned)(sf.off & 7)) & 7;
        for (int64_t k = 0; k < frames; k++) {
            const ScrubChain c{(uint32_t)f, (uint32_t)k};
            (phase ? pl->sheared : pl->aligned).push_back(c);
            phase = (phase + step) & 7;
        }
    }
    /* generation order is ascending (file, frame); a stable sort by
     * descending length keeps it among equals.  A scrub of whole frames of
     * one geometry is in order as generated: one pass finds that out */
    const auto longer = [pl](const ScrubChain &a, const ScrubChain &b) {
        return chain_len(*pl, a) > chain_len(*pl, b);
    };
    for (std::vector<ScrubChain> *list : {&pl->aligned, &pl->sheared})
        if (!std::is_sorted(list->begin(), list->end(), longer))
            std::stable_sort(list->begin(), list->end(), longer);
    return true;
}

void reduce_scrub(const ScrubPlan &pl, const uint8_t *ok, uint8_t *corrupt,
                  int64_t *first_bad) {
    const size_t n = pl.files.size();
    for (size_t f = 0; f < n; f++) {
        corrupt[f] = pl.early[f] == kScrubBadSize;
        if (first_bad) first_bad[f] = -1;
    }
    size_t slot = 0;
    for (const std::vector<ScrubChain> *list : {&pl.aligned, &pl.sheared})
        for (const ScrubChain &c : *list) {
            if (!ok[slot++]) {
                corrupt[c.file] = 1;
                if (first_bad && (first_bad[c.file] < 0 ||
                                  (int64_t)c.frame < first_bad[c.file]))
                    first_bad[c.file] = (int64_t)c.frame;
            }
        }
}

} // namespace mec
