/* Host planner for the mixed-pattern batch reconstruct (recon_plan.h). */
#include "recon_plan.h"
#include "gf_host.h"

#include <cstring>
#include <unordered_map>

namespace mec {

void bs_pack_matrix(uint8_t c, uint32_t out[2]) {
    uint64_t m = 0;
    for (int b = 0; b < 8; b++) {
        uint8_t row = 0;
        for (int a = 0; a < 8; a++)
            if ((gf_mul(c, (uint8_t)(1u << a)) >> b) & 1)
                row |= (uint8_t)(1u << a);
        m |= (uint64_t)row << (8 * b);
    }
    out[0] = (uint32_t)m;
    out[1] = (uint32_t)(m >> 32);
}

namespace {

struct PatternRef {
    uint32_t first; /* first entry of the pattern */
    uint32_t count; /* entries (ceil(n_dst / kPlanMaxE)); 0 = unrecoverable */
};

/* Append the entries for one mask; returns how many were added (0 when
 * build_decode_plan refuses the mask). */
uint32_t add_pattern(const uint8_t *enc_matrix, int d, int p,
                     const uint8_t *present, int data_only, uint64_t key,
                     ReconPlan *out) {
    int src_idx[kMaxShards], dst_idx[kMaxShards], n_dst = 0;
    std::vector<uint8_t> dec((size_t)(d + p) * d);
    if (!build_decode_plan(enc_matrix, d, p, present, data_only, src_idx,
                           dst_idx, &n_dst, dec.data()))
        return 0;
    uint32_t added = 0;
    for (int t0 = 0; t0 < n_dst; t0 += kPlanMaxE) {
        const int e = n_dst - t0 > kPlanMaxE ? kPlanMaxE : n_dst - t0;
        ReconPlanEntry ent;
        memset(&ent, 0, sizeof(ent));
        for (int k = 0; k < d; k++) ent.src_rows[k] = (uint8_t)src_idx[k];
        for (int i = 0; i < e; i++) ent.dst_rows[i] = (uint8_t)dst_idx[t0 + i];
        ent.mask_off = (uint32_t)out->masks.size();
        ent.n_dst = (uint32_t)e;
        out->masks.resize(out->masks.size() + (size_t)e * d * 2);
        uint32_t *m = out->masks.data() + ent.mask_off;
        for (int i = 0; i < e; i++)
            for (int k = 0; k < d; k++)
                bs_pack_matrix(dec[(size_t)(t0 + i) * d + k],
                               &m[((size_t)i * d + k) * 2]);
        out->entries.push_back(ent);
        out->entry_mask.push_back(key);
        added++;
    }
    return added;
}

} // namespace

bool build_reconstruct_plan(const uint8_t *enc_matrix, int d, int p, int n,
                            const uint8_t *present, int data_only,
                            ReconPlan *out) {
    const int total = d + p;
    if (d <= 0 || p < 0 || d > kPlanMaxD || total > kPlanMaxTotal || n < 0)
        return false;
    out->status.assign((size_t)n, kPlanOk);
    out->entries.clear();
    out->entry_mask.clear();
    out->masks.clear();
    for (auto &w : out->work) w.clear();
    out->n_too_few = 0;

    const uint64_t all = (total == 64) ? ~0ull : ((1ull << total) - 1);
    const uint64_t data_rows = (1ull << d) - 1;
    /* one call has one data_only, so the present bits alone key a pattern */
    std::unordered_map<uint64_t, PatternRef> seen;
    for (int i = 0; i < n; i++) {
        const uint8_t *pr = present + (size_t)i * total;
        uint64_t key = 0;
        for (int s = 0; s < total; s++)
            if (pr[s]) key |= 1ull << s;
        if (key == all) continue; /* nothing missing */
        if (__builtin_popcountll(key) < d) {
            out->status[i] = kPlanTooFew;
            out->n_too_few++;
            continue;
        }
        if (data_only && (key & data_rows) == data_rows) continue;
        auto it = seen.find(key);
        if (it == seen.end()) {
            PatternRef ref;
            ref.first = (uint32_t)out->entries.size();
            ref.count = add_pattern(enc_matrix, d, p, pr, data_only, key, out);
            it = seen.emplace(key, ref).first;
        }
        const PatternRef ref = it->second;
        if (ref.count == 0) { /* singular: as the uniform call reports it */
            out->status[i] = kPlanTooFew;
            out->n_too_few++;
            continue;
        }
        for (uint32_t c = 0; c < ref.count; c++) {
            const uint32_t e = ref.first + c;
            out->work[out->entries[e].n_dst].push_back(
                ReconWork{(uint32_t)i, e});
        }
    }
    return true;
}

} // namespace mec
