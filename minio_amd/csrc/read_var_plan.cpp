/* Host planner for mec_verify_reconstruct_batch_var* (see read_var_plan.h). */
#include "read_var_plan.h"

namespace mec {

void build_verify_list_ordered(const VarPlan &vp, int total,
                               const uint8_t *read_mask,
                               std::vector<uint32_t> *list) {
    list->clear();
    for (const uint32_t i : vp.order) {
        const uint8_t *rm = read_mask + (size_t)i * total;
        for (int s = 0; s < total; s++)
            if (rm[s]) list->push_back(i * (uint32_t)total + (uint32_t)s);
    }
}

void build_rehash_list_ordered(const VarPlan &vp, const ReconPlan &pl, int d,
                               int p, const uint8_t *present, int data_only,
                               std::vector<uint32_t> *list) {
    const int total = d + p;
    const int scope = data_only ? d : total;
    list->clear();
    for (const uint32_t i : vp.order) {
        if (pl.status[i] != kPlanOk) continue;
        const uint8_t *pr = present + (size_t)i * total;
        for (int s = 0; s < scope; s++)
            if (!pr[s]) list->push_back(i * (uint32_t)total + (uint32_t)s);
    }
}

bool build_tile_prefix(const VarPlan &vp, const std::vector<ReconWork> &work,
                       std::vector<int64_t> *prefix, int64_t max_tiles) {
    prefix->resize(work.size() + 1);
    int64_t T = 0;
    for (size_t w = 0; w < work.size(); w++) {
        (*prefix)[w] = T;
        if (work[w].item >= vp.items.size()) return false;
        const int64_t tiles = read_var_tiles(vp.items[work[w].item].shard_len);
        if (tiles > max_tiles - T) return false;
        T += tiles;
    }
    (*prefix)[work.size()] = T;
    return T <= max_tiles;
}

} // namespace mec
