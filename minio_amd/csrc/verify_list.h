/* Host list builder for mec_verify_reconstruct_batch*: which chains the
 * list-driven HighwayHash kernels (hh_list.hip) verify, how their verdicts
 * become the `present` mask the mixed planner takes, and which rebuilt
 * rows get a fresh digest afterwards.
 *
 * A chain id is item*(d+p)+row: the row's index in the shard buffer and
 * its digest's index in the fused sums layout.
 *
 * Pure host code, no HIP includes: linked into the library and into the
 * stand-alone checker tools/verify_list_check.cpp.
 */
#ifndef MEC_VERIFY_LIST_H
#define MEC_VERIFY_LIST_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "recon_plan.h"

namespace mec {

/* n*total chains must be addressable by a 32-bit id.  False when n < 0,
 * total <= 0 or n*total > UINT32_MAX; else *count = n*total. */
bool verify_chain_count(int64_t n, int total, uint32_t *count);

/* The verify list: the ids of the rows that were read (read_mask nonzero),
 * ascending.  False when verify_chain_count refuses the dimensions. */
bool build_verify_list(int64_t n, int total, const uint8_t *read_mask,
                       std::vector<uint32_t> *list);

/* present[c] = 1 where chain c was read and its digest matched, else 0.
 * ok holds the kernel's verdicts; slots of unread chains are ignored. */
void merge_verified(uint32_t count, const uint8_t *read_mask,
                    const uint8_t *ok, uint8_t *present);

/* The rehash list: the rows the plan's kernels rebuild, i.e. rows of
 * status-OK items that are not present and are in scope (data rows only
 * under data_only), ascending.  pl must be build_reconstruct_plan's result
 * for the same n, present and data_only.  An item that is complete in
 * scope, or TOO_FEW, contributes nothing. */
void build_rehash_list(const ReconPlan &pl, int d, int p, int64_t n,
                       const uint8_t *present, int data_only,
                       std::vector<uint32_t> *list);

} // namespace mec
#endif
