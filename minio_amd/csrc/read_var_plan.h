/* Host planner for mec_verify_reconstruct_batch_var*: the verified batch
 * read with a shard length per item.
 *
 * parallelReader.Read shortens shardSize for the last block of an object
 * (cmd/erasure-decode.go:138-139), and an object of at most one block is
 * only a short block, so a GET or heal batch across objects is a batch of
 * different shard lengths, as a PUT batch is (var_plan.h).
 *
 * The item table (R_i, S_i) and the descending-S_i order are
 * build_var_plan's; the decode plans are build_reconstruct_plan's and the
 * verdict merge is merge_verified's, all unchanged.  This file adds what
 * the per-item-length kernels (read_var.hip) need on top:
 *
 *  - ordered hash lists: the chain ids of build_verify_list /
 *    build_rehash_list, emitted item by item in the plan's descending-S_i
 *    order (rows ascending within an item), so the 16 chains of a wave are
 *    of near-equal length.  ok[] stays indexed by chain id, so
 *    merge_verified does not care about the order;
 *  - tile prefixes: for one work list of ReconPlan, T_0 = 0,
 *    T_{w+1} = T_w + ceil(ceil(S_item(w)/32) / 64).  One tile is 64 columns
 *    of 32 B, i.e. 2 KiB of every row of one (item, entry) pair, the work
 *    of one wave for one trip of gf_matmul_bs_mixed_var_kernel.
 *
 * Pure host code, no HIP includes: linked into the library and into the
 * stand-alone checker tools/read_var_plan_check.cpp.
 */
#ifndef MEC_READ_VAR_PLAN_H
#define MEC_READ_VAR_PLAN_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "recon_plan.h"
#include "var_plan.h"

namespace mec {

/* columns (of 32 B) per tile: one per lane of a wave */
constexpr int64_t kReadVarTileCols = 64;

/* default bound on T_m: every tile's byte offset (2048*T) fits in int64 */
constexpr int64_t kReadVarMaxTiles = INT64_MAX / (32 * kReadVarTileCols);

/* tiles of one row of S bytes, S >= 1 */
inline int64_t read_var_tiles(int64_t S) {
    const int64_t cols = S / 32 + (S % 32 != 0);
    return cols / kReadVarTileCols + (cols % kReadVarTileCols != 0);
}

/* The verify list in hash order.  vp must be build_var_plan's result for
 * the call's n items and total rows per item; read_mask has n*total
 * flags. */
void build_verify_list_ordered(const VarPlan &vp, int total,
                               const uint8_t *read_mask,
                               std::vector<uint32_t> *list);

/* The rehash list in hash order; pl, present and data_only as for
 * build_rehash_list. */
void build_rehash_list_ordered(const VarPlan &vp, const ReconPlan &pl, int d,
                               int p, const uint8_t *present, int data_only,
                               std::vector<uint32_t> *list);

/* Tile prefix T_0..T_m over one work list (m = work.size(), m+1 entries).
 * False, with *prefix unspecified, when a pair names an item outside vp or
 * T_m would exceed max_tiles. */
bool build_tile_prefix(const VarPlan &vp, const std::vector<ReconWork> &work,
                       std::vector<int64_t> *prefix,
                       int64_t max_tiles = kReadVarMaxTiles);

} // namespace mec
#endif
