/* Host planner for mec_encode_batch_var*: turns n per-item block lengths
 * into the packed row layout and the tables gf_encode_bs_var_kernel and
 * hh256_var_kernel (encode_var.hip) read.
 *
 * Erasure.Encode (cmd/erasure-encode.go:76-108) calls EncodeData(buf[:n])
 * with whatever io.ReadFull returned, so every object of at most one block
 * and the last block of every larger object is short, and a PUT batch
 * across objects is a batch of different lengths.  The shard size is
 * ceil(len/d) (Split, cmd/erasure-coding.go:81), so a different length moves
 * every byte to another shard and column: the lengths cannot be padded to a
 * common one.
 *
 * The layout is defined by the lengths alone.  For item i:
 *   S_i = ceil(len_i/d), stride_i = align64(S_i),
 *   R_0 = 0, R_{i+1} = R_i + stride_i,
 *   data row k at d*R_i + k*stride_i, parity row t at p*R_i + t*stride_i,
 *   cols_i = ceil(S_i/32), C_0 = 0, C_{i+1} = C_i + cols_i.
 *
 * Pure host code, no HIP includes: linked into the library and into the
 * stand-alone checker tools/var_plan_check.cpp.
 */
#ifndef MEC_VAR_PLAN_H
#define MEC_VAR_PLAN_H

#include <cstdint>
#include <vector>

namespace mec {

/* One item as the kernels read it (two little-endian qwords). */
struct VarItem {
    int64_t row_off;   /* R_i */
    int64_t shard_len; /* S_i */
};
static_assert(sizeof(VarItem) == 16, "kernels read 2 qwords per item");

struct VarPlan {
    std::vector<VarItem> items;   /* n */
    std::vector<int64_t> col_off; /* n+1: C_0..C_n, strictly increasing */
    /* hash order: the item indices by descending S_i, equal S_i in
     * ascending index order (stable), so the 16 chains of a wave are of
     * near-equal length and the longest start first */
    std::vector<uint32_t> order;  /* n */
    std::vector<uint32_t> scratch; /* the sort's second buffer, kept */
    int64_t rows_total = 0;   /* R_n */
    int64_t cols_total = 0;   /* C_n */
    int64_t bytes_total = 0;  /* sum len_i: the packed host input */
    int64_t shards_total = 0; /* sum S_i: p of these is the packed parity */
};

/* default bound on C_n: every column's byte offset (32*C) fits in int64 */
constexpr int64_t kVarMaxCols = INT64_MAX / 32;

/* total = d+p rows per item.  False, with *out unspecified, when d <= 0,
 * total < d, block_size <= 0, n <= 0, lens is null, any length is outside
 * [1, block_size], n*total does not fit in 32 bits (chain ids), C_n would
 * exceed max_cols, or total*R_n would overflow int64 (buffer sizes). */
bool build_var_plan(int d, int total, int64_t block_size, int64_t n,
                    const int64_t *lens, VarPlan *out,
                    int64_t max_cols = kVarMaxCols);

} // namespace mec
#endif
