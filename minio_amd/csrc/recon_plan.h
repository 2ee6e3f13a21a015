/* Host planner for mec_reconstruct_batch_mixed*: turns n per-item erasure
 * masks into a de-duplicated table of decode plans plus per-E work lists
 * for gf_matmul_bs_mixed_kernel<E>.
 *
 * One object read in the reference decodes with one pattern
 * (cmd/erasure-decode.go:239-314), but a batch ACROSS objects does not:
 * every object rotates its shards by hashOrder(bucket/object, d+p)
 * (cmd/erasure-metadata-utils.go:178), so one dead drive is a different
 * missing logical row per object.  The planner inverts once per DISTINCT
 * mask in the call, never per item.
 *
 * Pure host code, no HIP includes: linked into the library and into the
 * stand-alone checker tools/plan_check.cpp.
 */
#ifndef MEC_RECON_PLAN_H
#define MEC_RECON_PLAN_H

#include <cstdint>
#include <vector>

namespace mec {

/* mirror MEC_KMAX_D / MEC_KMAX_E / MEC_KMAX_TOTAL (kernels.h; ec_abi.cpp
 * static_asserts the equality — this header must not pull in HIP) */
constexpr int kPlanMaxD = 32;
constexpr int kPlanMaxE = 8;
constexpr int kPlanMaxTotal = 40;

/* per-item status values = mec_status MEC_OK / MEC_ERR_TOO_FEW_SHARDS */
constexpr uint8_t kPlanOk = 0;
constexpr uint8_t kPlanTooFew = 3;

/* One plan-table entry as the kernel reads it (12 little-endian dwords;
 * the kernel fetches the row bytes as packed dwords through scalar
 * loads).  A pattern that rebuilds more than kPlanMaxE rows becomes
 * several consecutive entries over the same src_rows. */
struct ReconPlanEntry {
    uint8_t src_rows[kPlanMaxD]; /* first d present rows; rest 0 */
    uint8_t dst_rows[kPlanMaxE]; /* n_dst rows to rebuild; rest 0 */
    uint32_t mask_off;           /* dword offset into ReconPlan::masks */
    uint32_t n_dst;              /* 1..kPlanMaxE */
};
static_assert(sizeof(ReconPlanEntry) == 48, "kernel reads 12 dwords");

/* One unit of kernel work: rebuild entry's rows of one batch item. */
struct ReconWork {
    uint32_t item;
    uint32_t entry;
};

struct ReconPlan {
    std::vector<uint8_t> status;         /* n: kPlanOk / kPlanTooFew */
    std::vector<ReconPlanEntry> entries; /* de-duplicated plan table */
    std::vector<uint64_t> entry_mask;    /* present-bit key of each entry */
    /* packed 8x8 bit matrices, bs_masks layout: entry e, output t, source
     * k at masks[e.mask_off + (t*d + k)*2 + w] */
    std::vector<uint32_t> masks;
    /* work[E]: every (item, entry) pair whose entry rebuilds E rows */
    std::vector<ReconWork> work[kPlanMaxE + 1];
    int n_too_few = 0;
};

/* 8x8 bit matrix of the GF(2^8)/0x11D map x -> c*x as two dwords (byte b =
 * row mask: bit a set iff output bit b depends on input bit a). */
void bs_pack_matrix(uint8_t c, uint32_t out[2]);

/* present: n*(d+p) flags, item i's mask at present + i*(d+p).
 * Items with nothing to rebuild get kPlanOk and no work; items with fewer
 * than d rows present get kPlanTooFew and no work.  Returns false only on
 * bad dimensions (d > kPlanMaxD, d+p > kPlanMaxTotal, n < 0). */
bool build_reconstruct_plan(const uint8_t *enc_matrix, int d, int p, int n,
                            const uint8_t *present, int data_only,
                            ReconPlan *out);

} // namespace mec
#endif
