/* Mixed-pattern batch reconstruct for MI355X (gfx950): one launch rebuilds
 * items that each miss DIFFERENT rows.
 *
 * The reference reconstructs one object's block with one pattern
 * (reedsolomon.Encoder.ReconstructData / Reconstruct, call sites
 * cmd/erasure-coding.go:106,112), but a degraded read or heal batched
 * ACROSS objects sees one pattern per object: each object rotates its
 * shards by hashOrder (cmd/erasure-metadata-utils.go:178).  The uniform
 * kernel (gf_matmul_bs_kernel, kernels.hip) takes its row lists and bit
 * matrices from the kernel arguments; here they come from a plan table in
 * device memory, selected per workgroup through a work list
 * (recon_plan.h).  Everything table-derived is workgroup-uniform, is
 * forced into SGPRs and so is fetched by scalar loads; the per-lane work
 * is the uniform kernel's, unchanged.
 */
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gf_bs.h"
#include "kernels.h"

/* plan-entry dword offsets (recon_plan.h ReconPlanEntry) */
#define MEC_PE_WORDS 12
#define MEC_PE_DST 8
#define MEC_PE_MASK_OFF 10

__device__ __forceinline__ uint32_t mx_sgpr(uint32_t v) {
    return __builtin_amdgcn_readfirstlane(v);
}

/* Same body as gf_matmul_bs_kernel<E, 0>: plane transpose, one v_bitop3
 * per matrix element, next-row prefetch, nontemporal 2x16 B stores.  The
 * grid is linear so the work list may exceed 65535 pairs:
 * blockIdx.x = pair * blocks_x + column block. */
template <int E>
__global__ void __launch_bounds__(256)
gf_matmul_bs_mixed_kernel(GfMixedArgs a) {
    const uint32_t w = blockIdx.x / a.blocks_x;
    const uint32_t bx = blockIdx.x - w * a.blocks_x;
    if (w >= a.n_work) return;
    const uint32_t item = mx_sgpr(a.work[2 * (size_t)w]);
    const uint32_t ent = mx_sgpr(a.work[2 * (size_t)w + 1]);
    const uint32_t *__restrict__ ew = a.entries + (size_t)ent * MEC_PE_WORDS;
    const uint32_t *__restrict__ mbase =
        a.masks + mx_sgpr(ew[MEC_PE_MASK_OFF]);
    const uint32_t dw0 = mx_sgpr(ew[MEC_PE_DST]);
    const uint32_t dw1 = mx_sgpr(ew[MEC_PE_DST + 1]);
    /* source row k: byte k of the entry's first 8 dwords */
    auto srow = [&](int k) -> int64_t {
        return (int64_t)((mx_sgpr(ew[k >> 2]) >> (8 * (k & 3))) & 0xffu);
    };

    const int64_t cols = (a.shard_len + 31) / 32;
    uint8_t *__restrict__ base = a.shards + (int64_t)item * a.item_stride;

    for (int64_t c = (int64_t)bx * blockDim.x + threadIdx.x; c < cols;
         c += (int64_t)a.blocks_x * blockDim.x) {
        const int64_t j = c * 32;
        uint32_t accp[E][8];
#pragma unroll
        for (int i = 0; i < E; i++)
#pragma unroll
            for (int pb = 0; pb < 8; pb++) accp[i][pb] = 0;
        uint32_t xc[8], xn[8];
        {
            const uint8_t *row = base + srow(0) * a.row_stride + j;
            uint4 lo = *(const uint4 *)row;
            uint4 hi = *(const uint4 *)(row + 16);
            xc[0] = lo.x; xc[1] = lo.y; xc[2] = lo.z; xc[3] = lo.w;
            xc[4] = hi.x; xc[5] = hi.y; xc[6] = hi.z; xc[7] = hi.w;
        }
        /* the next row's index is fetched one iteration ahead of the
         * prefetch that needs it, so the vector loads never wait on the
         * scalar load */
        int64_t r_next = srow(a.d > 1 ? 1 : 0);
        for (int k = 0; k < a.d; k++) {
            if (k + 1 < a.d) {
                const uint8_t *row = base + r_next * a.row_stride + j;
                uint4 lo = *(const uint4 *)row;
                uint4 hi = *(const uint4 *)(row + 16);
                xn[0] = lo.x; xn[1] = lo.y; xn[2] = lo.z; xn[3] = lo.w;
                xn[4] = hi.x; xn[5] = hi.y; xn[6] = hi.z; xn[7] = hi.w;
                r_next = srow(k + 2 < a.d ? k + 2 : k + 1);
            }
            bs_transpose(xc);
#pragma unroll
            for (int i = 0; i < E; i++) {
                const uint32_t *m = mbase + ((int64_t)i * a.d + k) * 2;
                const uint32_t mlo = mx_sgpr(m[0]);
                const uint32_t mhi = mx_sgpr(m[1]);
#pragma unroll
                for (int pb = 0; pb < 8; pb++) {
                    uint32_t acc = accp[i][pb];
                    const uint32_t mk =
                        (pb < 4) ? (mlo >> (8 * pb)) : (mhi >> (8 * (pb - 4)));
#pragma unroll
                    for (int pa = 0; pa < 8; pa++) {
                        const uint32_t mm = 0u - ((mk >> pa) & 1u);
                        acc = (uint32_t)__builtin_amdgcn_bitop3_b32(
                            xc[pa], mm, acc, 0x6a); /* (x & m) ^ acc */
                    }
                    accp[i][pb] = acc;
                }
            }
#pragma unroll
            for (int wd = 0; wd < 8; wd++) xc[wd] = xn[wd];
        }
#pragma unroll
        for (int i = 0; i < E; i++) {
            bs_transpose(accp[i]);
            const int64_t drow =
                (int64_t)(((i < 4 ? dw0 : dw1) >> (8 * (i & 3))) & 0xffu);
            uint8_t *orow = base + drow * a.row_stride + j;
            typedef unsigned int v4u __attribute__((ext_vector_type(4)));
            v4u vlo = {accp[i][0], accp[i][1], accp[i][2], accp[i][3]};
            v4u vhi = {accp[i][4], accp[i][5], accp[i][6], accp[i][7]};
            __builtin_nontemporal_store(vlo, (v4u *)orow);
            __builtin_nontemporal_store(vhi, (v4u *)(orow + 16));
        }
    }
}

extern "C" hipError_t mec_launch_gf_matmul_mixed(const GfMixedArgs *args,
                                                 int n_dst,
                                                 hipStream_t stream) {
    if (args->n_work == 0) return hipSuccess;
    /* grid sized from the work-list length as mec_launch_gf_matmul sizes
     * it from n: >= 8192 workgroups, never more than the columns */
    const int64_t cols32 = (args->shard_len + 31) / 32;
    const int64_t n = args->n_work;
    int64_t max_x = (cols32 + 255) / 256;
    int64_t want_x = ((int64_t)2048 * 4 + n - 1) / n;
    int64_t blocks_x = want_x < max_x ? want_x : max_x;
    if (blocks_x < 1) blocks_x = 1;
    if (n * blocks_x > 0x7fffffff) return hipErrorInvalidValue;
    GfMixedArgs a = *args;
    a.blocks_x = (uint32_t)blocks_x;
    dim3 grid((uint32_t)(n * blocks_x));
    dim3 blk(256);
#define CASEM(E)                                                             \
    case E:                                                                  \
        hipLaunchKernelGGL((gf_matmul_bs_mixed_kernel<E>), grid, blk, 0,     \
                           stream, a);                                       \
        return hipGetLastError();
    switch (n_dst) {
        CASEM(1) CASEM(2) CASEM(3) CASEM(4) CASEM(5) CASEM(6) CASEM(7)
        CASEM(8)
    default:
        return hipErrorInvalidValue;
    }
#undef CASEM
}
