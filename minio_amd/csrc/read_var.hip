/* Verified batch read with a different shard length per item
 * (mec_verify_reconstruct_batch_var*), MI355X (gfx950): the read-side twin
 * of encode_var.hip.
 *
 * parallelReader.Read shortens shardSize for the last block of an object
 * (cmd/erasure-decode.go:138-139), and an object of at most one block is
 * only a short block, so a GET or heal batch across objects has one shard
 * length per item.  The uniform kernels (recon_mixed.hip, hh_list.hip) take
 * one shard length and one row stride from their arguments; here every item
 * has its own S_i and stride_i = align64(S_i) in the packed layout of
 * var_plan.h, all d+p rows of an item together:
 *   row s of item i at shards + total*R_i + s*stride_i,
 * read from the device-resident item table items[2i], items[2i+1] = R_i, S_i.
 *
 * Per-lane math is the uniform kernels', unchanged: the bit-sliced GF body
 * of gf_matmul_bs_mixed_kernel (helpers in gf_bs.h) and the
 * 4-lanes-per-chain HighwayHash of hh_quad.h.
 */
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gf_bs.h"
#include "hh_quad.h"
#include "kernels.h"

/* plan-entry dword offsets (recon_plan.h ReconPlanEntry) */
#define MEC_PE_WORDS 12
#define MEC_PE_DST 8
#define MEC_PE_MASK_OFF 10

__device__ __forceinline__ uint32_t rv_sgpr(uint32_t v) {
    return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ int64_t rv_sgpr64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi =
        __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

/* gf_matmul_bs_mixed_kernel<E>'s body over the tile space [0, T_m) of one
 * work list: tile t belongs to the pair w with T[w] <= t < T[w+1] and
 * covers columns [(t - T[w])*64, +64) of that pair's item.  Each WAVE takes
 * one tile per grid-stride trip, so a tile, and with it every table-derived
 * value (plan entry, row bytes, bit matrices, R, S, the row stride), is
 * wave-uniform, is forced into SGPRs and is fetched by scalar loads.  The
 * pair is found by a binary search over T in scalar registers, with the
 * lower bound carried over from the previous trip since t only grows.
 *
 * The four waves of a workgroup may serve four different pairs, and take
 * different numbers of trips: nothing here is workgroup-uniform and there
 * is no barrier.  Keep it that way.
 *
 * Lane l handles column tile*64 + l when the item has that many columns
 * and idles otherwise; lane 0 of every tile is live (T counts
 * ceil(cols/64) tiles per pair), so the scalar reads inside the body always
 * have an active lane to read from. */
template <int E>
__global__ void __launch_bounds__(256)
gf_matmul_bs_mixed_var_kernel(GfMixedVarArgs a) {
    const int64_t *__restrict__ T = a.tiles;
    const uint32_t last = a.n_work - 1;
    const uint32_t lane = threadIdx.x & 63;
    /* blockDim.x is 256: four waves per workgroup */
    const uint32_t wave = rv_sgpr(threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    uint32_t first = 0; /* wave-uniform: pair of the previous tile */

    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < a.tiles_total;
         t += n_waves) {
        {
            /* largest w in [first, last] with T[w] <= t; it exists since
             * T[first] <= t (t grows) and t < T[n_work] */
            uint32_t lo = first, hi = last;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1) / 2;
                if (rv_sgpr64(T[mid]) <= t)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            first = rv_sgpr(lo);
        }
        const uint32_t w = first;
        const uint32_t item = rv_sgpr(a.work[2 * (size_t)w]);
        const uint32_t ent = rv_sgpr(a.work[2 * (size_t)w + 1]);
        const int64_t R = rv_sgpr64(a.items[2 * (size_t)item]);
        const int64_t S = rv_sgpr64(a.items[2 * (size_t)item + 1]);
        const int64_t row_stride = (S + 63) & ~int64_t(63);
        const int64_t cols = (S + 31) / 32;
        const int64_t c = (t - rv_sgpr64(T[w])) * 64 + lane;
        if (c >= cols) continue;

        const uint32_t *__restrict__ ew =
            a.entries + (size_t)ent * MEC_PE_WORDS;
        const uint32_t *__restrict__ mbase =
            a.masks + rv_sgpr(ew[MEC_PE_MASK_OFF]);
        const uint32_t dw0 = rv_sgpr(ew[MEC_PE_DST]);
        const uint32_t dw1 = rv_sgpr(ew[MEC_PE_DST + 1]);
        /* source row k: byte k of the entry's first 8 dwords */
        auto srow = [&](int k) -> int64_t {
            return (int64_t)((rv_sgpr(ew[k >> 2]) >> (8 * (k & 3))) & 0xffu);
        };
        /* c < cols, so j + 32 <= 32*cols <= row_stride */
        const int64_t j = c * 32;
        uint8_t *__restrict__ base = a.shards + (int64_t)a.total * R;

        uint32_t accp[E][8];
#pragma unroll
        for (int i = 0; i < E; i++)
#pragma unroll
            for (int pb = 0; pb < 8; pb++) accp[i][pb] = 0;
        uint32_t xc[8], xn[8];
        {
            const uint8_t *row = base + srow(0) * row_stride + j;
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
                const uint8_t *row = base + r_next * row_stride + j;
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
                const uint32_t mlo = rv_sgpr(m[0]);
                const uint32_t mhi = rv_sgpr(m[1]);
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
            uint8_t *orow = base + drow * row_stride + j;
            typedef unsigned int v4u __attribute__((ext_vector_type(4)));
            v4u vlo = {accp[i][0], accp[i][1], accp[i][2], accp[i][3]};
            v4u vhi = {accp[i][4], accp[i][5], accp[i][6], accp[i][7]};
            __builtin_nontemporal_store(vlo, (v4u *)orow);
            __builtin_nontemporal_store(vhi, (v4u *)(orow + 16));
        }
    }
}

/* hh_list.hip's list-driven chain with the row pointer and the message
 * length per chain: id = list[tid >> 2] names row id % total of item
 * id / total, hashed over exactly S_item bytes; the digest slot is
 * sums + id*32 and the verdict byte ok[id], as in the uniform kernels.
 *
 * The quad contract holds with per-chain lengths because the return, len
 * and the tail branch below depend on the chain alone (slot, S), never on
 * j; the tail is taken at run time.  Waves do diverge between chains of
 * different lengths; the planner's descending-S order keeps the 16 chains
 * of a wave near-equal. */
template <bool VERIFY>
__device__ __forceinline__ void hh256_list_var_body(const HashListVarArgs &a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t slot = tid >> 2;
    const int j = (int)(tid & 3); /* this lane's HighwayHash lane index */
    if (slot >= (int64_t)a.n_list) return;
    const uint32_t id32 = a.list[slot];
    const uint32_t item = id32 / a.total;
    const uint32_t srow = id32 - item * a.total;
    const int64_t id = (int64_t)id32;
    const int64_t R = a.items[2 * (size_t)item];
    const int64_t S = a.items[2 * (size_t)item + 1];
    const int64_t row_stride = (S + 63) & ~int64_t(63);
    const uint8_t *mp = a.shards + (int64_t)a.total * R +
                        (int64_t)srow * row_stride + 8 * j;
    const uint32_t S3 = hh1_sel(j);

    HH1 s;
    hh1_init(s, a.key, j);
    int64_t len = S;
    HH1_STREAM(s, mp, len, S3)
    if (len > 0) hh1_remainder(s, mp, (int)len, j, S3);
    const uint64_t out = hh1_finish(s, j, S3);
    hh1_emit<VERIFY>(out, a.sums + id * 32 + 8 * j, a.ok + id, j);
}

/* two names, so a kernel trace tells the modes apart */
__global__ void __launch_bounds__(256)
hh256_list_var_verify(HashListVarArgs a) {
    hh256_list_var_body<true>(a);
}

__global__ void __launch_bounds__(256) hh256_list_var_sum(HashListVarArgs a) {
    hh256_list_var_body<false>(a);
}

extern "C" hipError_t mec_launch_gf_matmul_mixed_var(
    const GfMixedVarArgs *args, int n_dst, hipStream_t stream) {
    if (args->n_work == 0) return hipSuccess;
    if (args->tiles_total < (int64_t)args->n_work || args->total <= 0)
        return hipErrorInvalidValue;
    /* capped linear grid of 4-wave workgroups, one tile per wave and trip,
     * the uniform launch's 2048*8 workgroups at the most; the grid-stride
     * loop takes the rest */
    const int64_t want = (args->tiles_total + 3) / 4;
    const int64_t cap = 2048 * 8;
    dim3 grid((uint32_t)(want < cap ? want : cap)), blk(256);
#define CASEV(E)                                                             \
    case E:                                                                  \
        hipLaunchKernelGGL((gf_matmul_bs_mixed_var_kernel<E>), grid, blk, 0, \
                           stream, *args);                                   \
        return hipGetLastError();
    switch (n_dst) {
        CASEV(1) CASEV(2) CASEV(3) CASEV(4) CASEV(5) CASEV(6) CASEV(7)
        CASEV(8)
    default:
        return hipErrorInvalidValue;
    }
#undef CASEV
}

extern "C" hipError_t mec_launch_hash_list_var(const HashListVarArgs *args,
                                               int verify,
                                               hipStream_t stream) {
    if (args->n_list == 0) return hipSuccess;
    if (args->total == 0) return hipErrorInvalidValue;
    /* 4 lanes per chain; n_list < 2^32 keeps the grid below 2^26 blocks */
    const int64_t lanes = (int64_t)args->n_list * 4;
    dim3 grid((uint32_t)((lanes + 255) / 256)), blk(256);
    if (verify)
        hipLaunchKernelGGL(hh256_list_var_verify, grid, blk, 0, stream,
                           *args);
    else
        hipLaunchKernelGGL(hh256_list_var_sum, grid, blk, 0, stream, *args);
    return hipGetLastError();
}
