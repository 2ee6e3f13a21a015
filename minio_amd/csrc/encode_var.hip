/* Batch encode + bitrot digests with a different block length per item
 * (mec_encode_batch_var*), MI355X (gfx950).
 *
 * Erasure.Encode (cmd/erasure-encode.go:76-108) hands EncodeData whatever
 * io.ReadFull returned, so a PUT batch across objects is a batch of
 * different lengths, and the shard size ceil(len/d) (Split,
 * cmd/erasure-coding.go:81) moves every byte when the length changes.  The
 * uniform kernels take one shard length and one row stride from their
 * arguments and one batch item per gridDim.y; here every item has its own
 * S_i and stride_i = align64(S_i) in a packed layout (var_plan.h), read
 * from three device-resident tables:
 *   items[2i], items[2i+1] = R_i, S_i
 *   col_off[0..n]          = prefix of cols_i = ceil(S_i/32)
 *   order[0..n)            = items by descending S_i (hash launch order)
 *
 * Per-lane math is the uniform kernels', unchanged: gf_encode_bs_kernel
 * (kernels.hip, helpers in gf_bs.h) and the 4-lanes-per-chain HighwayHash
 * of hh_quad.h.
 */
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gf_bs.h"
#include "hh_quad.h"
#include "kernels.h"
#include "ec_matrices_gen.h"

__device__ __forceinline__ int64_t ev_sgpr64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi =
        __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

/* gf_encode_bs_kernel's body over a flattened global column space: lane g
 * of col_off[n] columns belongs to the item i with col_off[i] <= g <
 * col_off[i+1], so a batch of 512-byte shards fills its waves instead of
 * running one mostly idle workgroup per item, and there is no gridDim.y = n.
 *
 * Item lookup, per grid-stride trip: one wave-uniform binary search for the
 * item of the wave's first column (scalar registers, lower bound carried
 * over from the previous trip since g only grows); when the wave's 64
 * columns end inside that item, which is every wave but one per item for
 * long shards, that is all.  Otherwise each lane searches the next 63
 * items (every item has at least one column), at most 6 steps.
 *
 * Lanes of one wave may belong to different items.  Nothing after the
 * lookup is cross-lane, so that is safe; keep it that way. */
template <int D, int P, const uint8_t (&MAT)[P][D], int PF>
__global__ void __launch_bounds__(256) gf_encode_bs_var_kernel(EncVarArgs a) {
    const int64_t *__restrict__ C = a.col_off;
    const int64_t *__restrict__ items = a.items;
    const uint32_t last = a.n - 1;
    uint32_t first = 0; /* wave-uniform: item of the wave's first column */

    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < a.cols_total; g += (int64_t)gridDim.x * blockDim.x) {
        /* blockDim.x is a multiple of 64, so g - lane is the same in every
         * active lane of the wave */
        const int64_t g0 = ev_sgpr64(g - (int64_t)(threadIdx.x & 63));
        {
            /* largest i in [first, last] with C[i] <= g0; it exists since
             * C[first] <= g0 (g0 grows) and g0 <= g < C[n] */
            uint32_t lo = first, hi = last;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1) / 2;
                if (ev_sgpr64(C[mid]) <= g0)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            first = __builtin_amdgcn_readfirstlane(lo);
        }
        uint32_t i = first;
        if (first < last && ev_sgpr64(C[first + 1]) <= g0 + 63) {
            uint32_t lo = first;
            uint32_t hi = last - first > 63 ? first + 63 : last;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1) / 2;
                if (C[mid] <= g)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            i = lo;
        }
        const int64_t R = items[2 * (size_t)i];
        const int64_t S = items[2 * (size_t)i + 1];
        const int64_t row_stride = (S + 63) & ~int64_t(63);
        /* g < C[i+1], so j + 32 <= 32*cols_i <= row_stride */
        const int64_t j = (g - C[i]) * 32;
        const uint8_t *__restrict__ sbase = a.data + (int64_t)D * R;
        uint8_t *__restrict__ obase = a.parity + (int64_t)P * R;

        uint32_t accp[P][8];
#pragma unroll
        for (int t = 0; t < P; t++)
#pragma unroll
            for (int pb = 0; pb < 8; pb++) accp[t][pb] = 0;
        /* software pipeline: the next PF rows' loads in flight during
         * this row's transpose + plane xors */
        uint32_t xq[PF + 1][8];
#pragma unroll
        for (int pf = 0; pf < PF && pf < D; pf++) {
            const uint8_t *row = sbase + (int64_t)pf * row_stride + j;
            uint4 lo = *(const uint4 *)row;
            uint4 hi = *(const uint4 *)(row + 16);
            xq[pf][0] = lo.x; xq[pf][1] = lo.y;
            xq[pf][2] = lo.z; xq[pf][3] = lo.w;
            xq[pf][4] = hi.x; xq[pf][5] = hi.y;
            xq[pf][6] = hi.z; xq[pf][7] = hi.w;
        }
#pragma unroll
        for (int k = 0; k < D; k++) {
            const int cur = k % (PF + 1);
            if (k + PF < D) {
                const int nxt = (k + PF) % (PF + 1);
                const uint8_t *row = sbase + (int64_t)(k + PF) * row_stride + j;
                uint4 lo = *(const uint4 *)row;
                uint4 hi = *(const uint4 *)(row + 16);
                xq[nxt][0] = lo.x; xq[nxt][1] = lo.y;
                xq[nxt][2] = lo.z; xq[nxt][3] = lo.w;
                xq[nxt][4] = hi.x; xq[nxt][5] = hi.y;
                xq[nxt][6] = hi.z; xq[nxt][7] = hi.w;
            }
            bs_transpose(xq[cur]);
            bs_acc_k<D, P, MAT>(k, xq[cur], accp);
        }
#pragma unroll
        for (int t = 0; t < P; t++) {
            bs_transpose(accp[t]);
            uint8_t *orow = obase + (int64_t)t * row_stride + j;
            typedef unsigned int v4u __attribute__((ext_vector_type(4)));
            v4u vlo = {accp[t][0], accp[t][1], accp[t][2], accp[t][3]};
            v4u vhi = {accp[t][4], accp[t][5], accp[t][6], accp[t][7]};
            __builtin_nontemporal_store(vlo, (v4u *)orow);
            __builtin_nontemporal_store(vhi, (v4u *)(orow + 16));
        }
    }
}

/* hh_quad.h's chain with the message length and the row pointer per chain:
 * slot = tid >> 2 names row slot % (d+p) of item order[slot / (d+p)], read
 * from the data or the parity buffer over exactly S_i bytes; its digest
 * goes to the fused slot (item*(d+p)+row)*32.
 *
 * The quad contract holds with per-chain lengths because the return, len
 * and the tail branch below depend on the chain alone (slot, S), never on
 * j.  Waves do diverge between chains of different lengths; the descending
 * order keeps the 16 chains of a wave near-equal. */
__global__ void __launch_bounds__(256) hh256_var_kernel(EncVarArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t slot = tid >> 2;
    const int j = (int)(tid & 3); /* this lane's HighwayHash lane index */
    const uint32_t total = (uint32_t)(a.d + a.p);
    if (slot >= (int64_t)a.n * total) return;
    /* n*(d+p) fits in 32 bits (planner) */
    const uint32_t oi = (uint32_t)slot / total;
    const uint32_t srow = (uint32_t)slot - oi * total;
    const int64_t item = (int64_t)a.order[oi];
    const int64_t R = a.items[2 * item];
    const int64_t S = a.items[2 * item + 1];
    const int64_t row_stride = (S + 63) & ~int64_t(63);
    const uint8_t *mp =
        (srow < (uint32_t)a.d
             ? a.data + (int64_t)a.d * R + (int64_t)srow * row_stride
             : a.parity + (int64_t)a.p * R +
                   (int64_t)(srow - (uint32_t)a.d) * row_stride) +
        8 * j;
    const uint32_t S3 = hh1_sel(j);

    HH1 s;
    hh1_init(s, a.key, j);
    int64_t len = S;
    HH1_STREAM(s, mp, len, S3)
    if (len > 0) hh1_remainder(s, mp, (int)len, j, S3);
    *(uint64_t *)(a.sums + (item * total + srow) * 32 + 8 * j) =
        hh1_finish(s, j, S3);
}

extern "C" int mec_encode_var_supported(int d, int p) {
#define X(D, P)                                                              \
    if (d == D && p == P) return 1;
    MEC_SPECIALIZED_GEOS(X)
#undef X
    return 0;
}

extern "C" hipError_t mec_launch_encode_var(const EncVarArgs *args,
                                            hipStream_t stream) {
    if (args->n == 0 || args->cols_total <= 0) return hipErrorInvalidValue;
    if (!mec_encode_var_supported(args->d, args->p))
        return hipErrorNotSupported;
    /* capped linear grid, the uniform launch's 2048*8 workgroups; the
     * grid-stride loop takes the rest */
    const int64_t want = (args->cols_total + 255) / 256;
    const int64_t cap = 2048 * 8;
    dim3 grid((uint32_t)(want < cap ? want : cap)), blk(256);
#define X(D, P)                                                              \
    if (args->d == D && args->p == P)                                        \
        hipLaunchKernelGGL(                                                  \
            (gf_encode_bs_var_kernel<D, P, MAT_##D##_##P, 2>), grid, blk, 0, \
            stream, *args);
    MEC_SPECIALIZED_GEOS(X)
#undef X
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || args->sums == nullptr) return e;
    /* 4 lanes per chain; n*(d+p) < 2^32 keeps the grid below 2^26 blocks */
    const int64_t lanes = (int64_t)args->n * (args->d + args->p) * 4;
    dim3 hgrid((uint32_t)((lanes + 255) / 256));
    hipLaunchKernelGGL(hh256_var_kernel, hgrid, blk, 0, stream, *args);
    return hipGetLastError();
}
