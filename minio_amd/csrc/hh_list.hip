/* List-driven HighwayHash-256 for the verified batch read
 * (mec_verify_reconstruct_batch*): bitrot-check, or re-hash, only the rows
 * a device-resident list names.
 *
 * The reference verifies a shard block as it reads it
 * (streamingBitrotReader.ReadAt, cmd/bitrot-streaming.go:161-200) and reads
 * only d of the d+p rows unless one fails (parallelReader.Read,
 * cmd/erasure-decode.go:127-235).  A batch across objects therefore hashes
 * an irregular subset of the n*(d+p) rows in HBM: the subset is the list.
 *
 * The chain is hh_quad.h's (4 GPU lanes per chain).  These kernels own two
 * things:
 *  - the chain id comes from list[tid >> 2], so row and digest slot are
 *    shards + id*row_stride and sums + id*32;
 *  - verify mode compares each lane's 8-byte output word with the expected
 *    digest, ANDs the four verdicts across the quad and stores one byte at
 *    ok[id]; no digest is written.  Sum mode stores the digest words.
 *    (hh_quad.h's hh1_emit, shared with read_var.hip.)
 * msg_len is uniform per launch, so waves never diverge in the packet
 * loops; a list length that is no multiple of 16 leaves whole quads
 * inactive, never part of one, which is what hh_quad.h's quad contract asks.
 */
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"
#include "hh_quad.h"

template <bool RAGGED, bool VERIFY>
__device__ __forceinline__ void hh256_list_body(const HashListArgs &a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t slot = tid >> 2;
    const int j = (int)(tid & 3); /* this lane's HighwayHash lane index */
    if (slot >= (int64_t)a.n_list) return;
    const int64_t id = (int64_t)a.list[slot];
    const uint8_t *mp = a.shards + id * a.row_stride + 8 * j;
    const uint32_t S3 = hh1_sel(j);

    HH1 s;
    hh1_init(s, a.key, j);
    int64_t len = a.msg_len;
    HH1_STREAM(s, mp, len, S3)
    if (RAGGED && len > 0) hh1_remainder(s, mp, (int)len, j, S3);
    const uint64_t out = hh1_finish(s, j, S3);
    hh1_emit<VERIFY>(out, a.sums + id * 32 + 8 * j, a.ok + id, j);
}

/* two names, so a kernel trace tells the modes apart */
template <bool RAGGED>
__global__ void __launch_bounds__(256) hh256_list_verify(HashListArgs a) {
    hh256_list_body<RAGGED, true>(a);
}

template <bool RAGGED>
__global__ void __launch_bounds__(256) hh256_list_sum(HashListArgs a) {
    hh256_list_body<RAGGED, false>(a);
}

extern "C" hipError_t mec_launch_hash_list(const HashListArgs *args,
                                           int verify, hipStream_t stream) {
    if (args->n_list == 0) return hipSuccess;
    if (args->msg_len < 0) return hipErrorInvalidValue;
    /* 4 lanes per chain; n_list < 2^32 keeps the grid below 2^26 blocks */
    const int64_t lanes = (int64_t)args->n_list * 4;
    dim3 grid((uint32_t)((lanes + 255) / 256)), blk(256);
    const bool ragged = args->msg_len % 32 != 0;
    if (verify) {
        if (ragged)
            hipLaunchKernelGGL((hh256_list_verify<true>), grid, blk, 0,
                               stream, *args);
        else
            hipLaunchKernelGGL((hh256_list_verify<false>), grid, blk, 0,
                               stream, *args);
    } else {
        if (ragged)
            hipLaunchKernelGGL((hh256_list_sum<true>), grid, blk, 0, stream,
                               *args);
        else
            hipLaunchKernelGGL((hh256_list_sum<false>), grid, blk, 0, stream,
                               *args);
    }
    return hipGetLastError();
}
