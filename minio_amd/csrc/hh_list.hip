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
 * Chain math and structure are hh256_batch4_kernel's (kernels.hip): 4 GPU
 * lanes per chain, quad-DPP zipper, 16-packet double-buffered prefetch,
 * len >= 32 loop, UpdateRemainder tail, 10 permute rounds.  Two things
 * differ:
 *  - the chain id comes from list[tid >> 2], so row and digest slot are
 *    shards + id*row_stride and sums + id*32;
 *  - verify mode compares each lane's 8-byte output word with the expected
 *    digest, ANDs the four verdicts across the quad and stores one byte at
 *    ok[id]; no digest is written.  Sum mode stores the digest words.
 * msg_len is uniform per launch, so waves never diverge in the packet
 * loops; a list length that is no multiple of 16 leaves whole quads
 * inactive, never part of one, so the quad DPP stays valid.
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
    const uint32_t S3 = (j & 1) ? 0x07000601u : 0x00070106u;

    const uint64_t init0[4] = {0xdbe6d5d5fe4cce2full, 0xa4093822299f31d0ull,
                               0x13198a2e03707344ull, 0x243f6a8885a308d3ull};
    const uint64_t init1[4] = {0x3bd39e10cb0ef593ull, 0xc0acf169b5f18a8cull,
                               0xbe5466cf34e90c6cull, 0x452821e638d01377ull};
    HH1 s;
    s.mul0 = init0[j];
    s.mul1 = init1[j];
    s.v0 = init0[j] ^ a.key[j];
    s.v1 = init1[j] ^ ((a.key[j] >> 32) | (a.key[j] << 32));

    int64_t len = a.msg_len;
    constexpr int DP = 16; /* prefetch depth (packets); 8 B each */
    uint64_t qa[DP], qb[DP];
#define HHL_LOAD(Q)                                                          \
    {                                                                        \
        _Pragma("unroll") for (int t = 0; t < DP; t++)                       \
            Q[t] = *(const uint64_t *)(mp + 32 * t);                         \
        mp += 32 * DP;                                                       \
    }
#define HHL_COMP(Q)                                                          \
    {                                                                        \
        _Pragma("unroll") for (int t = 0; t < DP; t++)                       \
            hh1_update(s, Q[t], S3);                                         \
    }
    __builtin_amdgcn_s_setprio(1);
    if (len >= 32 * DP) {
        HHL_LOAD(qa)
        len -= 32 * DP;
        while (len >= 2 * 32 * DP) {
            HHL_LOAD(qb)
            HHL_COMP(qa)
            HHL_LOAD(qa)
            HHL_COMP(qb)
            len -= 2 * 32 * DP;
        }
        if (len >= 32 * DP) {
            HHL_LOAD(qb)
            HHL_COMP(qa)
            HHL_COMP(qb)
            len -= 32 * DP;
        } else {
            HHL_COMP(qa)
        }
    }
#undef HHL_LOAD
#undef HHL_COMP
    __builtin_amdgcn_s_setprio(0);
    while (len >= 32) {
        uint64_t w = *(const uint64_t *)mp;
        hh1_update(s, w, S3);
        mp += 32;
        len -= 32;
    }
    if (RAGGED && len > 0) {
        /* UpdateRemainder, as in hh256_batch4_kernel: each lane builds the
         * padded 32-B packet privately and consumes its own 8-B word */
        const int mod32 = (int)len;
        const int mod4 = mod32 & 3;
        const uint8_t *tail_msg = mp - 8 * j;
        s.v0 += ((uint64_t)mod32 << 32) + (uint64_t)mod32;
        {
            uint32_t h0 = (uint32_t)s.v1;
            uint32_t h1 = (uint32_t)(s.v1 >> 32);
            s.v1 = (uint32_t)((h0 << mod32) | (h0 >> (32 - mod32)));
            s.v1 |= (uint64_t)((h1 << mod32) | (h1 >> (32 - mod32))) << 32;
        }
        uint8_t packet[32];
#pragma unroll
        for (int i = 0; i < 32; i++) packet[i] = 0;
        for (int i = 0; i < (mod32 & ~3); i++) packet[i] = tail_msg[i];
        const uint8_t *rem = tail_msg + (mod32 & ~3);
        if (mod32 & 16) {
            for (int i = 0; i < 4; i++)
                packet[28 + i] = rem[i + mod4 - 4];
        } else if (mod4) {
            packet[16] = rem[0];
            packet[17] = rem[mod4 >> 1];
            packet[18] = rem[mod4 - 1];
        }
        uint64_t w = 0;
        for (int bt = 7; bt >= 0; bt--) w = (w << 8) | packet[8 * j + bt];
        hh1_update(s, w, S3);
    }
    /* 10 permute-update rounds: permuted[j] = rot32(v0[j ^ 2]) */
#pragma unroll 1
    for (int r = 0; r < 10; r++) {
        uint32_t p_lo = dpp_swap2((uint32_t)s.v0);
        uint32_t p_hi = dpp_swap2((uint32_t)(s.v0 >> 32));
        hh1_update(s, ((uint64_t)p_lo << 32) | p_hi, S3);
    }
    /* modular reduction, as in hh256_batch4_kernel: lane j ends up with
     * digest word j */
    uint64_t t = s.v0 + s.mul0;
    uint64_t sv = s.v1 + s.mul1;
    uint32_t se_lo = dpp_swap1((uint32_t)sv);
    uint32_t se_hi = dpp_swap1((uint32_t)(sv >> 32));
    uint64_t se = ((uint64_t)se_hi << 32) | se_lo; /* partner's s */
    uint64_t out;
    if ((j & 1) == 0) {
        out = t ^ (sv << 1) ^ (sv << 2);
    } else {
        uint64_t a3 = sv & 0x3fffffffffffffffull;
        out = t ^ ((a3 << 1) | (se >> 63)) ^ ((a3 << 2) | (se >> 62));
    }
    uint8_t *slot_p = a.sums + id * 32 + 8 * j;
    if (VERIFY) {
        const uint64_t want = *(const uint64_t *)slot_p;
        uint32_t good = (out == want) ? 1u : 0u;
        good &= dpp_swap1(good); /* pair verdict */
        good &= dpp_swap2(good); /* quad verdict */
        if (j == 0) a.ok[id] = (uint8_t)good;
    } else {
        *(uint64_t *)slot_p = out;
    }
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
