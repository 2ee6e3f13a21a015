/* MI355X (gfx950, CDNA4) kernels for the MinIO erasure+bitrot hot path.
 *
 * Replaces the compute of:
 *  - reedsolomon.Encoder.Encode / Reconstruct (GF(2^8) shard arithmetic;
 *    reference call sites cmd/erasure-coding.go:85,106,112) —
 *    BIT-SLICED kernels (gf_encode_bs_kernel constexpr networks,
 *    gf_matmul_bs_kernel runtime bit-matrices; gf_bs.h).
 *    No MFMA: this is byte/integer work.
 *  - streamingBitrotWriter's per-shard hash (cmd/bitrot-streaming.go:57-59)
 *    and BitrotAlgorithm.New digests (cmd/bitrot.go:47-64) — HighwayHash
 *    at 4 GPU lanes per chain (hh256_batch4_kernel), SHA-256 (16-round
 *    body), BLAKE2b-512; hashing is sequential per shard, parallelism comes
 *    from shards x blocks x lanes-per-chain (SURVEY.md §7 hard part (b)).
 *
 * One kernel per operation lives here.  Encode + HighwayHash goes to the
 * one-pass kernel of fused4.hip when it is eligible; otherwise encode and
 * hash run as the two kernels of this file back to back — the bit-sliced
 * GF encode at ~90% of the HBM floor and the 4-lane HighwayHash at ~97% of
 * its memory floor while simultaneously at the per-wave VALU issue cadence
 * (profiles/probes_r2_valu.txt).  Cross-batch pipelining of
 * the pair is kept behind MEC_PIPE=1; the C-ABI signature treats the pair
 * as one fused operation either way.  The variants that were measured and
 * lost (ladder GF, pair-lane and LDS-staged hash, 64-round SHA body, the
 * earlier fused kernels) are recorded in DESIGN.md §9 and live in git
 * history only.
 */
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"
#include "hh_quad.h" /* the HighwayHash chain, 4 lanes each */

/* gfx950 3-input boolean LUT op (1 full-rate VALU slot) */
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); /* a^b^c */
}

/* ---- specialized encode kernels (constexpr matrix) ---------------------
 *
 * For the common geometries the encode matrix is baked in at compile time
 * (ec_matrices_gen.h, generated from the product's own matrix builder), so
 * the inner loop is a straight-line XOR schedule over bit planes (gf_bs.h):
 * no per-bit branches and no coefficient loads. */
#include "ec_matrices_gen.h"

#include "gf_bs.h"

/* PF: rows of load prefetch ahead of the transpose+fold; launched with
 * kEncPrefetch.  NT: nontemporal parity stores (parity is written once,
 * never re-read by this kernel). */
template <int D, int P, const uint8_t (&MAT)[P][D], bool NT, int PF = 1>
__global__ void __launch_bounds__(256) gf_encode_bs_kernel(GfEncArgs a) {
    const int b = blockIdx.y;
    const int64_t cols = (a.shard_len + 31) / 32;
    const uint8_t *__restrict__ sbase = a.data + (int64_t)b * D * a.row_stride;
    uint8_t *__restrict__ obase = a.parity + (int64_t)b * P * a.row_stride;

    for (int64_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cols;
         c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = c * 32;
        uint32_t accp[P][8];
#pragma unroll
        for (int i = 0; i < P; i++)
#pragma unroll
            for (int pb = 0; pb < 8; pb++) accp[i][pb] = 0;
        /* software pipeline: the next PF rows' loads in flight during
         * this row's transpose + plane xors */
        uint32_t xq[PF + 1][8];
#pragma unroll
        for (int pf = 0; pf < PF && pf < D; pf++) {
            const uint8_t *row = sbase + (int64_t)pf * a.row_stride + j;
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
                const uint8_t *row =
                    sbase + (int64_t)(k + PF) * a.row_stride + j;
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
        for (int i = 0; i < P; i++) {
            bs_transpose(accp[i]);
            uint8_t *orow = obase + (int64_t)i * a.row_stride + j;
            uint4 lo{accp[i][0], accp[i][1], accp[i][2], accp[i][3]};
            uint4 hi{accp[i][4], accp[i][5], accp[i][6], accp[i][7]};
            if (NT) {
                typedef unsigned int v4u __attribute__((ext_vector_type(4)));
                v4u vlo = {lo.x, lo.y, lo.z, lo.w};
                v4u vhi = {hi.x, hi.y, hi.z, hi.w};
                __builtin_nontemporal_store(vlo, (v4u *)orow);
                __builtin_nontemporal_store(vhi, (v4u *)(orow + 16));
            } else {
                *(uint4 *)orow = lo;
                *(uint4 *)(orow + 16) = hi;
            }
        }
    }
}

/* ---- bit-sliced generic matmul (runtime matrices) ----------------------
 *
 * out[t][j] = sum_k mat[t][k] * src[k][j]  (GF(2^8)), per batch item.
 * Works for encode (src = data rows, out = parity rows) and reconstruct
 * (src = surviving rows, out = missing rows) via row index lists.
 * E = number of output rows (template so accumulators stay in registers).
 *
 * Same plane-transpose trick as gf_encode_bs_kernel, but the matrix is
 * only known at run time, so the per-(output,plane) XOR selection uses
 * 0/~0 masks ((x & m) ^ acc as one v_bitop3) instead of compile-time
 * folds: 64 VALU per (src,dst) pair per 32 B regardless of matrix density.
 * Masks are built host-side (mec::bs_pack_matrix) and read through L1
 * (2 dwords per (t,k), hot after the first column). */
template <int E>
__global__ void __launch_bounds__(256) gf_matmul_bs_kernel(GfMatmulArgs a) {
    const int b = blockIdx.y;
    const int64_t cols = (a.shard_len + 31) / 32;
    const uint8_t *__restrict__ sbase = a.src + (int64_t)b * a.src_item_stride;
    uint8_t *__restrict__ obase = a.dst + (int64_t)b * a.dst_item_stride;

    for (int64_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cols;
         c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = c * 32;
        uint32_t accp[E][8];
#pragma unroll
        for (int i = 0; i < E; i++)
#pragma unroll
            for (int pb = 0; pb < 8; pb++) accp[i][pb] = 0;
        uint32_t xc[8], xn[8];
        {
            const uint8_t *row = sbase + (int64_t)a.src_rows[0] * a.row_stride + j;
            uint4 lo = *(const uint4 *)row;
            uint4 hi = *(const uint4 *)(row + 16);
            xc[0] = lo.x; xc[1] = lo.y; xc[2] = lo.z; xc[3] = lo.w;
            xc[4] = hi.x; xc[5] = hi.y; xc[6] = hi.z; xc[7] = hi.w;
        }
        for (int k = 0; k < a.d; k++) {
            if (k + 1 < a.d) {
                const uint8_t *row =
                    sbase + (int64_t)a.src_rows[k + 1] * a.row_stride + j;
                uint4 lo = *(const uint4 *)row;
                uint4 hi = *(const uint4 *)(row + 16);
                xn[0] = lo.x; xn[1] = lo.y; xn[2] = lo.z; xn[3] = lo.w;
                xn[4] = hi.x; xn[5] = hi.y; xn[6] = hi.z; xn[7] = hi.w;
            }
            bs_transpose(xc);
#pragma unroll
            for (int i = 0; i < E; i++) {
                /* the 8x8 bit matrix of mat[i][k], 2 dwords; loaded once
                 * per (i,k) and moved to SGPRs so the per-element mask
                 * expansion runs on the SCALAR pipe concurrently with the
                 * VALU — leaving exactly ONE v_bitop3 per matrix element
                 * (skipping zero bits with wave-uniform branches measured
                 * no better) */
                const uint32_t *m = a.bs_masks + ((int64_t)i * a.d + k) * 2;
                const uint32_t mlo = __builtin_amdgcn_readfirstlane(m[0]);
                const uint32_t mhi = __builtin_amdgcn_readfirstlane(m[1]);
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
            for (int w = 0; w < 8; w++) xc[w] = xn[w];
        }
#pragma unroll
        for (int i = 0; i < E; i++) {
            bs_transpose(accp[i]);
            uint8_t *orow = obase + (int64_t)a.dst_rows[i] * a.row_stride + j;
            /* nontemporal: rebuilt rows are written once and never
             * re-read by this kernel (reads and writes hit the SAME
             * in-place buffer — keeping stores out of the cache reduces
             * the read/write turnaround that parks 42% of wave-cycles,
             * gpurun decsq SQ pass) */
            typedef unsigned int v4u __attribute__((ext_vector_type(4)));
            v4u vlo = {accp[i][0], accp[i][1], accp[i][2], accp[i][3]};
            v4u vhi = {accp[i][4], accp[i][5], accp[i][6], accp[i][7]};
            __builtin_nontemporal_store(vlo, (v4u *)orow);
            __builtin_nontemporal_store(vhi, (v4u *)(orow + 16));
        }
    }
}

/* ---- HighwayHash-256 ---------------------------------------------------
 * Portable algorithm as published (minio/highwayhash v1.0.3 semantics,
 * magic key passed from host; pinned by tests/golden/bitrot_selftest.json).
 */

/* Map chain index -> (shard pointer, sum slot) for the fused encode
 * layout.  Sums always use the n x (d+p) layout regardless of mode, so
 * data-only + parity-only launches compose to the single-launch result. */
__device__ __forceinline__ const uint8_t *chain_ptr(const HashArgs &a,
                                                    int64_t chain,
                                                    int64_t &sum_idx) {
    if (a.parity == nullptr) {
        sum_idx = chain;
        return a.data + chain * a.row_stride;
    }
    const int total = a.d + a.p;
    if (a.mode == MEC_HASH_DATA) {
        const int64_t b = chain / a.d;
        const int s = (int)(chain % a.d);
        sum_idx = b * total + s;
        return a.data + (b * a.d + s) * a.row_stride;
    }
    if (a.mode == MEC_HASH_PARITY) {
        const int64_t b = chain / a.p;
        const int s = (int)(chain % a.p);
        sum_idx = b * total + a.d + s;
        return a.parity + (b * a.p + s) * a.row_stride;
    }
    const int64_t b = chain / total;
    const int s = (int)(chain % total);
    sum_idx = chain;
    if (s < a.d)
        return a.data + (b * a.d + s) * a.row_stride;
    return a.parity + (b * a.p + (s - a.d)) * a.row_stride;
}

/* ---- HighwayHash-256, 4 lanes per chain ---------------------------------
 *
 * Why 4 GPU lanes per chain instead of a pair-lane split (2 lanes per
 * chain, each owning one zipper pair — the r1 kernel, retired): at the
 * headline chain count (12288) the pair kernel is 384 waves — only 96 CUs
 * at WG 256 — and its ISA shows ~69 VALU/packet per lane (64-bit adds,
 * zipper perms, word re-packing), so each wave alone on its SIMD pays
 * dependency latency (~265 cyc/packet measured vs 138 issue floor) while
 * only ~96 CUs' worth of load bandwidth is engaged (the WG-512 "2
 * waves/SIMD" variant measured WORSE because it halved the engaged CUs —
 * per-CU global-load bandwidth ~10 B/cyc is the real wall).  Splitting
 * each chain over 4 lanes (one HighwayHash lane each):
 *  - doubles the wave count (768 waves -> ~192 CUs engaged),
 *  - cuts per-lane work to ~27 VALU/packet (zipper needs only the
 *    partner's v1/v0 HIGH word: one quad-perm DPP mov per phase, and the
 *    even/odd zipper variants collapse to one code path with a per-lane
 *    v_perm selector),
 *  - loads 8 B/lane/packet (dwordx2), same coalescing (a chain's 4 lanes
 *    cover its 32-B packet contiguously).
 * The chain itself (init, streaming loop, UpdateRemainder, finish) is
 * hh_quad.h's, shared by every HighwayHash kernel; this one owns chain_ptr
 * and the store.
 */

template <bool RAGGED, int WG = 256>
__global__ void __launch_bounds__(WG) hh256_batch4_kernel(HashArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t chain = tid >> 2;
    const int j = (int)(tid & 3); /* this lane's HighwayHash lane index */
    if (chain >= a.n_chains) return;
    int64_t sum_idx;
    const uint8_t *mp = chain_ptr(a, chain, sum_idx) + 8 * j;
    const uint32_t S3 = hh1_sel(j);

    HH1 s;
    hh1_init(s, a.key, j);
    int64_t len = a.msg_len;
    HH1_STREAM(s, mp, len, S3)
    if (RAGGED && len > 0) hh1_remainder(s, mp, (int)len, j, S3);
    *(uint64_t *)(a.sums + sum_idx * 32 + 8 * j) = hh1_finish(s, j, S3);
}

/* ---- SHA-256 (one chain per lane), FIPS 180-4 -------------------------- */

/* constexpr (not __constant__): the rounds are fully unrolled with
 * literal indices, so K folds to inline literal operands — as a
 * __constant__ buffer the compiler preloaded round constants into SGPRs
 * (measured 44-88 spilled SGPRs in the NC=2 kernels, r2) */
__device__ constexpr uint32_t SHA_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1,
    0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
    0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
    0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b,
    0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
    0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t rotr32(uint32_t x, int n) {
    return (x >> n) | (x << (32 - n));
}

__device__ __forceinline__ uint32_t bswap32(uint32_t v) {
    return __builtin_bswap32(v);
}

__device__ void sha256_block(uint32_t h[8], const uint32_t w_in[16]) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = w_in[i];
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5],
             g = h[6], hh = h[7];
    /* full unroll: every w[] index must be compile-time, or the 16-word
     * rolling schedule spills to scratch (measured 144 B/lane, 20x slower) */
#pragma unroll
    for (int i = 0; i < 64; i++) {
        uint32_t wi;
        if (i < 16) {
            wi = w[i];
        } else {
            uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
            uint32_t s0 = xor3(rotr32(w15, 7), rotr32(w15, 18), w15 >> 3);
            uint32_t s1 = xor3(rotr32(w2, 17), rotr32(w2, 19), w2 >> 10);
            wi = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
            w[i & 15] = wi;
        }
        /* Ch/Maj/Sigma as single v_bitop3_b32 LUT ops (gfx950): Ch and
         * Maj sit ON the round's dependency chain, so this shortens the
         * critical path as well as the issue count */
        uint32_t S1 = xor3(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25));
        uint32_t ch = __builtin_amdgcn_bitop3_b32(e, f, g, 0xca);
        uint32_t t1 = hh + S1 + ch + SHA_K[i] + wi;
        uint32_t S0 = xor3(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22));
        uint32_t maj = __builtin_amdgcn_bitop3_b32(a, b, c, 0xe8);
        uint32_t t2 = S0 + maj;
        hh = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
    h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

/* 16-round-body variant: the fully-unrolled 64-round loop at NC=2 is a
 * ~12 KiB body — big enough that co-resident waves thrash the 32 KiB
 * I-cache (r2: NC2 at WG512 measured 1.8x SLOWER than 1 wave/SIMD).
 * Rolling to a 16-round body (schedule indices stay static mod 16, the
 * a..h renaming closes every 8 rounds) cuts the body 4x; K for rounds
 * 16..63 comes from scalar loads of the rodata table. */
template <int NC, int LB = 256>
__global__ void __launch_bounds__(LB, 1) sha256_batch_r16_kernel(HashArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t c0 = tid * NC;
    if (c0 >= a.n_chains) return;

    bool act[NC];
    const uint8_t *mp[NC];
    int64_t sum_idx[NC];
    uint32_t h[NC][8];
#pragma unroll
    for (int u = 0; u < NC; u++) {
        act[u] = c0 + u < a.n_chains;
        mp[u] = chain_ptr(a, act[u] ? c0 + u : c0, sum_idx[u]);
        const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372,
                                0xa54ff53a, 0x510e527f, 0x9b05688c,
                                0x1f83d9ab, 0x5be0cd19};
#pragma unroll
        for (int i = 0; i < 8; i++) h[u][i] = iv[i];
    }
    int64_t len = a.msg_len;
    /* message double-buffer: the next 64-B block's loads ride under this
     * block's 64 rounds instead of stalling at each block boundary */
    uint4 mb[NC][4], mbn[NC][4];
    if (len >= 64) {
#pragma unroll
        for (int u = 0; u < NC; u++) {
            const uint4 *p = (const uint4 *)mp[u];
#pragma unroll
            for (int q = 0; q < 4; q++) mb[u][q] = p[q];
            mp[u] += 64;
        }
    }
    while (len >= 64) {
        if (len >= 128) {
#pragma unroll
            for (int u = 0; u < NC; u++) {
                const uint4 *p = (const uint4 *)mp[u];
#pragma unroll
                for (int q = 0; q < 4; q++) mbn[u][q] = p[q];
                mp[u] += 64;
            }
        }
        uint32_t w[NC][16];
#pragma unroll
        for (int u = 0; u < NC; u++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                w[u][4 * q + 0] = bswap32(mb[u][q].x);
                w[u][4 * q + 1] = bswap32(mb[u][q].y);
                w[u][4 * q + 2] = bswap32(mb[u][q].z);
                w[u][4 * q + 3] = bswap32(mb[u][q].w);
            }
        }
        uint32_t A[NC], B[NC], C[NC], D[NC], E[NC], F[NC], G[NC], H[NC];
#pragma unroll
        for (int u = 0; u < NC; u++) {
            A[u] = h[u][0]; B[u] = h[u][1]; C[u] = h[u][2]; D[u] = h[u][3];
            E[u] = h[u][4]; F[u] = h[u][5]; G[u] = h[u][6]; H[u] = h[u][7];
        }
#define SHA_ROUND(u, wi, kk)                                                 \
        {                                                                    \
            uint32_t S1 = xor3(rotr32(E[u], 6), rotr32(E[u], 11),            \
                               rotr32(E[u], 25));                            \
            uint32_t ch = (uint32_t)__builtin_amdgcn_bitop3_b32(             \
                E[u], F[u], G[u], 0xca);                                     \
            uint32_t t1 = H[u] + S1 + ch + (kk) + (wi);                      \
            uint32_t S0 = xor3(rotr32(A[u], 2), rotr32(A[u], 13),            \
                               rotr32(A[u], 22));                            \
            uint32_t maj = (uint32_t)__builtin_amdgcn_bitop3_b32(            \
                A[u], B[u], C[u], 0xe8);                                     \
            uint32_t t2 = S0 + maj;                                          \
            H[u] = G[u]; G[u] = F[u]; F[u] = E[u]; E[u] = D[u] + t1;         \
            D[u] = C[u]; C[u] = B[u]; B[u] = A[u]; A[u] = t1 + t2;           \
        }
        /* rounds 0..15: message words direct, K folds to literals */
#pragma unroll
        for (int r = 0; r < 16; r++)
#pragma unroll
            for (int u = 0; u < NC; u++) SHA_ROUND(u, w[u][r], SHA_K[r]);
        /* rounds 16..63: three passes of a 16-round body */
#pragma unroll 1
        for (int q = 1; q < 4; q++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t kk = SHA_K[(q << 4) + r];
#pragma unroll
                for (int u = 0; u < NC; u++) {
                    uint32_t w15 = w[u][(r + 1) & 15], w2 = w[u][(r + 14) & 15];
                    uint32_t s0 = xor3(rotr32(w15, 7), rotr32(w15, 18),
                                       w15 >> 3);
                    uint32_t s1 = xor3(rotr32(w2, 17), rotr32(w2, 19),
                                       w2 >> 10);
                    uint32_t wi = w[u][r] + s0 + w[u][(r + 9) & 15] + s1;
                    w[u][r] = wi;
                    SHA_ROUND(u, wi, kk);
                }
            }
        }
#undef SHA_ROUND
#pragma unroll
        for (int u = 0; u < NC; u++) {
            h[u][0] += A[u]; h[u][1] += B[u]; h[u][2] += C[u]; h[u][3] += D[u];
            h[u][4] += E[u]; h[u][5] += F[u]; h[u][6] += G[u]; h[u][7] += H[u];
        }
        if (len >= 128) {
#pragma unroll
            for (int u = 0; u < NC; u++)
#pragma unroll
                for (int q = 0; q < 4; q++) mb[u][q] = mbn[u][q];
        }
        len -= 64;
    }
    /* the double-buffer advanced mp one block past the remainder */
#pragma unroll
    for (int u = 0; u < NC; u++)
        mp[u] = chain_ptr(a, act[u] ? c0 + u : c0, sum_idx[u]) +
                (a.msg_len - len);
    /* tail: rem bytes + 0x80 pad + 8-byte big-endian bit length */
#pragma unroll
    for (int u = 0; u < NC; u++) {
        uint8_t tail[128];
#pragma unroll
        for (int i = 0; i < 128; i++) tail[i] = 0;
        for (int i = 0; i < (int)len; i++) tail[i] = mp[u][i];
        tail[(int)len] = 0x80;
        const int tlen = (len < 56) ? 64 : 128;
        uint64_t bits = (uint64_t)a.msg_len * 8;
        for (int i = 0; i < 8; i++)
            tail[tlen - 1 - i] = (uint8_t)(bits >> (8 * i));
        for (int blk = 0; blk < tlen; blk += 64) {
            uint32_t wt[16];
            for (int i = 0; i < 16; i++) {
                const uint8_t *q = tail + blk + 4 * i;
                wt[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) |
                        ((uint32_t)q[2] << 8) | q[3];
            }
            sha256_block(h[u], wt);
        }
        if (act[u]) {
            uint8_t *out = a.sums + sum_idx[u] * 32;
            for (int i = 0; i < 8; i++)
                *(uint32_t *)(out + 4 * i) = bswap32(h[u][i]);
        }
    }
}

/* ---- BLAKE2b-512 (one chain per lane), RFC 7693 ------------------------ */

__constant__ uint64_t B2B_IV[8] = {
    0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
    0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
    0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};

__constant__ uint8_t B2B_SIGMA[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
    {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
    {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13},
    {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11},
    {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},
    {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
    {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};

__device__ __forceinline__ uint64_t rotr64d(uint64_t x, int n) {
    return (x >> n) | (x << (64 - n));
}

__device__ void b2b_compress(uint64_t h[8], const uint64_t m[16], uint64_t t,
                             bool last) {
    uint64_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = h[i];
#pragma unroll
    for (int i = 0; i < 8; i++) v[8 + i] = B2B_IV[i];
    v[12] ^= t;
    if (last) v[14] = ~v[14];
#pragma unroll 1
    for (int r = 0; r < 12; r++) {
        const uint8_t *sg = B2B_SIGMA[r];
#define B2B_G(ai, bi, ci, di, x, y)                                          \
    {                                                                        \
        v[ai] = v[ai] + v[bi] + (x);                                         \
        v[di] = rotr64d(v[di] ^ v[ai], 32);                                  \
        v[ci] = v[ci] + v[di];                                               \
        v[bi] = rotr64d(v[bi] ^ v[ci], 24);                                  \
        v[ai] = v[ai] + v[bi] + (y);                                         \
        v[di] = rotr64d(v[di] ^ v[ai], 16);                                  \
        v[ci] = v[ci] + v[di];                                               \
        v[bi] = rotr64d(v[bi] ^ v[ci], 63);                                  \
    }
        B2B_G(0, 4, 8, 12, m[sg[0]], m[sg[1]]);
        B2B_G(1, 5, 9, 13, m[sg[2]], m[sg[3]]);
        B2B_G(2, 6, 10, 14, m[sg[4]], m[sg[5]]);
        B2B_G(3, 7, 11, 15, m[sg[6]], m[sg[7]]);
        B2B_G(0, 5, 10, 15, m[sg[8]], m[sg[9]]);
        B2B_G(1, 6, 11, 12, m[sg[10]], m[sg[11]]);
        B2B_G(2, 7, 8, 13, m[sg[12]], m[sg[13]]);
        B2B_G(3, 4, 9, 14, m[sg[14]], m[sg[15]]);
#undef B2B_G
    }
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}

__global__ void __launch_bounds__(256) blake2b512_batch_kernel(HashArgs a) {
    const int64_t chain = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (chain >= a.n_chains) return;
    int64_t sum_idx;
    const uint8_t *msg = chain_ptr(a, chain, sum_idx);

    uint64_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = B2B_IV[i];
    h[0] ^= 0x01010000ull ^ 64;
    int64_t off = 0;
    /* message double-buffer (r2, same treatment as SHA r16): the next
     * 128-B block's loads ride under this block's 12 rounds */
    uint64_t mA[16], mB[16];
#define B2B_LOAD(M, OFF)                                                     \
    {                                                                        \
        const uint4 *p = (const uint4 *)(msg + (OFF));                       \
        _Pragma("unroll") for (int q = 0; q < 8; q++) {                      \
            uint4 v = p[q];                                                  \
            M[2 * q] = (uint64_t)v.x | ((uint64_t)v.y << 32);                \
            M[2 * q + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);            \
        }                                                                    \
    }
    if (a.msg_len - off > 128) B2B_LOAD(mA, off)
    while (a.msg_len - off > 128) {
        if (a.msg_len - (off + 128) > 128) B2B_LOAD(mB, off + 128)
        b2b_compress(h, mA, (uint64_t)(off + 128), false);
        if (a.msg_len - (off + 128) > 128) {
#pragma unroll
            for (int i = 0; i < 16; i++) mA[i] = mB[i];
        }
        off += 128;
    }
#undef B2B_LOAD
    uint64_t m[16];
    {
        const int rem = (int)(a.msg_len - off);
        uint8_t tail[128];
#pragma unroll
        for (int i = 0; i < 128; i++) tail[i] = 0;
        for (int i = 0; i < rem; i++) tail[i] = msg[off + i];
        for (int i = 0; i < 16; i++) {
            uint64_t v = 0;
            for (int bt = 7; bt >= 0; bt--) v = (v << 8) | tail[8 * i + bt];
            m[i] = v;
        }
        b2b_compress(h, m, (uint64_t)a.msg_len, true);
    }
    uint8_t *out = a.sums + sum_idx * 64;
    for (int i = 0; i < 8; i++) *(uint64_t *)(out + 8 * i) = h[i];
}


/* ---- streaming-format device assembly -------------------
 * scatter_rows: packed object bytes -> padded strided shard rows (Split
 * semantics done on-device, cmd/erasure-coding.go:81).
 * stream_interleave: rows + sums -> per-drive on-disk [hash||shard]*
 * streams (cmd/bitrot-streaming.go:57-75) in one device buffer. */

__global__ void __launch_bounds__(256) scatter_rows_kernel(ScatterArgs a) {
    /* one 16-B slot per thread over n*d*ceil(S/16) */
    const int64_t per_row = (a.S + 15) >> 4;
    const int64_t total = a.n * a.d * per_row;
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         u < total; u += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = u / (a.d * per_row);
        const int64_t r = u % (a.d * per_row);
        const int k = (int)(r / per_row);
        const int64_t o = (r % per_row) * 16;
        const int64_t src_off = (int64_t)k * a.S + o;
        uint4 v = uint4{0, 0, 0, 0};
        const uint8_t *sp = a.src + b * a.block_len + src_off;
        if (src_off + 16 <= a.block_len) {
            /* interior slot: byte-wise safe unaligned gather is avoided by
             * the packed layout being arbitrary — use 4-B loads (packed
             * source has no 16-B alignment guarantee at shard boundaries) */
            const uint32_t *p4 = (const uint32_t *)sp;
            if (((uintptr_t)sp & 3) == 0) {
                v.x = p4[0]; v.y = p4[1]; v.z = p4[2]; v.w = p4[3];
            } else {
                alignas(16) uint8_t tmp[16];
                for (int i = 0; i < 16; i++) tmp[i] = sp[i];
                v = *(uint4 *)tmp;
            }
        } else if (src_off < a.block_len) {
            alignas(16) uint8_t tmp[16] = {0};
            const int have = (int)(a.block_len - src_off);
            for (int i = 0; i < have; i++) tmp[i] = sp[i];
            v = *(uint4 *)tmp;
        }
        *(uint4 *)&a.rows[(b * a.d + k) * a.row_stride + o] = v;
    }
}

__global__ void __launch_bounds__(256) stream_interleave_kernel(
    InterleaveArgs a) {
    /* One workgroup per [hash||shard] entry (drive s, block b).  The
     * entry's destination base (s*n+b)*pitch is byte-arbitrary whenever
     * pitch = 32+S is odd (every ragged-S geometry, e.g. EC12+4), so the
     * r1 version fell back to byte-wise copies for exactly those
     * geometries.  Here stores are always aligned
     * 16-B dwordx4 to the dst: a head/tail handles the odd edges
     * byte-wise, and the body gathers each 16 output bytes from two
     * aligned source loads sheared with v_alignbyte (constant shift per
     * entry). */
    const int total = a.d + a.p;
    const int64_t pitch = 32 + a.S;
    const int64_t e = blockIdx.x;          /* entry: s = e/n, b = e%n */
    const int s = (int)(e / a.n);
    const int64_t b = e % a.n;
    if (s >= total) return;
    uint8_t *dst = a.out + e * pitch;
    const uint8_t *h = a.sums + (b * total + s) * 32;
    const uint8_t *row = (s < a.d)
        ? a.data + (b * a.d + s) * a.row_stride
        : a.parity + (b * a.p + (s - a.d)) * a.row_stride;
    const int t = (int)threadIdx.x;
    /* hash half: 32 B, byte-wise (arbitrary dst alignment, tiny) */
    if (t < 32) dst[t] = h[t];
    /* shard: dst offset 32, src row 16-B aligned */
    uint8_t *sd = dst + 32;
    const int head = (int)((16 - ((uintptr_t)sd & 15)) & 15);
    const int64_t S = a.S;
    /* head + tail bytes */
    for (int64_t i = t; i < head && i < S; i += blockDim.x) sd[i] = row[i];
    const int64_t units = (S - head) / 16;   /* full 16-B dst units */
    for (int64_t i = head + units * 16 + t; i < S; i += blockDim.x)
        sd[i] = row[i];
    /* body: dst 16-B aligned; src at constant misalignment sh */
    const int sh = head & 15;
    const int dw = sh >> 2, bo = sh & 3;
    for (int64_t u = t; u < units; u += blockDim.x) {
        const int64_t off = head + u * 16;
        const int64_t base = off & ~(int64_t)15;
        if (base + 32 <= a.row_stride) {
            uint4 q0 = *(const uint4 *)(row + base);
            uint4 q1 = *(const uint4 *)(row + base + 16);
            uint32_t d8[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z,
                              q1.w};
            uint4 o;
            /* out dword i = bytes [off+4i, off+4i+4): alignbyte shears
             * the concat {hi:lo} right by bo bytes */
            o.x = __builtin_amdgcn_alignbyte(d8[dw + 1], d8[dw + 0], bo);
            o.y = __builtin_amdgcn_alignbyte(d8[dw + 2], d8[dw + 1], bo);
            o.z = __builtin_amdgcn_alignbyte(d8[dw + 3], d8[dw + 2], bo);
            o.w = __builtin_amdgcn_alignbyte(d8[dw + 4], d8[dw + 3], bo);
            *(uint4 *)(sd + off) = o;
        } else {
            /* last unit of the last row may not have 32 readable source
             * bytes within the stride: byte-wise */
            for (int i2 = 0; i2 < 16; i2++) sd[off + i2] = row[off + i2];
        }
    }
}

/* ---- launch wrappers (called from ec_abi.cpp) -------------------------- */

/* Launch shapes.  Each is the winner of a measured sweep;
 * the GF kernels are grid-stride, launched with grid scale * 2048
 * workgroups in all but never more than the work. */
constexpr int kWg = 256;           /* workgroup size, every kernel here */
constexpr int kEncGridScale = 8;   /* bit-sliced encode */
constexpr int kEncPrefetch = 2;    /* gf_encode_bs_kernel PF */
constexpr int kMatmulGridScale = 4;
constexpr int kShaChains = 2;      /* sha256_batch_r16_kernel NC */

static dim3 gf_grid(int64_t shard_len, int grid_scale, int n) {
    const int64_t cols = (shard_len + 31) / 32; /* 32 B per lane */
    int64_t max_x = (cols + kWg - 1) / kWg;
    int64_t want_x = ((int64_t)2048 * grid_scale + n - 1) / n;
    int64_t blocks_x = want_x < max_x ? want_x : max_x;
    if (blocks_x < 1) blocks_x = 1;
    return dim3((uint32_t)blocks_x, n);
}

/* The GF kernels take the batch item from blockIdx.y, and a grid's y
 * dimension is limited to 65535: a larger batch goes out in slices of at
 * most that many items, each with its own gf_grid and its base pointers
 * advanced by the item strides.  Every batch up to the limit is one launch,
 * as before. */
constexpr int kMaxGridY = 65535;

extern "C" {

/* Specialized encode launch; returns hipErrorNotSupported when (d,p) has no
 * compiled specialization (caller falls back to the generic kernel). */
hipError_t mec_launch_gf_encode_spec(int d, int p, const GfEncArgs *args,
                                     int n, hipStream_t stream) {
#define X(D, P)                                                              \
    if (d == D && p == P) {                                                  \
        for (int b0 = 0; b0 < n; b0 += kMaxGridY) {                          \
            const int nb = n - b0 < kMaxGridY ? n - b0 : kMaxGridY;          \
            GfEncArgs sl = *args;                                            \
            sl.data += (int64_t)b0 * D * args->row_stride;                   \
            sl.parity += (int64_t)b0 * P * args->row_stride;                 \
            hipLaunchKernelGGL(                                              \
                (gf_encode_bs_kernel<D, P, MAT_##D##_##P, true,              \
                                     kEncPrefetch>),                         \
                gf_grid(args->shard_len, kEncGridScale, nb), dim3(kWg), 0,   \
                stream, sl);                                                 \
            const hipError_t e = hipGetLastError();                          \
            if (e != hipSuccess) return e;                                   \
        }                                                                    \
        return hipSuccess;                                                   \
    }
    MEC_SPECIALIZED_GEOS(X)
#undef X
    return hipErrorNotSupported;
}

hipError_t mec_launch_gf_matmul(const GfMatmulArgs *args, int n_dst, int n,
                                hipStream_t stream) {
    if (args->bs_masks == nullptr) return hipErrorInvalidValue;
    for (int b0 = 0; b0 < n; b0 += kMaxGridY) {
        const int nb = n - b0 < kMaxGridY ? n - b0 : kMaxGridY;
        GfMatmulArgs sl = *args;
        sl.src += (int64_t)b0 * args->src_item_stride;
        sl.dst += (int64_t)b0 * args->dst_item_stride;
        const dim3 grid = gf_grid(args->shard_len, kMatmulGridScale, nb);
#define CASE(E)                                                              \
    case E:                                                                  \
        hipLaunchKernelGGL((gf_matmul_bs_kernel<E>), grid, dim3(kWg), 0,     \
                           stream, sl);                                      \
        break;
        switch (n_dst) {
            CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
        default:
            return hipErrorInvalidValue;
        }
#undef CASE
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t mec_launch_scatter_rows(const ScatterArgs *args,
                                   hipStream_t stream) {
    const int64_t per_row = (args->S + 15) >> 4;
    int64_t units = args->n * args->d * per_row;
    int64_t blocks = (units + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((uint32_t)blocks), dim3(256),
                       0, stream, *args);
    return hipGetLastError();
}

hipError_t mec_launch_stream_interleave(const InterleaveArgs *args,
                                        hipStream_t stream) {
    int64_t entries = (int64_t)(args->d + args->p) * args->n;
    hipLaunchKernelGGL(stream_interleave_kernel, dim3((uint32_t)entries),
                       dim3(256), 0, stream, *args);
    return hipGetLastError();
}

hipError_t mec_launch_hash(int algo, const HashArgs *args,
                           hipStream_t stream) {
    const dim3 blk(kWg);
    switch (algo) {
    case 1: { /* SHA256: the round chain is serial, so kShaChains chains
                 interleaved per lane fill its dependency stalls */
        const int64_t lanes = (args->n_chains + kShaChains - 1) / kShaChains;
        dim3 grid((uint32_t)((lanes + kWg - 1) / kWg));
        hipLaunchKernelGGL((sha256_batch_r16_kernel<kShaChains>), grid, blk,
                           0, stream, *args);
        break;
    }
    case 2:   /* HighwayHash256 */
    case 3: { /* HighwayHash256S: 4 lanes per chain; 32-aligned lengths
                 get the kernel with the ragged-tail code compiled out */
        const int64_t lanes = args->n_chains * 4;
        dim3 grid((uint32_t)((lanes + kWg - 1) / kWg));
        if (args->msg_len % 32 == 0)
            hipLaunchKernelGGL((hh256_batch4_kernel<false, kWg>), grid, blk,
                               0, stream, *args);
        else
            hipLaunchKernelGGL((hh256_batch4_kernel<true, kWg>), grid, blk,
                               0, stream, *args);
        break;
    }
    case 4: { /* BLAKE2b512: one chain per lane */
        dim3 grid((uint32_t)((args->n_chains + kWg - 1) / kWg));
        hipLaunchKernelGGL(blake2b512_batch_kernel, grid, blk, 0, stream,
                           *args);
        break;
    }
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
}
