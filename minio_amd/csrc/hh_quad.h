/* HighwayHash-256 at 4 GPU lanes per chain: the whole per-chain computation
 * (lane selector, init, packet update, streaming loop, UpdateRemainder,
 * finish).  Every HighwayHash kernel of the library is built from it:
 * hh256_batch4_kernel (kernels.hip), hh256_list_* (hh_list.hip),
 * hh256_var_kernel (encode_var.hip), hh256_list_var_* (read_var.hip) and
 * the hash waves of
 * fused4_encode_hh_kernel (fused4.hip), which brings its own packet loop.
 * Device code only; why 4 lanes per chain: see the comment above
 * hh256_batch4_kernel in kernels.hip.
 *
 * The quad contract.  GPU lane j (0..3) of a quad owns HighwayHash lane j of
 * one chain.  Every helper below except hh1_sel and hh1_init executes
 * quad-perm DPP, which takes values from the other lanes of the quad; an
 * inactive lane reads as zero (bound_ctrl) and yields a wrong digest with no
 * fault.  So the four lanes of a chain enter each helper together and take
 * the same loop trips: every branch, trip count and return around and inside
 * them depends on the chain alone (its length, its slot), never on j. */
#ifndef MEC_HH_QUAD_H
#define MEC_HH_QUAD_H

#include <hip/hip_runtime.h>
#include <cstdint>

__device__ __forceinline__ uint32_t permb(uint32_t hi, uint32_t lo,
                                          uint32_t sel) {
    return __builtin_amdgcn_perm(hi, lo, sel);
}

__device__ __forceinline__ uint32_t dpp_swap1(uint32_t v) {
    /* value from lane ^ 1 (zipper pair partner); quad_perm [1,0,3,2] */
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t dpp_swap2(uint32_t v) {
    /* value from lane ^ 2 (finalization permute); quad_perm [2,3,0,1] */
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);
}

struct HH1 {
    uint64_t v0, v1, mul0, mul1; /* this lane's single HighwayHash lane */
};

/* One packet update for HH lane j.
 *
 * The zipper merge is a pure byte permutation of a lane pair (the reference
 * implements it with pshufb); on CDNA4 that is v_perm_b32: 3 perms + 1 or
 * per output word instead of a ~17-op shift/mask tree.  With A = the even
 * lane's word and B = the odd lane's word of the pair:
 *   even lane out bytes (LSB..MSB): [A3 B4 A2 A5 | B6 A1 B7 A0]
 *   odd lane out bytes:             [B3 A4 B2 B5 | B1 A6 B0 A7]
 * v_perm pool = {hi:lo}, selector byte 12 yields 0x00.  Seen from either
 * lane the low word takes the same bytes of (own, partner's high word), so
 * its two selectors are parity-independent; only the high word's selector
 * S3 depends on lane parity (0x00070106 even, 0x07000601 odd). */
__device__ __forceinline__ void hh1_update(HH1 &s, uint64_t w, uint32_t S3) {
    s.v1 += s.mul0 + w;
    s.mul0 ^= (s.v1 & 0xffffffffull) * (s.v0 >> 32);
    s.v0 += s.mul1;
    s.mul1 ^= (s.v0 & 0xffffffffull) * (s.v1 >> 32);
    {
        uint32_t own_lo = (uint32_t)s.v1, own_hi = (uint32_t)(s.v1 >> 32);
        uint32_t p_hi = dpp_swap1(own_hi);
        uint32_t lo = permb(own_hi, own_lo, 0x05020C03u) |
                      permb(0u, p_hi, 0x0C0C000Cu);
        uint32_t hi = permb(p_hi, own_lo, S3);
        s.v0 += ((uint64_t)hi << 32) | lo;
    }
    {
        uint32_t own_lo = (uint32_t)s.v0, own_hi = (uint32_t)(s.v0 >> 32);
        uint32_t p_hi = dpp_swap1(own_hi);
        uint32_t lo = permb(own_hi, own_lo, 0x05020C03u) |
                      permb(0u, p_hi, 0x0C0C000Cu);
        uint32_t hi = permb(p_hi, own_lo, S3);
        s.v1 += ((uint64_t)hi << 32) | lo;
    }
}

/* v_perm selector of lane j's zipper high word (see hh1_update) */
__device__ __forceinline__ uint32_t hh1_sel(int j) {
    return (j & 1) ? 0x07000601u : 0x00070106u;
}

/* initial state of HighwayHash lane j under the 4-word key */
__device__ __forceinline__ void hh1_init(HH1 &s, const uint64_t *key, int j) {
    const uint64_t init0[4] = {0xdbe6d5d5fe4cce2full, 0xa4093822299f31d0ull,
                               0x13198a2e03707344ull, 0x243f6a8885a308d3ull};
    const uint64_t init1[4] = {0x3bd39e10cb0ef593ull, 0xc0acf169b5f18a8cull,
                               0xbe5466cf34e90c6cull, 0x452821e638d01377ull};
    s.mul0 = init0[j];
    s.mul1 = init1[j];
    s.v0 = init0[j] ^ key[j];
    s.v1 = init1[j] ^ ((key[j] >> 32) | (key[j] << 32));
}

/* Consume every whole 32-byte packet of the message: HH1_STREAM(s, mp, len,
 * S3) with s an HH1, mp this lane's pointer (chain base + 8*j, a
 * const uint8_t * variable) and len an int64_t variable; mp and len are left
 * at the tail, len < 32.  The first part keeps 16 packets in flight in one
 * register buffer while the other is hashed, at raised wave priority.
 *
 * A macro and not a function on purpose.  As a __forceinline__ function
 * (mp and len by reference, or everything by value and returned) the
 * compiler places the prefetch loads differently, and hh256_batch4_kernel
 * and hh256_var_kernel measured 5-10% slower on the MI355X; expanded in
 * place the kernels get the code they had when each carried its own copy. */
#define HH1_DP 16 /* prefetch depth (packets); 8 B each */
#define HH1_LOAD(Q, mp)                                                      \
    {                                                                        \
        _Pragma("unroll") for (int t = 0; t < HH1_DP; t++)                   \
            Q[t] = *(const uint64_t *)(mp + 32 * t);                         \
        mp += 32 * HH1_DP;                                                   \
    }
#define HH1_COMP(Q, s, S3)                                                   \
    {                                                                        \
        _Pragma("unroll") for (int t = 0; t < HH1_DP; t++)                   \
            hh1_update(s, Q[t], S3);                                         \
    }
#define HH1_STREAM(s, mp, len, S3)                                           \
    {                                                                        \
        uint64_t qa[HH1_DP], qb[HH1_DP];                                     \
        __builtin_amdgcn_s_setprio(1);                                       \
        if (len >= 32 * HH1_DP) {                                            \
            HH1_LOAD(qa, mp)                                                 \
            len -= 32 * HH1_DP;                                              \
            while (len >= 2 * 32 * HH1_DP) {                                 \
                HH1_LOAD(qb, mp)                                             \
                HH1_COMP(qa, s, S3)                                          \
                HH1_LOAD(qa, mp)                                             \
                HH1_COMP(qb, s, S3)                                          \
                len -= 2 * 32 * HH1_DP;                                      \
            }                                                                \
            if (len >= 32 * HH1_DP) {                                        \
                HH1_LOAD(qb, mp)                                             \
                HH1_COMP(qa, s, S3)                                          \
                HH1_COMP(qb, s, S3)                                          \
                len -= 32 * HH1_DP;                                          \
            } else {                                                         \
                HH1_COMP(qa, s, S3)                                          \
            }                                                                \
        }                                                                    \
        __builtin_amdgcn_s_setprio(0);                                       \
        while (len >= 32) {                                                  \
            hh1_update(s, *(const uint64_t *)mp, S3);                        \
            mp += 32;                                                        \
            len -= 32;                                                       \
        }                                                                    \
    }

/* UpdateRemainder's padded 32-byte packet for a tail of mod32 (1..31) bytes:
 *   [0, mod32 & ~3)      the tail's whole dwords,
 *   mod32 & 16:  [28,32) the tail's last 4 bytes,
 *   else mod4:   16,17,18 = rem[0], rem[mod4>>1], rem[mod4-1],
 *   zero elsewhere.
 * Returns the tail byte that packet byte q comes from, -1 for zero. */
__host__ __device__ constexpr int hh_tail_src(int q, int mod32) {
    const int mod4 = mod32 & 3, whole = mod32 & ~3;
    if (q < whole) return q;
    if (mod32 & 16) return q >= 28 ? mod32 - 32 + q : -1;
    if (mod4) {
        if (q == 16) return whole;
        if (q == 17) return whole + (mod4 >> 1);
        if (q == 18) return whole + mod4 - 1;
    }
    return -1;
}

/* Compile-time reference: the portable packet builder (published
 * semantics, the form the kernels used to run per lane), applied to a tail
 * whose byte i holds i.  It must give hh_tail_src's map for all 31 tail
 * lengths, and never read at or past mod32. */
constexpr bool hh_tail_src_matches_packet_builder() {
    for (int mod32 = 1; mod32 < 32; mod32++) {
        const int mod4 = mod32 & 3;
        int tail_msg[32] = {};
        for (int i = 0; i < 32; i++) tail_msg[i] = i;
        int packet[32] = {};
        for (int i = 0; i < 32; i++) packet[i] = -1;
        for (int i = 0; i < (mod32 & ~3); i++) packet[i] = tail_msg[i];
        const int *rem = tail_msg + (mod32 & ~3);
        if (mod32 & 16) {
            for (int i = 0; i < 4; i++) packet[28 + i] = rem[i + mod4 - 4];
        } else if (mod4) {
            packet[16] = rem[0];
            packet[17] = rem[mod4 >> 1];
            packet[18] = rem[mod4 - 1];
        }
        for (int q = 0; q < 32; q++)
            if (hh_tail_src(q, mod32) != packet[q] || packet[q] >= mod32)
                return false;
    }
    return true;
}
static_assert(hh_tail_src_matches_packet_builder(),
              "hh_tail_src disagrees with the portable UpdateRemainder");

/* UpdateRemainder for a tail of mod32 (1..31) bytes at mp (left there by
 * HH1_STREAM).  Each lane fetches only the 8 bytes of its own packet word,
 * and only message bytes [0, mod32) are read. */
__device__ __forceinline__ void hh1_remainder(HH1 &s, const uint8_t *mp,
                                              int mod32, int j, uint32_t S3) {
    const uint8_t *tail_msg = mp - 8 * j;
    s.v0 += ((uint64_t)mod32 << 32) + (uint64_t)mod32;
    {
        uint32_t h0 = (uint32_t)s.v1;
        uint32_t h1 = (uint32_t)(s.v1 >> 32);
        s.v1 = (uint32_t)((h0 << mod32) | (h0 >> (32 - mod32)));
        s.v1 |= (uint64_t)((h1 << mod32) | (h1 >> (32 - mod32))) << 32;
    }
    uint64_t w = 0;
#pragma unroll
    for (int bt = 7; bt >= 0; bt--) {
        const int src = hh_tail_src(8 * j + bt, mod32);
        /* tail_msg[0] is a message byte (mod32 > 0): load, then select */
        const uint32_t b = tail_msg[src < 0 ? 0 : src];
        w = (w << 8) | (src < 0 ? 0u : b);
    }
    hh1_update(s, w, S3);
}

/* The 10 permute rounds and the modular reduction; returns digest word j
 * (bytes [8j, 8j+8) of the 32-byte digest). */
__device__ __forceinline__ uint64_t hh1_finish(HH1 &s, int j, uint32_t S3) {
    /* permuted[j] = rot32(v0[j ^ 2]) — rot32 of the cross-pair partner is
     * just its halves swapped */
#pragma unroll 1
    for (int r = 0; r < 10; r++) {
        uint32_t p_lo = dpp_swap2((uint32_t)s.v0);
        uint32_t p_hi = dpp_swap2((uint32_t)(s.v0 >> 32));
        hh1_update(s, ((uint64_t)p_lo << 32) | p_hi, S3);
    }
    /* modular reduction: lanes {0,1} emit hash[0..1], {2,3} hash[2..3].
     * m for the pair needs a2 = s0 = partner-even's (v1+mul1):
     *   even lane j: out = t_j ^ (s_j << 1) ^ (s_j << 2)
     *   odd lane j:  out = t_j ^ ((s_j' << 1) | (s_e >> 63))
     *                          ^ ((s_j' << 2) | (s_e >> 62)),
     *   s_j' = s_j & 0x3fff..., s_e = even partner's s. */
    uint64_t t = s.v0 + s.mul0;
    uint64_t sv = s.v1 + s.mul1;
    uint32_t se_lo = dpp_swap1((uint32_t)sv);
    uint32_t se_hi = dpp_swap1((uint32_t)(sv >> 32));
    uint64_t se = ((uint64_t)se_hi << 32) | se_lo; /* partner's s */
    if ((j & 1) == 0) return t ^ (sv << 1) ^ (sv << 2);
    uint64_t a3 = sv & 0x3fffffffffffffffull;
    return t ^ ((a3 << 1) | (se >> 63)) ^ ((a3 << 2) | (se >> 62));
}

/* What the list-driven kernels (hh_list.hip, read_var.hip) do with digest
 * word `out` of lane j, slot_p being that word's place in the chain's
 * digest slot.  VERIFY: compare with the expected word, AND the four
 * verdicts across the quad and store one byte at *ok_p; no digest is
 * written.  Otherwise store the word.  The quad contract covers it: all
 * four lanes of the chain call it together. */
template <bool VERIFY>
__device__ __forceinline__ void hh1_emit(uint64_t out, uint8_t *slot_p,
                                         uint8_t *ok_p, int j) {
    if (VERIFY) {
        const uint64_t want = *(const uint64_t *)slot_p;
        uint32_t good = (out == want) ? 1u : 0u;
        good &= dpp_swap1(good); /* pair verdict */
        good &= dpp_swap2(good); /* quad verdict */
        if (j == 0) *ok_p = (uint8_t)good;
    } else {
        *(uint64_t *)slot_p = out;
    }
}

#endif
