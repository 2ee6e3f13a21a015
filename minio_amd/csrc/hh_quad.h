/* HighwayHash-256 at 4 GPU lanes per chain: the per-lane state and packet
 * update shared by hh256_batch4_kernel (kernels.hip) and the list-driven
 * kernels (hh_list.hip).  Device code only; why 4 lanes per chain: see the
 * comment above hh256_batch4_kernel in kernels.hip. */
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

#endif
