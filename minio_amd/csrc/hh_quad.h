/* HighwayHash-256 at 4 GPU lanes per chain: the per-lane state and packet
 * update shared by hh256_batch4_kernel (kernels.hip) and the list-driven
 * kernels (hh_list.hip).  Device code only; why 4 lanes per chain, and the
 * byte layout behind the v_perm selectors: see the comments above
 * zip_even/zip_odd and hh256_batch4_kernel in kernels.hip. */
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

/* One packet update for HH lane j (lane parity selects the zipper hi
 * selector; S1/S2 are parity-independent — see zip_even/zip_odd, kernels.hip). */
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
