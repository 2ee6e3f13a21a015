/* Bit-sliced GF(2^8) device helpers shared by the standalone encode and
 * matmul kernels (kernels.hip, encode_var.hip, recon_mixed.hip) and the GF
 * waves of the one-pass kernel (fused4.hip). */
#ifndef MEC_GF_BS_H
#define MEC_GF_BS_H
#include <hip/hip_runtime.h>
#include <cstdint>

/* ---- bit-sliced specialized encode (r2) --------------------------------
 *
 * The SWAR xtime ladder this replaced (r1; retired) costs
 * ~1.46 VALU per input byte (and the int-VALU
 * pipe measures ~4 cyc/instr on gfx950, making the GF leg VALU-PIPE-bound
 * at ~0.32 ms for the headline batch — r2 SQ counters).  Bit-slicing cuts
 * the instruction count ~2.4x: each lane takes a 32-byte column per row,
 * transposes it to 8 bit-planes (3-stage delta-swap network, an
 * involution — verified exhaustively on CPU), and then EVERY GF(2^8)
 * constant-multiply-accumulate is a straight-line XOR of planes with the
 * coefficient's bit-matrix rows folded at compile time (constexpr over
 * MAT): ~16 xors per (input,parity) pair instead of the ladder's ~90
 * slots.  Transposes: 60 ops per 32 B, amortized over P outputs.
 */
__device__ __forceinline__ void bs_pair(uint32_t &A, uint32_t &B, int s,
                                        uint32_t m) {
    /* delta-swap: exchanges bit groups between regs A and B */
    uint32_t t = (uint32_t)__builtin_amdgcn_bitop3_b32(B << s, A, m,
                                                       0x28); /* (b^a)&m */
    A ^= t;
    B ^= t >> s;
}

__device__ __forceinline__ void bs_transpose(uint32_t r[8]) {
    /* stages d=1,2,4: after this, r[b] holds bit b of all 32 bytes
     * (slot order is a fixed byte permutation, identical across planes;
     * the same network inverts it — involution) */
    bs_pair(r[0], r[1], 1, 0xAAAAAAAAu);
    bs_pair(r[2], r[3], 1, 0xAAAAAAAAu);
    bs_pair(r[4], r[5], 1, 0xAAAAAAAAu);
    bs_pair(r[6], r[7], 1, 0xAAAAAAAAu);
    bs_pair(r[0], r[2], 2, 0xCCCCCCCCu);
    bs_pair(r[1], r[3], 2, 0xCCCCCCCCu);
    bs_pair(r[4], r[6], 2, 0xCCCCCCCCu);
    bs_pair(r[5], r[7], 2, 0xCCCCCCCCu);
    bs_pair(r[0], r[4], 4, 0xF0F0F0F0u);
    bs_pair(r[1], r[5], 4, 0xF0F0F0F0u);
    bs_pair(r[2], r[6], 4, 0xF0F0F0F0u);
    bs_pair(r[3], r[7], 4, 0xF0F0F0F0u);
}

/* ---- the same transpose in 4 VALU per exchange --------------------------
 *
 * A delta-swap is shift, bitop3, xor, shift, xor.  The exchange it performs
 * is also two bit-field selects, each one v_bitop3 on a shifted operand:
 *   A' = (A & ~m) | ((B << s) & m)      B' = (B & m) | ((A >> s) & ~m)
 * (m >> s == ~m for the three stage masks): 48 operations per transpose
 * instead of 60.  The network is written once over an operation policy, so
 * that the device code and the compile-time proof below run the same stages
 * with the same truth tables. */
constexpr uint8_t BS_SEL_C_BA = 0xD8; /* bitop3(a, b, c): c ? b : a */
constexpr uint8_t BS_SEL_C_AB = 0xE4; /* bitop3(a, b, c): c ? a : b */

template <class Op>
__host__ __device__ constexpr void bs_pair4_net(uint32_t &A, uint32_t &B,
                                                int s, uint32_t m) {
    const uint32_t a = Op::bitop3(A, B << s, m, BS_SEL_C_BA);
    B = Op::bitop3(B, A >> s, m, BS_SEL_C_AB);
    A = a;
}

template <class Op>
__host__ __device__ constexpr void bs_transpose4_net(uint32_t r[8]) {
    bs_pair4_net<Op>(r[0], r[1], 1, 0xAAAAAAAAu);
    bs_pair4_net<Op>(r[2], r[3], 1, 0xAAAAAAAAu);
    bs_pair4_net<Op>(r[4], r[5], 1, 0xAAAAAAAAu);
    bs_pair4_net<Op>(r[6], r[7], 1, 0xAAAAAAAAu);
    bs_pair4_net<Op>(r[0], r[2], 2, 0xCCCCCCCCu);
    bs_pair4_net<Op>(r[1], r[3], 2, 0xCCCCCCCCu);
    bs_pair4_net<Op>(r[4], r[6], 2, 0xCCCCCCCCu);
    bs_pair4_net<Op>(r[5], r[7], 2, 0xCCCCCCCCu);
    bs_pair4_net<Op>(r[0], r[4], 4, 0xF0F0F0F0u);
    bs_pair4_net<Op>(r[1], r[5], 4, 0xF0F0F0F0u);
    bs_pair4_net<Op>(r[2], r[6], 4, 0xF0F0F0F0u);
    bs_pair4_net<Op>(r[3], r[7], 4, 0xF0F0F0F0u);
}

struct BsOpDevice {
    static __device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b,
                                                      uint32_t c,
                                                      uint8_t tbl) {
        /* the table must be an immediate */
        return tbl == BS_SEL_C_BA
                   ? (uint32_t)__builtin_amdgcn_bitop3_b32(a, b, c,
                                                           BS_SEL_C_BA)
                   : (uint32_t)__builtin_amdgcn_bitop3_b32(a, b, c,
                                                           BS_SEL_C_AB);
    }
};

/* v_bitop3_b32 as the ISA defines it: result bit = tbl[a*4 + b*2 + c] */
struct BsOpModel {
    static constexpr uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c,
                                     uint8_t tbl) {
        uint32_t r = 0;
        for (int idx = 0; idx < 8; idx++)
            if ((tbl >> idx) & 1)
                r |= ((idx & 4) ? a : ~a) & ((idx & 2) ? b : ~b) &
                     ((idx & 1) ? c : ~c);
        return r;
    }
};

/* bs_transpose's delta-swap network in plain C++, for the proof only */
constexpr void bs_transpose_model(uint32_t r[8]) {
    constexpr int ia[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
    constexpr int ib[12] = {1, 3, 5, 7, 2, 3, 6, 7, 4, 5, 6, 7};
    constexpr int sh[3] = {1, 2, 4};
    constexpr uint32_t mk[3] = {0xAAAAAAAAu, 0xCCCCCCCCu, 0xF0F0F0F0u};
    for (int e = 0; e < 12; e++) {
        const int s = sh[e / 4];
        const uint32_t t = ((r[ib[e]] << s) ^ r[ia[e]]) & mk[e / 4];
        r[ia[e]] ^= t;
        r[ib[e]] ^= t >> s;
    }
}

/* Both networks are linear over GF(2), so equality on the 256 single-bit
 * states (and on zero) is equality on every input; a few dense states ride
 * along.  Evaluated by every build, host and device pass. */
constexpr bool bs_transpose4_equals_delta_swap() {
    for (int n = 0; n < 256 + 8; n++) {
        uint32_t x[8] = {}, y[8] = {};
        if (n < 256) {
            x[n / 32] = 1u << (n % 32);
        } else {
            uint32_t v = 0x9E3779B9u * (uint32_t)(n - 255);
            for (int i = 0; i < 8; i++) {
                v ^= v << 13; v ^= v >> 17; v ^= v << 5;
                x[i] = v;
            }
        }
        for (int i = 0; i < 8; i++) y[i] = x[i];
        bs_transpose_model(x);
        bs_transpose4_net<BsOpModel>(y);
        for (int i = 0; i < 8; i++)
            if (x[i] != y[i]) return false;
    }
    return true;
}
static_assert(bs_transpose4_equals_delta_swap(),
              "the 4-operation transpose must equal bs_transpose");

__device__ __forceinline__ void bs_transpose4(uint32_t r[8]) {
    bs_transpose4_net<BsOpDevice>(r);
}

/* constexpr GF(2^8)/0x11D multiply and bit-matrix row masks */
constexpr uint8_t bs_gfmul(uint8_t a, uint8_t b) {
    uint32_t r = 0, x = a;
    for (int i = 0; i < 8; i++) {
        if ((b >> i) & 1) r ^= x << i;
    }
    /* reduce 15-bit poly product mod 0x11D */
    for (int i = 14; i >= 8; i--)
        if ((r >> i) & 1) r ^= 0x11Du << (i - 8);
    return (uint8_t)r;
}
/* rowmask(c, b) bit a: output bit b of c*x depends on input bit a */
constexpr uint8_t bs_rowmask(uint8_t c, int b) {
    uint8_t m = 0;
    for (int a = 0; a < 8; a++)
        if ((bs_gfmul(c, (uint8_t)(1u << a)) >> b) & 1)
            m |= (uint8_t)(1u << a);
    return m;
}

/* explicit xor3 pair-folding of a plane-XOR set (the compiler leaves
 * these as chains of v_xor otherwise — measured 1267 plain xors/loop) */
template <uint8_t M>
__device__ __forceinline__ uint32_t bs_fold(const uint32_t x[8],
                                            uint32_t acc) {
    if constexpr (M == 0) {
        return acc;
    } else {
        constexpr int a0 = __builtin_ctz(M);
        constexpr uint8_t M1 = M & (M - 1);
        if constexpr (M1 == 0) {
            return acc ^ x[a0];
        } else {
            constexpr int a1 = __builtin_ctz(M1);
            constexpr uint8_t M2 = M1 & (M1 - 1);
            return bs_fold<M2>(
                x, (uint32_t)__builtin_amdgcn_bitop3_b32(acc, x[a0], x[a1],
                                                         0x96));
        }
    }
}

/* compile-time iteration over (parity row, plane) so the fold masks are
 * constant expressions */
template <int D, int P, const uint8_t (&MAT)[P][D], int K, int I, int PB>
__device__ __forceinline__ void bs_acc_all(const uint32_t xc[8],
                                           uint32_t accp[P][8]) {
    if constexpr (I < P) {
        accp[I][PB] = bs_fold<bs_rowmask(MAT[I][K], PB)>(xc, accp[I][PB]);
        if constexpr (PB < 7)
            bs_acc_all<D, P, MAT, K, I, PB + 1>(xc, accp);
        else
            bs_acc_all<D, P, MAT, K, I + 1, 0>(xc, accp);
    }
}

template <int D, int P, const uint8_t (&MAT)[P][D], int K = 0>
__device__ __forceinline__ void bs_acc_k(int k, const uint32_t xc[8],
                                         uint32_t accp[P][8]) {
    if constexpr (K < D) {
        if (k == K)
            bs_acc_all<D, P, MAT, K, 0, 0>(xc, accp);
        else
            bs_acc_k<D, P, MAT, K + 1>(k, xc, accp);
    }
}


#endif /* MEC_GF_BS_H */
