/* Batch scrub (mec_bitrot_verify_files*), MI355X (gfx950): HighwayHash-256
 * over the frames of on-disk shard files, hashed where they lie.
 *
 * bitrotVerify (cmd/bitrot.go:177-215) walks a [hash||shard]* file: frame k
 * of a file at shard size S starts at k*(32+S), 32 digest bytes and then the
 * message.  The files of a batch sit in one device buffer at byte offsets of
 * any alignment, and 32+S is odd for every ragged geometry (EC12+4:
 * S = 87382), so a message can start at any address.  The planner
 * (scrub_plan.h) splits the chains by that address:
 *
 *   hh256_frames_verify          message address % 8 == 0: the loop of
 *                                hh256_list_var_verify (read_var.hip), base
 *                                pointer, length and expected digest taken
 *                                from the file table;
 *   hh256_frames_verify_sheared  every other chain: only naturally aligned
 *                                qwords are loaded, and each lane's packet
 *                                word is sheared out of two of them with
 *                                v_alignbyte, the load-side twin of
 *                                stream_interleave_kernel (kernels.hip).
 *
 * Both are hh_quad.h's chain at 4 lanes per chain and keep its quad
 * contract: every branch and trip count below depends on the chain alone
 * (its list slot, its length, its address), never on the lane index j.
 * Where lane 3 differs from the others it differs by a select or by a load
 * address, not by control flow.
 *
 * Load bounds.  An allocation can end right behind the last file, so no load
 * may touch a naturally aligned 16-byte granule that holds no byte of the
 * chain's own file.  Every load here is naturally aligned and at most 8
 * bytes wide, so it lies within one granule; the comment at each load names
 * a byte of the chain's frame that the loaded qword contains.
 */
#include <hip/hip_runtime.h>
#include <cstdint>

#include "hh_quad.h"
#include "kernels.h"

/* what both kernels read per chain */
struct FrameChain {
    const uint8_t *msg; /* first message byte; the digest is the 32 before */
    int64_t len;        /* message bytes, >= 1 */
};

__device__ __forceinline__ FrameChain frame_chain(const HashFramesArgs &a,
                                                  int64_t slot) {
    const uint32_t file = a.list[2 * slot];
    const uint32_t frame = a.list[2 * slot + 1];
    const int64_t *row = a.table + 4 * (size_t)file;
    const int64_t off = row[0], S = row[1], last = row[2];
    const uint32_t frames = (uint32_t)row[3];
    FrameChain c;
    c.msg = a.files + off + (int64_t)frame * (32 + S) + 32;
    c.len = frame + 1 == frames ? last : S;
    return c;
}

/* hh1_emit<true>'s verdict with the expected word in a register */
__device__ __forceinline__ void hh1_verdict(uint64_t out, uint64_t want,
                                            uint8_t *ok_p, int j) {
    uint32_t good = (out == want) ? 1u : 0u;
    good &= dpp_swap1(good); /* pair verdict */
    good &= dpp_swap2(good); /* quad verdict */
    if (j == 0) *ok_p = (uint8_t)good;
}

__global__ void __launch_bounds__(256) hh256_frames_verify(HashFramesArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t slot = tid >> 2;
    const int j = (int)(tid & 3); /* this lane's HighwayHash lane index */
    if (slot >= (int64_t)a.n_list) return;
    const FrameChain c = frame_chain(a, slot);
    /* c.msg is a multiple of 8 (the planner's aligned list), so every
     * qword HH1_STREAM loads is naturally aligned and made of message bytes
     * only, and hh1_remainder loads single message bytes */
    const uint8_t *mp = c.msg + 8 * j;
    const uint32_t S3 = hh1_sel(j);

    HH1 s;
    hh1_init(s, a.key, j);
    int64_t len = c.len;
    HH1_STREAM(s, mp, len, S3)
    if (len > 0) hh1_remainder(s, mp, (int)len, j, S3);
    const uint64_t out = hh1_finish(s, j, S3);
    /* digest word j: bytes [8j, 8j+8) of the frame's 32-byte header, a
     * naturally aligned qword of digest bytes only */
    hh1_verdict(out, *(const uint64_t *)(c.msg - 32 + 8 * j), a.ok + slot, j);
}

/* ---- the sheared chain --------------------------------------------------
 *
 * A = the message address, sh8 = A % 8 (1..7 here), A8 = A - sh8.  With
 * W[i] the aligned qword at A8 + 8i, message word m (the 8 bytes at A + 8m)
 * is the 16 bytes {W[m+1]:W[m]} shifted right by sh8 bytes.  Lane j takes
 * word 4t + j of packet t: it loads W[4t+j] itself and gets W[4t+j+1] from
 * its quad neighbour j+1 by DPP.  Lane 3's upper qword W[4t+4] is lane 0's
 * qword of packet t+1, or, where packet t+1 is not loaded with packet t,
 * the packet's lookahead qword, which every lane of the quad loads from the
 * same address.
 *
 * The shift: v_alignbyte shears two dwords by 0..3 bytes; sh8 >= 4 moves
 * the three source dwords up by one first.  sh8 is per chain, so the shift
 * and the dword choice are VGPR operands and selects, not branches. */

struct Shear {
    uint32_t sh;  /* sh8 & 3: v_alignbyte's byte shift */
    bool hi4;     /* sh8 >= 4 */
    bool is3;     /* j == 3: the upper qword is not the neighbour's */
    int lk;       /* from a lane's qword pointer to its packet's lookahead */
};

__device__ __forceinline__ uint64_t hhs_rot1(uint64_t v) {
    /* value from lane (j + 1) & 3 of the quad; quad_perm [1,2,3,0] */
    const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp(
        (int)(uint32_t)v, 0x39, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp(
        (int)(uint32_t)(v >> 32), 0x39, 0xF, 0xF, true);
    return ((uint64_t)hi << 32) | lo;
}

/* bytes [sh8, sh8 + 8) of the 16 bytes {up:q} */
__device__ __forceinline__ uint64_t hhs_shear(uint64_t q, uint64_t up,
                                              const Shear &x) {
    const uint32_t a0 = (uint32_t)q, a1 = (uint32_t)(q >> 32);
    const uint32_t b0 = (uint32_t)up, b1 = (uint32_t)(up >> 32);
    const uint32_t x0 = x.hi4 ? a1 : a0;
    const uint32_t x1 = x.hi4 ? b0 : a1;
    const uint32_t x2 = x.hi4 ? b1 : b0;
    const uint32_t lo = __builtin_amdgcn_alignbyte(x1, x0, x.sh);
    const uint32_t hi = __builtin_amdgcn_alignbyte(x2, x1, x.sh);
    return ((uint64_t)hi << 32) | lo;
}

/* Lane j's word of the single 32-byte unit whose lane qword pointer is qp
 * (unit base & ~7, plus 8j); all four lanes of the chain call it together.
 * Bounds, with U the unit's first byte: the lane's qword holds byte
 * U + 8j, and the lookahead qword at (U + 31) & ~7 holds byte U + 31, both
 * bytes of the unit itself. */
__device__ __forceinline__ uint64_t hhs_word(const uint8_t *qp,
                                             const Shear &x) {
    const uint64_t q = *(const uint64_t *)qp;
    const uint64_t look = *(const uint64_t *)(qp + x.lk);
    const uint64_t nb = hhs_rot1(q);
    return hhs_shear(q, x.is3 ? look : nb, x);
}

/* HH1_STREAM's twin over aligned qwords: HHS_STREAM(s, qp, len, S3, x) with
 * qp the lane's qword pointer of packet 0 and len an int64_t variable; qp is
 * left at the tail's packet position and len < 32.  The same two-buffer ring
 * of 16 packets at raised wave priority, a macro for HH1_STREAM's reason.
 * Each buffer carries a 17th qword, the lookahead of its last packet.
 *
 * Bounds: HHS_LOAD runs only with 16 whole packets left.  Q[t] holds byte
 * 8j of packet t and Q[16], at (packet 15's base + 31) & ~7, holds packet
 * 15's last byte: message bytes all. */
#define HHS_LOAD(Q, qp, x)                                                   \
    {                                                                        \
        _Pragma("unroll") for (int t = 0; t < HH1_DP; t++)                   \
            Q[t] = *(const uint64_t *)(qp + 32 * t);                         \
        Q[HH1_DP] = *(const uint64_t *)(qp + x.lk + 32 * (HH1_DP - 1));      \
        qp += 32 * HH1_DP;                                                   \
    }
#define HHS_COMP(Q, s, S3, x)                                                \
    {                                                                        \
        uint64_t nb = hhs_rot1(Q[0]);                                        \
        _Pragma("unroll") for (int t = 0; t < HH1_DP; t++) {                 \
            /* lane 3's upper qword: lane 0's of the next packet */          \
            const uint64_t nx =                                              \
                t + 1 < HH1_DP ? hhs_rot1(Q[t + 1]) : Q[HH1_DP];             \
            hh1_update(s, hhs_shear(Q[t], x.is3 ? nx : nb, x), S3);          \
            nb = nx;                                                         \
        }                                                                    \
    }
#define HHS_STREAM(s, qp, len, S3, x)                                        \
    {                                                                        \
        uint64_t qa[HH1_DP + 1], qb[HH1_DP + 1];                             \
        __builtin_amdgcn_s_setprio(1);                                       \
        if (len >= 32 * HH1_DP) {                                            \
            HHS_LOAD(qa, qp, x)                                              \
            len -= 32 * HH1_DP;                                              \
            while (len >= 2 * 32 * HH1_DP) {                                 \
                HHS_LOAD(qb, qp, x)                                          \
                HHS_COMP(qa, s, S3, x)                                       \
                HHS_LOAD(qa, qp, x)                                          \
                HHS_COMP(qb, s, S3, x)                                       \
                len -= 2 * 32 * HH1_DP;                                      \
            }                                                                \
            if (len >= 32 * HH1_DP) {                                        \
                HHS_LOAD(qb, qp, x)                                          \
                HHS_COMP(qa, s, S3, x)                                       \
                HHS_COMP(qb, s, S3, x)                                       \
                len -= 32 * HH1_DP;                                          \
            } else {                                                         \
                HHS_COMP(qa, s, S3, x)                                       \
            }                                                                \
        }                                                                    \
        __builtin_amdgcn_s_setprio(0);                                       \
        while (len >= 32) {                                                  \
            /* a whole packet of the message: hhs_word's bounds */           \
            hh1_update(s, hhs_word(qp, x), S3);                              \
            qp += 32;                                                        \
            len -= 32;                                                       \
        }                                                                    \
    }

__global__ void __launch_bounds__(256)
hh256_frames_verify_sheared(HashFramesArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t slot = tid >> 2;
    const int j = (int)(tid & 3); /* this lane's HighwayHash lane index */
    if (slot >= (int64_t)a.n_list) return;
    const FrameChain c = frame_chain(a, slot);
    const uintptr_t A = (uintptr_t)c.msg;
    const uint32_t sh8 = (uint32_t)(A & 7);
    Shear x;
    x.sh = sh8 & 3;
    x.hi4 = sh8 >= 4;
    x.is3 = j == 3;
    /* (U + 31) & ~7 for a unit at U = A (mod 8): U - sh8 + 32, or + 24 for
     * sh8 == 0, where the upper qword is shifted out whole and any qword of
     * the unit will do */
    x.lk = (sh8 ? 32 : 24) - 8 * j;
    const uint8_t *qp = (const uint8_t *)(A - sh8) + 8 * j;
    const uint32_t S3 = hh1_sel(j);

    /* the expected digest is the 32-byte unit in front of the message, at
     * the message's own shift: hhs_word's bounds with U the frame's first
     * byte */
    const uint64_t want = hhs_word(qp - 32, x);

    HH1 s;
    hh1_init(s, a.key, j);
    int64_t len = c.len;
    HHS_STREAM(s, qp, len, S3, x)
    /* qp stands sh8 bytes below this lane's place in the tail;
     * hh1_remainder loads single bytes of the tail's [0, len) only */
    if (len > 0) hh1_remainder(s, qp + sh8, (int)len, j, S3);
    const uint64_t out = hh1_finish(s, j, S3);
    hh1_verdict(out, want, a.ok + slot, j);
}

extern "C" hipError_t mec_launch_hash_frames(const HashFramesArgs *args,
                                             int sheared,
                                             hipStream_t stream) {
    if (args->n_list == 0) return hipSuccess;
    /* 4 lanes per chain; n_list < 2^32 keeps the grid below 2^26 blocks */
    const int64_t lanes = (int64_t)args->n_list * 4;
    dim3 grid((uint32_t)((lanes + 255) / 256)), blk(256);
    if (sheared)
        hipLaunchKernelGGL(hh256_frames_verify_sheared, grid, blk, 0, stream,
                           *args);
    else
        hipLaunchKernelGGL(hh256_frames_verify, grid, blk, 0, stream, *args);
    return hipGetLastError();
}
