/* Batch encode into on-disk [hash||shard] frames with a block length per
 * item (mec_encode_frames_batch_var*), MI355X (gfx950).
 *
 * Launches 1 and 2 are mec_encode_batch_var's (encode_var.hip): parity into
 * context scratch, digests into a context-owned sums table.  Launch 3, here,
 * packs the data rows, the parity rows and the digests into the layout of
 * frames_plan.h: d+p row streams, each the [hash||shard]* byte stream that
 * streamingBitrotWriter (cmd/bitrot-streaming.go:44-75) sends to a drive.
 * It is the per-item-length successor of stream_interleave_kernel
 * (kernels.hip) and the store-side twin of hh256_frames_verify_sheared
 * (hh_frames.hip).
 *
 * Work is flattened over the output: a thread owns one naturally aligned
 * 16-byte granule of `frames` per trip (frames_map.h has the mapping, shared
 * with the CPU checker), so 66000 frames of 33 bytes and one frame of
 * 128 KiB both fill their waves.  A wave takes per_wave consecutive groups
 * of 64 granules.  For the first it divides by F_n and searches the whole F
 * prefix, wave-uniformly; every further group starts 1 KiB behind the one
 * before, so inside a long frame it reads no table at all and otherwise
 * searches 32 entries (fm_wave_next).  When the group's 1 KiB ends inside
 * the frame it starts in, which is every group but a few per frame for long
 * shards, that is all; otherwise each lane searches the at most 32 frames
 * that follow.  (A grid-stride walk with the lower bound carried, as
 * gf_encode_bs_var_kernel has it, was measured first: at 1 KiB per trip the
 * log2(n) dependent table loads of every trip were most of the kernel's
 * time)
 *
 * Load bounds.  The row strides of the packed data and parity are multiples
 * of 64 and both buffers start 16-aligned, so a naturally aligned 16-byte
 * load that holds one byte of a row's own S_i bytes lies inside that row's
 * stride.  The comment at each load names such a byte, or the table entry.
 * Stores go to bytes of [frames, frames + total*F_n) only.
 */
#include <hip/hip_runtime.h>
#include <cstdint>

#include "frames_map.h"
#include "kernels.h"

__device__ __forceinline__ int64_t ef_sgpr64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi =
        __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

/* the wave state in scalar registers */
__device__ __forceinline__ void ef_uniform(mec::FmWave &w) {
    w.row = __builtin_amdgcn_readfirstlane(w.row);
    w.first = __builtin_amdgcn_readfirstlane(w.first);
    w.o0 = ef_sgpr64(w.o0);
    w.r0 = ef_sgpr64(w.r0);
    w.fs = ef_sgpr64(w.fs);
    w.fe = ef_sgpr64(w.fe);
    w.one = __builtin_amdgcn_readfirstlane((uint32_t)w.one) != 0;
}

/* One granule: dst is its 16 aligned bytes, R the row offset of m's item. */
__device__ __forceinline__ void ef_granule(const FramesPackArgs &a,
                                           const mec::FmGeom &g,
                                           const mec::FmGran &m, int64_t R,
                                           uint8_t *dst) {
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    if (m.body) {
        const mec::FmBody b = mec::fm_body(g, m, R);
        const uint8_t *base = m.row < g.d ? a.data : a.parity;
        /* src0 holds the row's byte k, src1 its byte k+15 < S_i (or is src0
         * again): fm_body */
        const uint4 q0 = *(const uint4 *)(base + b.src0);
        const uint4 q1 = *(const uint4 *)(base + b.src1);
        const uint32_t x[8] = {q0.x, q0.y, q0.z, q0.w,
                               q1.x, q1.y, q1.z, q1.w};
        uint32_t o[4];
        mec::fm_shear(x, b.sh, o);
        const v4u v = {o[0], o[1], o[2], o[3]};
        __builtin_nontemporal_store(v, (v4u *)dst);
        return;
    }
    const mec::FmBoundary b = mec::fm_boundary(g, m, R);
    const int nb = m.hi_b - m.lo_b;
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int rel = i - m.lo_b;
        if (rel >= 0 && rel < nb) {
            /* a digest byte of a frame's own 32, or a byte below S_i of
             * frame A's row: fm_byte */
            const mec::FmByte s = mec::fm_byte(b, rel);
            const uint8_t *base = s.where == mec::kFmSums   ? a.sums
                                  : s.where == mec::kFmData ? a.data
                                                            : a.parity;
            o[i >> 2] |= (uint32_t)base[s.off] << (8 * (i & 3));
        }
    }
    if (nb == 16) {
        const v4u v = {o[0], o[1], o[2], o[3]};
        __builtin_nontemporal_store(v, (v4u *)dst);
    } else {
        /* the buffer's first or last granule: its own bytes only */
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (i >= m.lo_b && i < m.hi_b)
                dst[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
    }
}

/* Lanes of one wave may belong to different frames and take different
 * paths (body, boundary).  Nothing after the wave state is cross-lane. */
__global__ void __launch_bounds__(256)
frames_pack_var_kernel(FramesPackArgs a) {
    const int64_t *__restrict__ F = a.frame_off;
    const int64_t *__restrict__ items = a.items;
    mec::FmGeom g;
    g.fn = a.fn;
    g.bytes = a.bytes;
    g.n = a.n;
    g.d = (uint32_t)a.d;
    g.p = (uint32_t)a.p;
    g.a0 = a.a0;
    /* granule q is the 16 bytes at out16 + 16q; only bytes at or above
     * a.out are ever stored */
    uint8_t *const out16 = a.out - a.a0;

    /* blockDim.x is a multiple of 64: the wave index is wave-uniform */
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave =
        ef_sgpr64(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t grp0 = wave * a.per_wave;
    if (grp0 >= a.groups) return;
    const int64_t grp1 =
        grp0 + a.per_wave < a.groups ? grp0 + a.per_wave : a.groups;

    /* F[1 .. n-1], then F[first], F[first+1], first <= n-1: table entries */
    mec::FmWave w = mec::fm_wave_first(g, F, grp0 * mec::kFmWave);
    uint32_t r_of = 0xFFFFFFFFu; /* the item whose row offset r_w holds */
    int64_t r_w = 0;
    for (int64_t grp = grp0;;) {
        ef_uniform(w);
        if (w.first != r_of) {
            r_of = w.first;
            r_w = ef_sgpr64(items[2 * (size_t)w.first]); /* first < n */
        }
        const int64_t q = grp * mec::kFmWave + lane;
        if (q < a.granules) {
            /* F[lo+1 .. hi], hi <= n-1, then F[item], F[item+1] */
            const mec::FmGran m = mec::fm_granule(g, F, w, q);
            const int64_t R = m.item == w.first
                                  ? r_w
                                  : items[2 * (size_t)m.item]; /* item < n */
            ef_granule(a, g, m, R, out16 + 16 * q);
        }
        if (++grp == grp1) break;
        /* F[lo+1 .. hi], hi <= n-1, then F[first], F[first+1] */
        w = mec::fm_wave_next(g, F, grp * mec::kFmWave, w);
    }
}

extern "C" hipError_t mec_launch_frames_pack(const FramesPackArgs *args_in,
                                             hipStream_t stream) {
    if (args_in->n == 0 || args_in->granules <= 0) return hipErrorInvalidValue;
    FramesPackArgs args = *args_in;
    /* at most 2048*8 workgroups of 4 waves, as mec_launch_encode_var's cap;
     * past that a wave takes more consecutive groups */
    args.groups = (args.granules + mec::kFmWave - 1) / mec::kFmWave;
    const int64_t max_waves = 2048 * 8 * 4;
    args.per_wave = (args.groups + max_waves - 1) / max_waves;
    const int64_t waves = (args.groups + args.per_wave - 1) / args.per_wave;
    dim3 grid((uint32_t)((waves + 3) / 4)), blk(256);
    hipLaunchKernelGGL(frames_pack_var_kernel, grid, blk, 0, stream, args);
    return hipGetLastError();
}
