/* Where every byte of mec_encode_frames_batch_var*'s output comes from: the
 * mapping from a 16-byte granule of `frames` to its row stream, its frame,
 * its source and its kind.  One implementation for frames_pack_var_kernel
 * (encode_frames.hip) and for the CPU checker tools/frames_plan_check.cpp,
 * so it is plain C++ with no HIP includes; under hipcc the functions are
 * __host__ __device__.
 *
 * Output layout (frames_plan.h): total = d+p row streams of F_n bytes each,
 * row s at s*F_n; in it the frame of item i at F_i: 32 digest bytes, then
 * the S_i = F_{i+1} - F_i - 32 shard bytes.
 *
 * Granules.  `frames` may have any byte alignment, a0 = address % 16.  With
 * v = a0 + (byte offset in frames), granule q is v in [16q, 16q + 16): a
 * naturally aligned 16 bytes of memory.  There are ceil((a0 + bytes)/16) of
 * them; the first holds no buffer byte below v = a0 and the last none from
 * v = a0 + bytes on.  A frame is at least 33 bytes, so a granule holds at
 * most one frame edge (row-stream edges are frame edges) and so bytes of at
 * most two frames, and the bytes of the second are digest bytes.
 *
 *   body granule      all 16 bytes are shard bytes of one frame: one
 *                     aligned 16-byte store, gathered from the 16-aligned
 *                     source row by two aligned loads and a byte shear
 *   boundary granule  everything else (a digest, a frame edge, a row-stream
 *                     edge, the buffer's first or last bytes): byte-wise
 */
#ifndef MEC_FRAMES_MAP_H
#define MEC_FRAMES_MAP_H

#include <cstdint>

#if defined(__HIPCC__)
#define MEC_HD __host__ __device__ __forceinline__
#else
#define MEC_HD inline
#endif

namespace mec {

/* granules per wave, and the bytes they span */
constexpr int kFmWave = 64;
constexpr int64_t kFmWaveBytes = 16 * kFmWave;
/* a frame is 32 + S_i >= 33 bytes: the frames that start within one wave's
 * span, rounded up */
constexpr uint32_t kFmWaveFrames = 32;
static_assert(kFmWaveBytes / 33 < kFmWaveFrames, "per-lane search window");

struct FmGeom {
    int64_t fn;     /* F_n: bytes per row stream */
    int64_t bytes;  /* total * F_n */
    uint32_t n;
    uint32_t d, p;
    uint32_t a0;    /* frames address % 16 */
};

MEC_HD int64_t fm_granules(const FmGeom &g) {
    return (g.a0 + g.bytes + 15) >> 4;
}

/* largest i in [lo, hi] with F[i] <= r; the caller guarantees F[lo] <= r.
 * Loads F[lo+1 .. hi] at most: hi <= n - 1 keeps them inside the n+1
 * entries. */
MEC_HD uint32_t fm_find(const int64_t *F, uint32_t lo, uint32_t hi,
                        int64_t r) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (F[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

/* What the 64 granules q0 .. q0+63 of a wave share (q0 a multiple of 64,
 * below fm_granules): the row stream and the frame of the wave's first
 * buffer byte. */
struct FmWave {
    uint32_t row;   /* row stream of the first byte */
    uint32_t first; /* its frame */
    int64_t o0;     /* the first byte's offset in frames */
    int64_t r0;     /* and in its row stream */
    int64_t fs, fe; /* F[first], F[first+1] */
    bool one;       /* every byte of the wave lies in that one frame */
};

/* A wave walks consecutive groups of 64 granules.  Its first group costs a
 * division and a binary search over the whole prefix ... */
MEC_HD FmWave fm_wave_first(const FmGeom &g, const int64_t *F, int64_t q0) {
    FmWave w;
    const int64_t o_lo = 16 * q0 - (int64_t)g.a0;
    w.o0 = o_lo < 0 ? 0 : o_lo; /* negative in granule 0 only */
    w.row = (uint32_t)(w.o0 / g.fn);
    w.r0 = w.o0 - (int64_t)w.row * g.fn;
    w.first = fm_find(F, 0, g.n - 1, w.r0);
    w.fs = F[w.first];
    w.fe = F[w.first + 1]; /* first <= n-1: inside the n+1 entries */
    /* the wave's last byte is at most o0 + 1023 */
    w.one = w.r0 + kFmWaveBytes <= w.fe;
    return w;
}

/* ... and every further one, q0 = the previous q0 + 64, starts at most 1024
 * bytes behind the previous start: inside a long frame no table is read at
 * all, otherwise the frame is one of the next 32 (or, in a later row stream,
 * of the first 32). */
MEC_HD FmWave fm_wave_next(const FmGeom &g, const int64_t *F, int64_t q0,
                           const FmWave &prev) {
    FmWave w = prev;
    w.o0 = 16 * q0 - (int64_t)g.a0; /* q0 >= 64 */
    w.r0 = prev.r0 + (w.o0 - prev.o0);
    if (w.r0 >= prev.fe) {
        uint32_t lo = prev.first;
        if (w.r0 >= g.fn) {
            do {
                w.r0 -= g.fn;
                w.row++;
            } while (w.r0 >= g.fn);
            lo = 0;
        }
        const uint32_t last = g.n - 1;
        const uint32_t hi = last - lo > kFmWaveFrames ? lo + kFmWaveFrames
                                                      : last;
        w.first = fm_find(F, lo, hi, w.r0);
        w.fs = F[w.first];
        w.fe = F[w.first + 1];
    }
    w.one = w.r0 + kFmWaveBytes <= w.fe;
    return w;
}

struct FmGran {
    uint32_t row, item; /* frame of the granule's first buffer byte */
    int lo_b, hi_b;     /* its buffer bytes are [lo_b, hi_b) of the 16 */
    int64_t r;          /* the first buffer byte's offset in its row stream */
    int64_t fs, fe;     /* F[item], F[item+1] */
    bool body;
};

/* q in [q0, q0 + 64), q < fm_granules */
MEC_HD FmGran fm_granule(const FmGeom &g, const int64_t *F, const FmWave &w,
                         int64_t q) {
    FmGran m;
    const int64_t o_lo = 16 * q - (int64_t)g.a0;
    m.lo_b = o_lo < 0 ? (int)-o_lo : 0;
    const int64_t left = g.bytes - o_lo; /* >= 1 */
    m.hi_b = left < 16 ? (int)left : 16;
    const int64_t o = o_lo + m.lo_b;
    m.row = w.row;
    m.item = w.first;
    m.r = w.r0 + (o - w.o0);
    m.fs = w.fs;
    m.fe = w.fe;
    if (!w.one) {
        /* at most 1023 bytes past r0: at most 31 row streams further */
        while (m.r >= g.fn) {
            m.r -= g.fn;
            m.row++;
        }
        /* in the wave's row the frame is one of the 32 from `first` on, in
         * a later row (r < 1024 + 15) one of the first 32 */
        const uint32_t lo = m.row == w.row ? w.first : 0;
        const uint32_t last = g.n - 1;
        const uint32_t hi = last - lo > kFmWaveFrames ? lo + kFmWaveFrames
                                                      : last;
        m.item = fm_find(F, lo, hi, m.r);
        m.fs = F[m.item];
        m.fe = F[m.item + 1]; /* item <= n-1 */
    }
    m.body = m.lo_b == 0 && m.hi_b == 16 && m.r - m.fs >= 32 &&
             m.r + 16 <= m.fe;
    return m;
}

MEC_HD int64_t fm_stride(int64_t S) { return (S + 63) & ~int64_t(63); }

/* byte offset of row `row` of an item with row offset R and shard length S
 * in the packed data buffer (row < d) or the packed parity buffer */
MEC_HD int64_t fm_row_off(const FmGeom &g, uint32_t row, int64_t R,
                          int64_t S) {
    return row < g.d ? (int64_t)g.d * R + (int64_t)row * fm_stride(S)
                     : (int64_t)g.p * R + (int64_t)(row - g.d) * fm_stride(S);
}

MEC_HD int64_t fm_sum_off(const FmGeom &g, uint32_t row, uint32_t item) {
    return ((int64_t)item * (g.d + g.p) + row) * 32;
}

/* ---- body granules ------------------------------------------------------
 * The granule's 16 bytes are bytes [k, k+16) of the source row, k in
 * [0, S-16].  The row starts 64-aligned, so with sh = k % 16 they lie in the
 * aligned 16 bytes at k - sh and, where sh != 0, in the next 16 too. */
struct FmBody {
    int64_t src0;  /* offset in the row's buffer of the first aligned load */
    int64_t src1;  /* of the second: src0 + 16, or src0 again for sh == 0 */
    uint32_t sh;
};

MEC_HD FmBody fm_body(const FmGeom &g, const FmGran &m, int64_t R) {
    const int64_t S = m.fe - m.fs - 32;
    const int64_t k = m.r - m.fs - 32;
    FmBody b;
    b.sh = (uint32_t)k & 15;
    /* src0 holds row byte k.  src1: for sh != 0 it holds row byte k + 15,
     * which is below S, so both loads are inside the row's stride (a
     * multiple of 16).  For sh == 0 the window [k+16, k+32) may start at
     * the stride's end (k = S - 16 with S a multiple of 64), so the second
     * load repeats the first; its bytes are shifted out. */
    b.src0 = fm_row_off(g, m.row, R, S) + (k - b.sh);
    b.src1 = b.src0 + (b.sh ? 16 : 0);
    return b;
}

MEC_HD uint32_t fm_alignbyte(uint32_t hi, uint32_t lo, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, b);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (b & 3)));
#endif
}

/* o = bytes [sh, sh+16) of the 32 bytes x (little-endian dwords).  sh differs
 * per thread, so the dword choice is two levels of selects and the byte
 * shift a register operand: no branch, no indexed register array. */
MEC_HD void fm_shear(const uint32_t x[8], uint32_t sh, uint32_t o[4]) {
    const bool by2 = (sh & 8) != 0, by1 = (sh & 4) != 0;
    /* written out: every register index is a constant */
    const uint32_t y0 = by2 ? x[2] : x[0], y1 = by2 ? x[3] : x[1];
    const uint32_t y2 = by2 ? x[4] : x[2], y3 = by2 ? x[5] : x[3];
    const uint32_t y4 = by2 ? x[6] : x[4], y5 = by2 ? x[7] : x[5];
    const uint32_t z0 = by1 ? y1 : y0, z1 = by1 ? y2 : y1;
    const uint32_t z2 = by1 ? y3 : y2, z3 = by1 ? y4 : y3;
    const uint32_t z4 = by1 ? y5 : y4;
    const uint32_t bo = sh & 3;
    o[0] = fm_alignbyte(z1, z0, bo);
    o[1] = fm_alignbyte(z2, z1, bo);
    o[2] = fm_alignbyte(z3, z2, bo);
    o[3] = fm_alignbyte(z4, z3, bo);
}

/* ---- boundary granules --------------------------------------------------
 * Buffer byte `rel` (0-based from the granule's first buffer byte) belongs
 * to frame A = (row, item) while rel < edge, else to the frame that follows
 * it in memory: item+1 of the same row stream, or item 0 of the next. */
struct FmBoundary {
    int64_t wa;    /* the first byte's offset in frame A, digest included */
    int64_t edge;  /* bytes from it to frame A's end, >= 1 */
    int64_t a_sum; /* frame A's digest in the sums table */
    int64_t a_row; /* frame A's row in its buffer */
    bool a_par;    /* that buffer is the parity scratch */
    int64_t b_sum; /* the following frame's digest in the sums table */
};

MEC_HD FmBoundary fm_boundary(const FmGeom &g, const FmGran &m, int64_t R) {
    FmBoundary b;
    b.wa = m.r - m.fs;
    b.edge = m.fe - m.r;
    b.a_sum = fm_sum_off(g, m.row, m.item);
    b.a_row = fm_row_off(g, m.row, R, m.fe - m.fs - 32);
    b.a_par = m.row >= g.d;
    const bool wrap = m.item + 1 == g.n;
    /* row + 1 == d + p only for bytes past the buffer's end, which no
     * granule asks for */
    b.b_sum = fm_sum_off(g, wrap ? m.row + 1 : m.row, wrap ? 0 : m.item + 1);
    return b;
}

enum FmWhere { kFmSums = 0, kFmData = 1, kFmParity = 2 };
struct FmByte {
    int where;
    int64_t off;
};

/* rel in [0, hi_b - lo_b).  Bounds: a digest offset is below 32 in both
 * frames (rel - edge <= 14), and a shard offset wa + rel - 32 is below S_A
 * because rel < edge. */
MEC_HD FmByte fm_byte(const FmBoundary &b, int rel) {
    if (rel >= b.edge) return FmByte{kFmSums, b.b_sum + (rel - b.edge)};
    const int64_t w = b.wa + rel;
    if (w < 32) return FmByte{kFmSums, b.a_sum + w};
    return FmByte{b.a_par ? kFmParity : kFmData, b.a_row + (w - 32)};
}

} // namespace mec
#endif
