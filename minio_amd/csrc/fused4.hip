/* One-pass erasure-encode + HighwayHash-256 kernel (v4): every data byte
 * is fetched from HBM exactly once.
 *
 * Semantics of cmd/erasure-coding.go:85 (GF parity) +
 * cmd/bitrot-streaming.go:57-59 (per-shard HH256) in ONE launch.  Three
 * earlier one-launch kernels were measured slower than the kernel pair and
 * are retired; what differs here is how the bytes travel:
 *
 *  - a LOADER wave streams the data rows of the workgroup's G blocks into
 *    an LDS ring with global_load_lds_dwordx4 (no VGPR, no ds_write: the
 *    ds_write_b128 issue cost is what sank the earlier LDS-ring attempts),
 *    one T-byte tile of every row per step, LA tiles ahead;
 *  - NGF GF waves read two 16-B half-columns per row from that ring, run
 *    the bit-sliced transpose / fold / transpose of gf_bs.h (its
 *    4-operation form, bs_transpose4), and write parity twice: to global
 *    memory (nontemporal) and into a small LDS parity ring;
 *  - NHW hash waves (4 lanes per chain, hh_quad.h) hash data rows AND
 *    parity rows out of LDS; data chains and parity chains run the same
 *    code, only the per-lane base and the lag differ.
 *
 * HBM traffic: data 1x read + parity 1x write = 1.5 B per input byte (the
 * kernel pair moves 3.0).
 *
 * Synchronisation is deliberately dumb.  Every wave of the workgroup
 * executes exactly 1 + NS barriers, NS = shard_len/T + NGF, a number that
 * depends on the kernel arguments alone.  Which ring slot a role touches
 * in step s is a pure function of s.  There is no wait loop, no progress
 * counter and no polling anywhere: the kernel cannot deadlock and cannot
 * read a slot early.  Schedule, for tile t (T bytes of every row):
 *
 *    step t-LA            loader issues the tile's DMAs
 *    end of step t-1      loader's counted vmcnt retires them, barrier
 *    step t               data chains hash tile t
 *    steps t .. t+NGF-1   GF wave (t % NGF) computes its parity, a share
 *                         of the rows per step (row_begin)
 *    end of step t+NGF-1  that wave's lgkmcnt(0) lands parity in LDS
 *    step t+NGF           parity chains hash tile t
 *
 * so a data slot is live for LA + NGF steps (DP slots) and a parity slot
 * for 2 (PS slots).  Each wave waits lgkmcnt(0) before every barrier, which
 * retires its LDS reads before a slot can be refilled.
 *
 * LDS image: one DMA instruction writes 1 KiB contiguously (two rows of a
 * tile), so rows lie T = 512 B apart and sixteen chains of a hash wave
 * would hit the same banks.  The image stays linear — it has to — but row
 * r is stored rotated by (r mod 16) packets: the rotation is applied to
 * the loader's per-lane SOURCE address and to every reader's offset.
 *
 * GF lane mapping: lane (g, o), g = lane / 16 the block, o = lane % 16,
 * holds 32 bytes of each row of block g's tile (GF is byte-wise, any 32 will
 * do): bytes [16o, 16o+16) and [T/2 + 16o, T/2 + 16o + 16).  The rotation is
 * a multiple of 32 B, so both pieces stay 16-B aligned and whole.  What the
 * split buys over one 32-B column per lane:
 *  - a global parity store instruction writes 256 contiguous bytes per
 *    block, two whole 128-B lines, and every line is written once (a 32-B
 *    lane stride wrote 16 B and skipped 16: half of every line, twice);
 *  - a ds_read_b128 is served in four groups of 16 lanes over a 256-B bank
 *    row.  Each group holds 8 lanes of block g and 8 of block g+1, whose
 *    rows g*D+k and (g+1)*D+k are rotated by 32k and 32k + 256 ≡ 32k mod
 *    256; their o values together are 0..15, so the group's addresses are
 *    16 distinct 16-B slots of the bank row: conflict-free for g = 0..3,
 *    k = 0..7, both halves (T/2 ≡ 0 mod 256).  The 32-B stride used only
 *    the even slots, 2-way;
 *  - a ds_write_b128 is served in groups of 8 contiguous lanes over a 128-B
 *    bank row; 8 lanes x 16 B are 128 contiguous bytes (they were 256).
 * Requesting all rows of a GF step ahead of the first fold (counted
 * lgkmcnt) was built and measured neutral, so each row is read where it is
 * used.
 *
 * Eligibility: a compiled specialisation, shard_len % T == 0; anything
 * else is hipErrorNotSupported and the caller takes the kernel pair.
 */
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "kernels.h"
#include "ec_matrices_gen.h"
#include "gf_bs.h"
#include "hh_quad.h"

namespace fused4 {

constexpr int T = 512;  /* bytes per row per tile (16 packets) */
constexpr int NHW = 3;  /* hash waves: 48 chains x 4 lanes */
constexpr int PS = 2;   /* parity ring slots */

/* First data row of GF step ph.  A tile's GF work is D row units
 * (transpose + fold) and, in the last step, P output transposes and the
 * stores, about 1.5 row units; the steps share D + 1.5 units evenly.  One
 * wave issues at its own dependent rate whatever else the SIMD does, so
 * the heaviest step paces the whole workgroup. */
constexpr int row_begin(int D, int ngf, int ph) {
    const int b = (ph * (2 * D + 3) + ngf) / (2 * ngf);
    return b < D ? b : D;
}

/* byte offset of byte x of row `row` inside a ring slot (rotated image) */
__device__ __forceinline__ int rot_off(int row, int x) {
    return row * T + ((x + 32 * (row & 15)) & (T - 1));
}

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

/* the one barrier of a step: this wave's LDS reads and writes retired
 * first; raw s_barrier so that DMAs in flight are not drained */
__device__ __forceinline__ void step_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

} // namespace fused4

/* NGF: GF waves, also the steps one tile's GF takes; LA: tiles the loader
 * runs ahead */
template <int D, int P, const uint8_t (&MAT)[P][D], int NGF, int LA>
__global__ void __launch_bounds__((1 + NGF + fused4::NHW) * 64)
fused4_encode_hh_kernel(FusedArgs a) {
    using namespace fused4;
    constexpr int TOT = D + P;
    constexpr int DP = LA + NGF;              /* data ring slots */
    constexpr int GH = NHW * 16 / TOT;        /* chains the hash waves hold */
    constexpr int GC = 64 / (T / 32);         /* columns one GF wave holds */
    constexpr int G = GH < GC ? GH : GC;      /* blocks per workgroup */
    static_assert(G >= 1, "geometry too wide for the hash waves");
    static_assert((G * D) % 2 == 0, "a DMA instruction carries two rows");
    constexpr int NDMA = G * D / 2;           /* DMA instructions per tile */
    static_assert(NDMA * LA <= 63, "vmcnt is a 6-bit counter");
    constexpr int DSLOT = G * D * T;
    constexpr int PSLOT = G * P * T;
    constexpr int PBASE = DP * DSLOT;
    __shared__ __attribute__((aligned(1024))) uint8_t lds[PBASE + PS * PSLOT];

    const int lane = threadIdx.x & 63;
    /* wave-uniform by construction; saying so keeps the role branches and
     * the barriers inside them on the scalar unit */
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t b0 = (int64_t)blockIdx.x * G;
    const int64_t stride = a.row_stride;
    const int64_t ntiles = a.shard_len / T; /* exact (launcher) */
    const int64_t NS = ntiles + NGF;        /* steps; barriers = 1 + NS */

    if (wid == 0) {
        /* ---- loader: DMA i of a tile carries rows 2i (lanes 0-31) and
         * 2i+1 (lanes 32-63), 16 B per lane.  A missing block of a partial
         * group re-reads block b0: its lanes stay in bounds and nothing
         * consumes what they bring. */
        const uint8_t *src[NDMA];
#pragma unroll
        for (int i = 0; i < NDMA; i++) {
            const int row = 2 * i + (lane >> 5);
            int g = row / D;
            const int k = row % D;
            if (b0 + g >= a.n) g = 0;
            const int x = (lane & 31) * 16; /* LDS position inside the row */
            src[i] = a.data + ((b0 + g) * D + k) * stride +
                     ((x - 32 * (row & 15)) & (T - 1));
        }
#define F4_ISSUE(TILE)                                                       \
    {                                                                        \
        const int64_t goff_ = (int64_t)(TILE) * T;                           \
        uint8_t *slot_ = lds + (int)((TILE) % DP) * DSLOT;                   \
        _Pragma("unroll") for (int i = 0; i < NDMA; i++)                     \
            __builtin_amdgcn_global_load_lds(                                \
                (const __attribute__((address_space(1))) uint32_t            \
                     *)(src[i] + goff_),                                     \
                (__attribute__((address_space(3))) uint32_t                  \
                     *)(slot_ + i * 1024),                                   \
                16, 0, 2 /* nt: the stream is read once */);                 \
    }
        /* prologue: tiles 0..LA-1 go out, tile 0 lands */
#pragma unroll
        for (int t = 0; t < LA; t++)
            if (t < ntiles && !(a.probe & 4)) F4_ISSUE(t)
        /* tile 0 landed: at most the later ones still in flight */
        if (ntiles >= LA) wait_vm<NDMA*(LA - 1)>();
        else if (LA > 2 && ntiles == 2) wait_vm<NDMA>();
        else wait_vm<0>();
        step_barrier();
        for (int64_t s = 0; s < NS; s++) {
            /* slot (s+LA) % DP last held tile s-NGF, whose readers retired
             * before the barrier that ended step s-1 */
            if (s + LA < ntiles) {
                if (!(a.probe & 4)) F4_ISSUE(s + LA)
                wait_vm<NDMA*(LA - 1)>(); /* tile s+1 landed */
            } else {
                wait_vm<0>();
            }
            step_barrier();
        }
#undef F4_ISSUE
        return;
    }

    if (wid <= NGF) {
        /* ---- GF wave w owns tiles w, w+NGF, ...; lane = (block g,
         * half-column pair o): bytes [16o, 16o+16) and [T/2 + 16o,
         * T/2 + 16o + 16) of each row of the tile ---- */
        static_assert((T / 2) % (16 * (T / 32)) == 0,
                      "the lanes of a block cover each half of a tile row "
                      "in 16-B pieces");
        const int w = wid - 1;
        const int g = lane / (T / 32);
        const int o = lane % (T / 32);
        const int xlo = o * 16, xhi = T / 2 + o * 16;
        const bool gact = g < G && b0 + g < a.n;
        const int gg = g < G ? g : 0; /* lanes past G mirror block 0 */
        uint8_t *prow = a.parity + ((b0 + gg) * P) * stride + xlo;
        typedef unsigned int v4u __attribute__((ext_vector_type(4)));
        uint32_t accp[P][8];
        step_barrier(); /* prologue */
        int64_t s = 0;
        for (; s < w && s < NS; s++) step_barrier();
        for (int64_t t = w; s < NS; t += NGF) {
            const bool on = t < ntiles && !(a.probe & 2);
            const uint8_t *dslot = lds + (int)(t % DP) * DSLOT;
            uint8_t *pslot = lds + PBASE + (int)(t % PS) * PSLOT;
#pragma unroll
            for (int ph = 0; ph < NGF; ph++) {
                if (s >= NS) break;
                if (on) {
                    if (ph == 0) {
#pragma unroll
                        for (int i = 0; i < P; i++)
#pragma unroll
                            for (int pb = 0; pb < 8; pb++) accp[i][pb] = 0;
                    }
#pragma unroll
                    for (int k = 0; k < D; k++) {
                        if (k >= row_begin(D, NGF, ph) &&
                            k < row_begin(D, NGF, ph + 1)) {
                            uint4 lo = *(const uint4 *)(
                                dslot + rot_off(gg * D + k, xlo));
                            uint4 hi = *(const uint4 *)(
                                dslot + rot_off(gg * D + k, xhi));
                            uint32_t xc[8] = {lo.x, lo.y, lo.z, lo.w,
                                              hi.x, hi.y, hi.z, hi.w};
                            bs_transpose4(xc);
                            bs_acc_k<D, P, MAT>(k, xc, accp);
                        }
                    }
                    if (ph == NGF - 1) {
#pragma unroll
                        for (int i = 0; i < P; i++) {
                            bs_transpose4(accp[i]);
                            v4u vlo = {accp[i][0], accp[i][1], accp[i][2],
                                       accp[i][3]};
                            v4u vhi = {accp[i][4], accp[i][5], accp[i][6],
                                       accp[i][7]};
                            if (!(a.probe & 16)) {
                                *(v4u *)(pslot + rot_off(gg * P + i, xlo)) =
                                    vlo;
                                *(v4u *)(pslot + rot_off(gg * P + i, xhi)) =
                                    vhi;
                            }
                            if (gact && !(a.probe & 8)) {
                                uint8_t *orow = prow + i * stride + t * T;
                                __builtin_nontemporal_store(vlo, (v4u *)orow);
                                __builtin_nontemporal_store(
                                    vhi, (v4u *)(orow + T / 2));
                            }
                        }
                    }
                }
                step_barrier();
                s++;
            }
        }
        return;
    }

    /* ---- hash waves: 4 lanes per chain; init and finish are hh_quad.h's,
     * the packet loop is paced by the step barriers.  Data chains hash
     * tile s in step s, parity chains tile s-NGF. ---- */
    const int ln = (wid - 1 - NGF) * 64 + lane;
    const int cp = ln >> 2; /* chain index in the workgroup */
    const int j = ln & 3;   /* HighwayHash lane */
    const int cg = cp / TOT;
    const int cs = cp % TOT;
    const bool act = cp < G * TOT && b0 + cg < a.n;
    const bool isp = cs >= D;
    const int row = isp ? cg * P + (cs - D) : cg * D + cs;
    const int lag = isp ? NGF : 0;
    const int rr = 32 * (row & 15) + 8 * j;
    const int rbase = (isp ? PBASE : 0) + row * T;
    const uint32_t S3 = hh1_sel(j);

    __builtin_amdgcn_s_setprio(1);

    HH1 st;
    hh1_init(st, a.key, j);

    step_barrier(); /* prologue */
    for (int64_t s = 0; s < NS; s++) {
        const int64_t u = s - lag;
        if (act && u >= 0 && u < ntiles && !(a.probe & 1)) {
            const int slot = isp ? (int)(u % PS) * PSLOT : (int)(u % DP) * DSLOT;
            const uint8_t *base = lds + rbase + slot;
            uint64_t q[T / 32];
#pragma unroll
            for (int pk = 0; pk < T / 32; pk++)
                q[pk] = *(const uint64_t *)(base + ((32 * pk + rr) & (T - 1)));
#pragma unroll
            for (int pk = 0; pk < T / 32; pk++) hh1_update(st, q[pk], S3);
        }
        step_barrier();
    }
    __builtin_amdgcn_s_setprio(0);

    /* finalise + store sums */
    if (act)
        *(uint64_t *)(a.sums + ((b0 + cg) * TOT + cs) * 32 + 8 * j) =
            hh1_finish(st, j, S3);
}

/* MEC_FUSED4, if set, decides.  Otherwise fused4 is off exactly when
 * MEC_PIPE is in the environment (whatever its value): that knob asks for
 * the kernel pair, whose cross-batch pipelining it switches. */
static bool fused4_env_enabled() {
    if (const char *v = getenv("MEC_FUSED4")) return atoi(v) != 0;
    return getenv("MEC_PIPE") == nullptr;
}

static std::atomic<uint64_t> g_fused4_launches{0};

extern "C" uint64_t mec_fused4_launches(void) {
    return g_fused4_launches.load(std::memory_order_relaxed);
}

extern "C" hipError_t mec_launch_fused4_encode_hh(int d, int p,
                                                  const FusedArgs *args,
                                                  hipStream_t stream) {
    static const bool enabled = fused4_env_enabled();
    if (!enabled) return hipErrorNotSupported;
    /* MEC_F4_LA: loader lookahead in tiles (2 or 3).  MEC_F4_PROBE: perf
     * isolation, results INVALID: bit 0 hash waves idle, bit 1 GF waves
     * idle, bit 2 loader issues nothing, bit 3 GF waves skip the global
     * parity stores (the LDS parity writes still run), bit 4 GF waves skip
     * the LDS parity writes (the parity chains hash stale bytes).  Every
     * wave still executes every barrier under any combination of bits. */
    static const int f4la = [] {
        const char *v = getenv("MEC_F4_LA");
        return v ? atoi(v) : 2;
    }();
    static const int f4ngf = [] {
        const char *v = getenv("MEC_F4_NGF");
        return v ? atoi(v) : 4;
    }();
    static const int f4probe = [] {
        const char *v = getenv("MEC_F4_PROBE");
        return v ? atoi(v) : 0;
    }();
    if (args->shard_len <= 0 || args->shard_len % fused4::T != 0)
        return hipErrorNotSupported;
    if (d == 8 && p == 4) {
        constexpr int G = 4;
        FusedArgs aa = *args;
        aa.probe = f4probe;
        dim3 grid((uint32_t)((aa.n + G - 1) / G));
#define F4_GO(NGF_, LA_)                                                     \
    hipLaunchKernelGGL(                                                      \
        (fused4_encode_hh_kernel<8, 4, MAT_8_4, NGF_, LA_>), grid,           \
        dim3((1 + NGF_ + fused4::NHW) * 64), 0, stream, aa)
        if (f4ngf == 6) {
            if (f4la == 3) F4_GO(6, 3); else F4_GO(6, 2);
        } else if (f4ngf == 5) {
            if (f4la == 3) F4_GO(5, 3); else F4_GO(5, 2);
        } else {
            if (f4la == 3) F4_GO(4, 3); else F4_GO(4, 2);
        }
#undef F4_GO
        g_fused4_launches.fetch_add(1, std::memory_order_relaxed);
        return hipGetLastError();
    }
    return hipErrorNotSupported;
}
