/* C-ABI implementation for the MI355X erasure+bitrot hot path.
 * Public surface: include/minio_ec.h (see the header for the Go-interface
 * mapping this library drops in behind).  Host driver logic mirrors the
 * reference's Go drivers:
 *   - Erasure.Encode loop          cmd/erasure-encode.go:76-108
 *   - streamingBitrotWriter        cmd/bitrot-streaming.go:44-75
 *   - streamingBitrotReader.ReadAt cmd/bitrot-streaming.go:161-200
 *   - Erasure.Decode / Heal        cmd/erasure-decode.go:239-364
 *   - writeDataBlocks              cmd/erasure-utils.go:42-105
 *   - bitrotVerify                 cmd/bitrot.go:164-216
 * All GF arithmetic and hashing runs in the HIP kernels (kernels.hip);
 * there is no CPU compute fallback — a missing GPU fails loudly
 * (MEC_ERR_NO_GPU / MEC_ERR_HIP).
 */
#include "../../include/minio_ec.h"
#include "frames_plan.h"
#include "gf_host.h"
#include "kernels.h"
#include "read_var_plan.h"
#include "recon_plan.h"
#include "scrub_plan.h"
#include "var_plan.h"
#include "verify_list.h"

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace {

thread_local std::string g_last_error;

void set_err(const char *what, hipError_t e) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
}

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) {                                              \
            set_err(#expr, _e);                                              \
            return MEC_ERR_HIP;                                              \
        }                                                                    \
    } while (0)

int64_t ceil_frac(int64_t num, int64_t den) {
    /* cmd/utils.go:689 (positive operands on this path) */
    if (den == 0) return 0;
    return (num + den - 1) / den;
}

/* magic HighwayHash key, cmd/bitrot.go:37, as 4 little-endian u64 words */
const uint8_t kMagicHHKey[32] = {
    0x4b, 0xe7, 0x34, 0xfa, 0x8e, 0x23, 0x8a, 0xcd, 0x26, 0x3e, 0x83,
    0xe6, 0xbb, 0x96, 0x85, 0x52, 0x04, 0x0f, 0x93, 0x5d, 0xa3, 0x9f,
    0x44, 0x14, 0x97, 0xe0, 0x9d, 0x13, 0x22, 0xde, 0x36, 0xa0};

int hash_size(int algo) {
    switch (algo) {
    case MEC_BITROT_SHA256:
    case MEC_BITROT_HIGHWAYHASH256:
    case MEC_BITROT_HIGHWAYHASH256S:
        return 32;
    case MEC_BITROT_BLAKE2B512:
        return 64;
    default:
        return 0;
    }
}

using mec::bs_pack_matrix; /* recon_plan.cpp */

static_assert(mec::kPlanMaxD == MEC_KMAX_D && mec::kPlanMaxE == MEC_KMAX_E &&
                  mec::kPlanMaxTotal == MEC_KMAX_TOTAL,
              "recon_plan.h caps must mirror kernels.h");

} // namespace

struct mec_ctx {
    int device = 0;
    int d = 0, p = 0;
    int64_t block_size = 0;
    int64_t S = 0;      /* shard size  = ceil(block_size / d) */
    int64_t stride = 0; /* device row stride = align64(S) */
    std::vector<uint8_t> enc_matrix; /* (d+p) x d */
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; /* hash(data) overlap lane */
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    hipEvent_t ev_gf = nullptr, ev_h = nullptr;
    hipEvent_t ev_pipe[2] = {nullptr, nullptr}; /* hash-done per buffer slot */
    int pipe_idx = 0;
    /* Which batches the one-pass fused4 kernel takes (f4_takes).  Read
     * per context at mec_ctx_create, never latched: f4_min_n is MEC_F4_MIN,
     * -1 when unset; f4_cus the device's compute-unit count. */
    int f4_min_n = -1;
    int f4_cus = 0;
    std::mutex mu;

    /* grow-only scratch (device + pinned host) for host-pointer calls */
    void *dev_a = nullptr, *dev_b = nullptr, *dev_c = nullptr;
    void *dev_d = nullptr; /* stream-assembly output */
    void *dev_m = nullptr;  /* bit-matrix masks for the BS matmul (r2) */
    std::vector<uint32_t> m_cached; /* host copy of what dev_m holds — the
        chunked reconstruct path re-sends identical masks per chunk, and
        re-uploading would need a stream sync that serializes the
        overlapped ingest */
    size_t cap_a = 0, cap_b = 0, cap_c = 0, cap_d = 0, cap_m = 0;
    void *pin = nullptr;
    size_t cap_pin = 0;

    /* mixed-pattern reconstruct: the plan table + work lists of one call
     * live in dev_x; they get there by a stream-ordered copy from one of
     * two pinned staging slots, so back-to-back async calls never drain
     * the stream.  ev_x[s] marks slot s's copy done (the slot may then be
     * refilled); dev_x itself is only rewritten behind the kernels that
     * read it, by stream order. */
    void *dev_x = nullptr;
    size_t cap_x = 0;
    void *pin_x[2] = {nullptr, nullptr};
    size_t cap_pin_x[2] = {0, 0};
    hipEvent_t ev_x[2] = {nullptr, nullptr};
    int x_idx = 0;
    mec::ReconPlan plan; /* reused across calls to keep its allocations */

    /* verified batch read: dev_v holds [chain-id list | ok bytes], pin_v
     * stages the list up and the ok bytes down.  The call is synchronous,
     * so one pinned buffer is enough.  Grow-only, sized by n*(d+p). */
    void *dev_v = nullptr, *pin_v = nullptr;
    size_t cap_v = 0, cap_pin_v = 0;
    std::vector<uint32_t> vlist;   /* verify list, then the rehash list */
    std::vector<uint8_t> vpresent; /* read_mask & ok */

    /* per-item-length encode: the tables of one call (items, column
     * prefix, hash order) live in dev_e and get there as the mixed
     * reconstruct's plan does: a stream-ordered copy from one of two pinned
     * slots, ev_e[s] marking slot s's copy done. */
    void *dev_e = nullptr;
    size_t cap_e = 0;
    void *pin_e[2] = {nullptr, nullptr};
    size_t cap_pin_e[2] = {0, 0};
    hipEvent_t ev_e[2] = {nullptr, nullptr};
    int e_idx = 0;
    mec::VarPlan vplan; /* reused across calls to keep its allocations */
    /* encode into frames: the F prefix rides in dev_e behind the encode's
     * tables; dev_f holds the call's parity rows and, behind them, its sums
     * table.  Grow-only, rewritten only behind the kernels that read it, by
     * stream order. */
    mec::FramesPlan fplan;
    void *dev_f = nullptr;
    size_t cap_f = 0;
    /* per-item-length verified read: tile prefixes of the call's work
     * lists, and the host offsets of the packed rows (host-pointer call) */
    std::vector<int64_t> vtiles[MEC_KMAX_E + 1];
    std::vector<int64_t> vhost_off;

    /* batch scrub: the plan of one call; its tables and ok bytes go through
     * dev_v / pin_v, the host-pointer variant's files through dev_a / pin */
    mec::ScrubPlan splan;
    std::vector<int64_t> shost_off;
    std::vector<uint8_t> scorrupt;

    mec_status ensure(void **buf, size_t *cap, size_t need) {
        if (*cap >= need) return MEC_OK;
        if (*buf) (void)hipFree(*buf);
        *buf = nullptr;
        *cap = 0;
        HIP_TRY(hipMalloc(buf, need));
        *cap = need;
        return MEC_OK;
    }
    mec_status ensure_pin(size_t need) {
        if (cap_pin >= need) return MEC_OK;
        if (pin) (void)hipHostFree(pin);
        pin = nullptr;
        cap_pin = 0;
        HIP_TRY(hipHostMalloc(&pin, need));
        cap_pin = need;
        return MEC_OK;
    }
};

extern "C" {

int mec_version(void) { return 10000; /* 1.0.0 */ }

const char *mec_last_error(void) { return g_last_error.c_str(); }

int mec_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* ---- shard-size math (exact mirrors) ---------------------------------- */

int64_t mec_shard_size(int64_t block_size, int d) {
    /* cmd/erasure-coding.go:116-118 */
    return ceil_frac(block_size, d);
}

int64_t mec_shard_file_size(int64_t block_size, int d, int64_t total_length) {
    /* cmd/erasure-coding.go:121-132 */
    if (total_length == 0) return 0;
    if (total_length == -1) return -1;
    int64_t num = total_length / block_size;
    int64_t last = total_length % block_size;
    int64_t last_shard = ceil_frac(last, d);
    return num * mec_shard_size(block_size, d) + last_shard;
}

int64_t mec_shard_file_offset(int64_t block_size, int d, int64_t start_offset,
                              int64_t length, int64_t total_length) {
    /* cmd/erasure-coding.go:135-141 */
    int64_t shard_size = mec_shard_size(block_size, d);
    int64_t shard_file_size = mec_shard_file_size(block_size, d, total_length);
    int64_t end_shard = (start_offset + length) / block_size;
    int64_t till = end_shard * shard_size + shard_size;
    if (till > shard_file_size) till = shard_file_size;
    return till;
}

int64_t mec_bitrot_shard_file_size(int64_t size, int64_t shard_size,
                                   int algo) {
    /* cmd/bitrot.go:156-161 */
    if (algo != MEC_BITROT_HIGHWAYHASH256S) return size;
    return ceil_frac(size, shard_size) * hash_size(algo) + size;
}

int64_t mec_shard_stride(int64_t block_size, int d) {
    return (mec_shard_size(block_size, d) + 63) & ~int64_t(63);
}

/* ---- context ----------------------------------------------------------- */

mec_status mec_ctx_create(int d, int p, int64_t block_size, int device,
                          mec_ctx **out) {
    /* sanity mirrors NewErasure, cmd/erasure-coding.go:43-50 */
    if (d <= 0 || p < 0) return MEC_ERR_INV_SHARD_NUM;
    if (d + p > 256) return MEC_ERR_MAX_SHARD_NUM;
    if (d > MEC_KMAX_D || d + p > MEC_KMAX_TOTAL) return MEC_ERR_MAX_SHARD_NUM;
    if (block_size <= 0) return MEC_ERR_INVALID_ARG;
    int ndev = mec_device_count();
    if (ndev == 0) {
        g_last_error = "no HIP device visible (MI355X required; this library "
                       "has no CPU fallback)";
        return MEC_ERR_NO_GPU;
    }
    if (device < 0 || device >= ndev) return MEC_ERR_INVALID_ARG;

    auto ctx = new mec_ctx();
    ctx->device = device;
    ctx->d = d;
    ctx->p = p;
    ctx->block_size = block_size;
    ctx->S = mec_shard_size(block_size, d);
    ctx->stride = mec_shard_stride(block_size, d);
    ctx->enc_matrix.resize((size_t)(d + p) * d);
    if (!mec::build_encode_matrix(d, p, ctx->enc_matrix.data())) {
        delete ctx;
        return MEC_ERR_INVALID_ARG;
    }
    if (const char *s = getenv("MEC_F4_MIN")) ctx->f4_min_n = atoi(s);
    (void)hipDeviceGetAttribute(&ctx->f4_cus,
                                hipDeviceAttributeMultiprocessorCount, device);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreate(&ctx->stream);
    if (e == hipSuccess) e = hipStreamCreate(&ctx->stream2);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev_start);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev_stop);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_gf, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_h, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_pipe[0], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_pipe[1], hipEventDisableTiming);
    if (e != hipSuccess) {
        set_err("ctx_create", e);
        delete ctx;
        return MEC_ERR_HIP;
    }
    *out = ctx;
    return MEC_OK;
}

int mec_ctx_d(mec_ctx *ctx) { return ctx->d; }
int mec_ctx_p(mec_ctx *ctx) { return ctx->p; }
int64_t mec_ctx_block_size(mec_ctx *ctx) { return ctx->block_size; }

void mec_ctx_destroy(mec_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->dev_a) (void)hipFree(ctx->dev_a);
    if (ctx->dev_b) (void)hipFree(ctx->dev_b);
    if (ctx->dev_c) (void)hipFree(ctx->dev_c);
    if (ctx->dev_d) (void)hipFree(ctx->dev_d);
    if (ctx->dev_m) (void)hipFree(ctx->dev_m);
    if (ctx->dev_x) (void)hipFree(ctx->dev_x);
    if (ctx->dev_v) (void)hipFree(ctx->dev_v);
    if (ctx->pin_v) (void)hipHostFree(ctx->pin_v);
    if (ctx->dev_e) (void)hipFree(ctx->dev_e);
    if (ctx->dev_f) (void)hipFree(ctx->dev_f);
    for (int s = 0; s < 2; s++) {
        if (ctx->pin_e[s]) (void)hipHostFree(ctx->pin_e[s]);
        if (ctx->ev_e[s]) (void)hipEventDestroy(ctx->ev_e[s]);
    }
    for (int s = 0; s < 2; s++) {
        if (ctx->pin_x[s]) (void)hipHostFree(ctx->pin_x[s]);
        if (ctx->ev_x[s]) (void)hipEventDestroy(ctx->ev_x[s]);
    }
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
    if (ctx->ev_stop) (void)hipEventDestroy(ctx->ev_stop);
    if (ctx->ev_gf) (void)hipEventDestroy(ctx->ev_gf);
    if (ctx->ev_h) (void)hipEventDestroy(ctx->ev_h);
    if (ctx->ev_pipe[0]) (void)hipEventDestroy(ctx->ev_pipe[0]);
    if (ctx->ev_pipe[1]) (void)hipEventDestroy(ctx->ev_pipe[1]);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

/* ---- batch encode ------------------------------------------------------ */

/* fused4 runs one workgroup of 4 blocks per compute unit, so a launch
 * costs whole rounds of f4_cus workgroups, while the kernel pair scales
 * with n: fused4 wins when its rounds are at least 3/4 full.  Measured at
 * EC8+4/1 MiB on 256 CUs: it wins at n = 768, 896,
 * 1024 and 2048 (fill 0.75 to 1) and loses at 1280 (0.625).  With
 * MEC_F4_MIN set, n >= MEC_F4_MIN decides alone. */
static bool f4_takes(const mec_ctx *ctx, int n) {
    if (ctx->f4_min_n >= 0) return n >= ctx->f4_min_n;
    if (ctx->f4_cus <= 0) return false;
    const int64_t wgs = ((int64_t)n + 3) / 4;
    const int64_t rounds = (wgs + ctx->f4_cus - 1) / ctx->f4_cus;
    return wgs * 4 >= rounds * ctx->f4_cus * 3;
}

/* What became of a batch offered to the one-pass kernel. */
enum class F4 { Launched, NotTaken, Error };

/* One-pass encode + HighwayHash (fused4.hip; 1.5 B of HBM traffic per
 * input byte vs 3.0 for the kernel pair) on ctx->stream, for the batches
 * f4_takes gives it.  NotTaken: nothing was launched and the caller runs
 * the kernel pair.  Error: set_err has been called. */
static F4 try_fused4(mec_ctx *ctx, int n, const void *data_dev,
                     int64_t shard_len, void *parity_dev, int algo,
                     void *sums_dev) {
    if (algo != MEC_BITROT_HIGHWAYHASH256 &&
        algo != MEC_BITROT_HIGHWAYHASH256S)
        return F4::NotTaken;
    if (!f4_takes(ctx, n)) return F4::NotTaken;
    FusedArgs fa{};
    fa.data = (const uint8_t *)data_dev;
    fa.parity = (uint8_t *)parity_dev;
    fa.sums = (uint8_t *)sums_dev;
    fa.row_stride = ctx->stride;
    fa.shard_len = shard_len;
    fa.n = n;
    memcpy(fa.key, kMagicHHKey, 32);
    hipError_t he =
        mec_launch_fused4_encode_hh(ctx->d, ctx->p, &fa, ctx->stream);
    if (he == hipSuccess) return F4::Launched;
    if (he == hipErrorNotSupported) return F4::NotTaken;
    set_err("fused4_encode_hh", he);
    return F4::Error;
}

/* Bitrot sums of every data and parity row of an encoded batch, one launch
 * on `stream`. */
static mec_status hash_all_rows(mec_ctx *ctx, int n, const void *data_dev,
                                int64_t shard_len, const void *parity_dev,
                                int algo, void *sums_dev,
                                hipStream_t stream) {
    HashArgs h{};
    h.data = (const uint8_t *)data_dev;
    h.parity = (const uint8_t *)parity_dev;
    h.sums = (uint8_t *)sums_dev;
    h.row_stride = ctx->stride;
    h.msg_len = shard_len;
    h.d = ctx->d;
    h.p = ctx->p;
    h.mode = MEC_HASH_ALL;
    h.n_chains = (int64_t)n * (ctx->d + ctx->p);
    memcpy(h.key, kMagicHHKey, 32);
    HIP_TRY(mec_launch_hash(algo, &h, stream));
    return MEC_OK;
}

/* Pack the e x d coefficients of mat (rows MEC_KMAX_D apart, as in
 * GfMatmulArgs::mat) into 8x8 bit matrices, make dev_m hold them and
 * return it in *masks_dev.  A few hundred bytes, uploaded synchronously,
 * and only when they differ from what dev_m already holds (m_cached). */
static mec_status bs_masks_dev(mec_ctx *ctx, const uint8_t *mat, int e, int d,
                               const uint32_t **masks_dev) {
    uint32_t masks[MEC_KMAX_E * MEC_KMAX_D * 2];
    for (int i = 0; i < e; i++)
        for (int k = 0; k < d; k++)
            bs_pack_matrix(mat[i * MEC_KMAX_D + k],
                           &masks[((size_t)i * d + k) * 2]);
    size_t mw = (size_t)e * d * 2;
    size_t mb = mw * sizeof(uint32_t);
    if (ctx->m_cached.size() != mw ||
        memcmp(ctx->m_cached.data(), masks, mb) != 0) {
        mec_status st;
        if ((st = ctx->ensure(&ctx->dev_m, &ctx->cap_m, mb)) != MEC_OK)
            return st;
        /* prior launches may still read dev_m */
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpy(ctx->dev_m, masks, mb, hipMemcpyHostToDevice));
        ctx->m_cached.assign(masks, masks + mw);
    }
    *masks_dev = (const uint32_t *)ctx->dev_m;
    return MEC_OK;
}

/* Encode for a geometry without a compiled specialization: GF parity rows
 * by the runtime-matrix kernel, in groups of <= MEC_KMAX_E. */
static mec_status encode_generic(mec_ctx *ctx, int n, const void *data_dev,
                                 int64_t shard_len, void *parity_dev) {
    const int d = ctx->d, p = ctx->p;
    for (int i0 = 0; i0 < p; i0 += MEC_KMAX_E) {
        int e = p - i0 > MEC_KMAX_E ? MEC_KMAX_E : p - i0;
        GfMatmulArgs a{};
        a.src = (const uint8_t *)data_dev;
        a.dst = (uint8_t *)parity_dev;
        a.src_item_stride = (int64_t)d * ctx->stride;
        a.dst_item_stride = (int64_t)p * ctx->stride;
        a.row_stride = ctx->stride;
        a.shard_len = shard_len;
        a.d = d;
        for (int k = 0; k < d; k++) a.src_rows[k] = (uint8_t)k;
        for (int i = 0; i < e; i++) a.dst_rows[i] = (uint8_t)(i0 + i);
        for (int i = 0; i < e; i++)
            for (int k = 0; k < d; k++)
                a.mat[i * MEC_KMAX_D + k] =
                    ctx->enc_matrix[(size_t)(d + i0 + i) * d + k];
        mec_status st = bs_masks_dev(ctx, a.mat, e, d, &a.bs_masks);
        if (st != MEC_OK) return st;
        HIP_TRY(mec_launch_gf_matmul(&a, e, n, ctx->stream));
    }
    return MEC_OK;
}

static mec_status encode_dev_locked(mec_ctx *ctx, int n, const void *data_dev,
                                    int64_t block_len, void *parity_dev,
                                    int algo, void *sums_dev) {
    if (n <= 0 || block_len <= 0 || block_len > ctx->block_size)
        return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));

    const int d = ctx->d, p = ctx->p;
    /* per-call shard size mirrors Split: ceil(block_len/d)
     * (cmd/erasure-coding.go:81 + :117); rows stay at ctx->stride */
    const int64_t S_call = ceil_frac(block_len, d);
    if (sums_dev != nullptr) {
        switch (try_fused4(ctx, n, data_dev, S_call, parity_dev, algo,
                           sums_dev)) {
        case F4::Launched: return MEC_OK;
        case F4::Error: return MEC_ERR_HIP;
        case F4::NotTaken: break;
        }
    }
    /* specialized straight-line kernel for common geometries */
    GfEncArgs ea{};
    ea.data = (const uint8_t *)data_dev;
    ea.parity = (uint8_t *)parity_dev;
    ea.row_stride = ctx->stride;
    ea.shard_len = S_call;
    const hipError_t he_spec =
        mec_launch_gf_encode_spec(d, p, &ea, n, ctx->stream);
    if (he_spec != hipSuccess && he_spec != hipErrorNotSupported) {
        set_err("gf_encode_spec", he_spec);
        return MEC_ERR_HIP;
    }
    if (he_spec == hipErrorNotSupported) {
        mec_status st = encode_generic(ctx, n, data_dev, S_call, parity_dev);
        if (st != MEC_OK) return st;
    }
    if (sums_dev != nullptr) {
        if (!hash_size(algo)) return MEC_ERR_INVALID_ARG;
        /* single launch with every chain in flight: the hash is
         * latency-bound per chain, so splitting it (or overlapping it with
         * the GF kernel's 8-waves/SIMD occupancy) measurably regresses —
         * measured: overlapped split 2.04 ms/step vs sequential
         * single-launch 1.12 ms/step at EC8+4/1MiB/1024. */
        return hash_all_rows(ctx, n, data_dev, S_call, parity_dev, algo,
                             sums_dev, ctx->stream);
    }
    return MEC_OK;
}

/* Pipelined encode: batch t's hash (on the context's second stream)
 * overlaps batch t+1's GF.  CONTRACT: the caller alternates between TWO
 * parity/sums buffer sets in strict round-robin and calls mec_pipe_sync
 * before reading any results.  Results are identical to
 * mec_encode_batch_dev per call; only cross-call scheduling differs
 * (independent batches — MinIO objects — pipeline the same way). */
mec_status mec_encode_batch_dev_pipe(mec_ctx *ctx, int n,
                                     const void *data_dev, int64_t block_len,
                                     void *parity_dev, int algo,
                                     void *sums_dev) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (n <= 0 || block_len <= 0 || block_len > ctx->block_size ||
        sums_dev == nullptr || !hash_size(algo))
        return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const int d = ctx->d, p = ctx->p;
    const int64_t S_call = ceil_frac(block_len, d);
    const int idx = ctx->pipe_idx & 1;
    ctx->pipe_idx ^= 1;
    /* this buffer slot's previous hash must be drained before GF rewrites
     * the parity buffer */
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_pipe[idx], 0));
    /* one-pass kernel: one launch does GF + hash at 1.5 B/input byte —
     * cross-batch pipelining degenerates to back-to-back fused launches,
     * which is what we want (the fused kernel is memory-bound; overlapping
     * two of them cannot beat sequential) */
    switch (try_fused4(ctx, n, data_dev, S_call, parity_dev, algo, sums_dev)) {
    case F4::Launched:
        HIP_TRY(hipEventRecord(ctx->ev_pipe[idx], ctx->stream));
        return MEC_OK;
    case F4::Error: return MEC_ERR_HIP;
    case F4::NotTaken: break;
    }
    {
        GfEncArgs ea{};
        ea.data = (const uint8_t *)data_dev;
        ea.parity = (uint8_t *)parity_dev;
        ea.row_stride = ctx->stride;
        ea.shard_len = S_call;
        hipError_t he = mec_launch_gf_encode_spec(d, p, &ea, n, ctx->stream);
        if (he == hipErrorNotSupported)
            return MEC_ERR_INVALID_ARG; /* pipe mode needs a specialization */
        if (he != hipSuccess) {
            set_err("gf_encode_spec", he);
            return MEC_ERR_HIP;
        }
    }
    HIP_TRY(hipEventRecord(ctx->ev_gf, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->ev_gf, 0));
    mec_status st = hash_all_rows(ctx, n, data_dev, S_call, parity_dev, algo,
                                  sums_dev, ctx->stream2);
    if (st != MEC_OK) return st;
    HIP_TRY(hipEventRecord(ctx->ev_pipe[idx], ctx->stream2));
    return MEC_OK;
}

mec_status mec_pipe_sync(mec_ctx *ctx) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream2));
    return MEC_OK;
}

mec_status mec_encode_batch_dev_async(mec_ctx *ctx, int n,
                                      const void *data_dev, int64_t block_len,
                                      void *parity_dev, int algo,
                                      void *sums_dev) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return encode_dev_locked(ctx, n, data_dev, block_len, parity_dev, algo,
                             sums_dev);
}

mec_status mec_encode_batch_dev(mec_ctx *ctx, int n, const void *data_dev,
                                int64_t block_len, void *parity_dev, int algo,
                                void *sums_dev) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status s = encode_dev_locked(ctx, n, data_dev, block_len, parity_dev,
                                     algo, sums_dev);
    if (s != MEC_OK) return s;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_encode_batch(mec_ctx *ctx, int n, const uint8_t *data,
                            int64_t block_len, uint8_t *parity, int algo,
                            uint8_t *sums) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (n <= 0 || block_len <= 0 || block_len > ctx->block_size)
        return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const int d = ctx->d, p = ctx->p;
    const int real_hsz = sums ? hash_size(algo) : 0;
    const int64_t S = ceil_frac(block_len, d), stride = ctx->stride;
    size_t data_bytes = (size_t)n * d * stride;
    size_t par_bytes = (size_t)n * p * stride;
    size_t sum_bytes = (size_t)n * (d + p) * (size_t)real_hsz;
    mec_status st;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, data_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure(&ctx->dev_b, &ctx->cap_b, par_bytes)) != MEC_OK)
        return st;
    if (sums &&
        (st = ctx->ensure(&ctx->dev_c, &ctx->cap_c, sum_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(data_bytes > par_bytes + sum_bytes
                                  ? data_bytes
                                  : par_bytes + sum_bytes)) != MEC_OK)
        return st;

    /* scatter packed object bytes into the padded strided shard layout
     * (Split semantics, cmd/erasure-coding.go:81: shard k gets bytes
     * [k*S, (k+1)*S) of the block, zero-padded) */
    uint8_t *pinb = (uint8_t *)ctx->pin;
    for (int b = 0; b < n; b++) {
        const uint8_t *blk = data + (size_t)b * block_len;
        for (int k = 0; k < d; k++) {
            uint8_t *dst = pinb + ((size_t)b * d + k) * stride;
            int64_t have = block_len - (int64_t)k * S;
            if (have < 0) have = 0;
            if (have > S) have = S;
            if (have) memcpy(dst, blk + (int64_t)k * S, (size_t)have);
            if (have < S) memset(dst + have, 0, (size_t)(S - have));
        }
    }
    HIP_TRY(hipMemcpyAsync(ctx->dev_a, pinb, data_bytes, hipMemcpyHostToDevice,
                           ctx->stream));
    st = encode_dev_locked(ctx, n, ctx->dev_a, block_len, ctx->dev_b, algo,
                           sums ? ctx->dev_c : nullptr);
    if (st != MEC_OK) return st;
    HIP_TRY(hipMemcpyAsync(pinb, ctx->dev_b, par_bytes, hipMemcpyDeviceToHost,
                           ctx->stream));
    if (sums)
        HIP_TRY(hipMemcpyAsync(pinb + par_bytes, ctx->dev_c, sum_bytes,
                               hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    /* gather parity (packed, no stride padding) */
    for (int b = 0; b < n; b++)
        for (int i = 0; i < p; i++)
            memcpy(parity + ((size_t)b * p + i) * S,
                   pinb + ((size_t)b * p + i) * stride, (size_t)S);
    if (sums) memcpy(sums, pinb + par_bytes, sum_bytes);
    return MEC_OK;
}

/* ---- batch encode, one block length PER ITEM ---------------------------- */

mec_status mec_var_row_offsets(int d, int64_t block_size, int n,
                               const int64_t *block_lens, int64_t *row_off) {
    /* p is not known here: the 32-bit chain-id guard is applied to n*d;
     * the encode calls apply it to n*(d+p) */
    mec::VarPlan pl;
    if (!row_off ||
        !mec::build_var_plan(d, d, block_size, n, block_lens, &pl))
        return MEC_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) row_off[i] = pl.items[(size_t)i].row_off;
    row_off[n] = pl.rows_total;
    return MEC_OK;
}

/* MEC_ERR_INVALID_ARG, with the message, for a geometry that has no compiled
 * gf_encode_bs_var_kernel */
static mec_status var_geometry_check(const mec_ctx *ctx) {
    if (mec_encode_var_supported(ctx->d, ctx->p)) return MEC_OK;
    g_last_error = "per-item-length encode needs a compiled (d,p) "
                   "specialization; EC" + std::to_string(ctx->d) + "+" +
                   std::to_string(ctx->p) + " has none";
    return MEC_ERR_INVALID_ARG;
}

/* Everything that can be refused is refused here, before anything is
 * launched or written; on MEC_OK ctx->vplan holds the call's plan. */
static mec_status var_check_locked(mec_ctx *ctx, int n, const void *data,
                                   const int64_t *block_lens,
                                   const void *parity, int algo,
                                   const void *sums) {
    if (n <= 0 || !data || !block_lens || !parity) return MEC_ERR_INVALID_ARG;
    /* only HighwayHash has a per-item-length kernel; both ids name the
     * same keyed function */
    if (sums && algo != MEC_BITROT_HIGHWAYHASH256S &&
        algo != MEC_BITROT_HIGHWAYHASH256)
        return MEC_ERR_INVALID_ARG;
    if (var_geometry_check(ctx) != MEC_OK) return MEC_ERR_INVALID_ARG;
    if (!mec::build_var_plan(ctx->d, ctx->d + ctx->p, ctx->block_size, n,
                             block_lens, &ctx->vplan))
        return MEC_ERR_INVALID_ARG;
    return MEC_OK;
}

/* Split scatter (cmd/erasure-coding.go:81) of each block of the
 * concatenated `data` into its own rows of the packed layout at pinb: shard
 * k gets bytes [k*S_i, (k+1)*S_i), zero-padded to S_i. */
static void var_scatter_host(const mec::VarPlan &pl, int d,
                             const uint8_t *data, const int64_t *block_lens,
                             uint8_t *pinb) {
    const uint8_t *blk = data;
    const size_t n = pl.items.size();
    for (size_t b = 0; b < n; b++) {
        const int64_t S = pl.items[b].shard_len;
        const int64_t stride = (S + 63) & ~int64_t(63);
        uint8_t *rows = pinb + (size_t)d * pl.items[b].row_off;
        for (int k = 0; k < d; k++) {
            uint8_t *dst = rows + (size_t)k * stride;
            int64_t have = block_lens[b] - (int64_t)k * S;
            if (have < 0) have = 0;
            if (have > S) have = S;
            if (have) memcpy(dst, blk + (int64_t)k * S, (size_t)have);
            if (have < S) memset(dst + have, 0, (size_t)(S - have));
        }
        blk += block_lens[b];
    }
}

/* Uploads ctx->vplan's tables and launches the two kernels.  Never
 * synchronizes the stream; the only host wait is on the copy that last
 * read the pinned slot being refilled (two calls back). */
/* extra, when given, is one more table of the call (the frames path's F
 * prefix): it rides in the same upload, and *extra_dev is where it lands. */
static mec_status var_launch_locked(mec_ctx *ctx, const void *data_dev,
                                    void *parity_dev, void *sums_dev,
                                    const std::vector<int64_t> *extra = nullptr,
                                    const int64_t **extra_dev = nullptr) {
    const mec::VarPlan &pl = ctx->vplan;
    const size_t n = pl.items.size();
    auto al16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t item_bytes = n * sizeof(mec::VarItem);
    const size_t col_off = al16(item_bytes);
    const size_t col_bytes = (n + 1) * sizeof(int64_t);
    const size_t ord_off = al16(col_off + col_bytes);
    const size_t ext_off = al16(ord_off + n * sizeof(uint32_t));
    const size_t ext_bytes = extra ? extra->size() * sizeof(int64_t) : 0;
    const size_t end = al16(ext_off + ext_bytes);

    const int slot = ctx->e_idx & 1;
    ctx->e_idx ^= 1;
    if (!ctx->ev_e[slot])
        HIP_TRY(hipEventCreateWithFlags(&ctx->ev_e[slot],
                                        hipEventDisableTiming));
    else
        HIP_TRY(hipEventSynchronize(ctx->ev_e[slot]));
    if (ctx->cap_pin_e[slot] < end) {
        if (ctx->pin_e[slot]) (void)hipHostFree(ctx->pin_e[slot]);
        ctx->pin_e[slot] = nullptr;
        ctx->cap_pin_e[slot] = 0;
        HIP_TRY(hipHostMalloc(&ctx->pin_e[slot], end * 2));
        ctx->cap_pin_e[slot] = end * 2;
    }
    /* growing dev_e frees the old buffer, which waits for the kernels
     * still reading it; grow with slack so that stays rare */
    if (ctx->cap_e < end) {
        mec_status st = ctx->ensure(&ctx->dev_e, &ctx->cap_e, end * 2);
        if (st != MEC_OK) return st;
    }
    uint8_t *pinb = (uint8_t *)ctx->pin_e[slot];
    memcpy(pinb, pl.items.data(), item_bytes);
    memcpy(pinb + col_off, pl.col_off.data(), col_bytes);
    memcpy(pinb + ord_off, pl.order.data(), n * sizeof(uint32_t));
    if (extra) memcpy(pinb + ext_off, extra->data(), ext_bytes);
    HIP_TRY(hipMemcpyAsync(ctx->dev_e, pinb, end, hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev_e[slot], ctx->stream));

    const uint8_t *de = (const uint8_t *)ctx->dev_e;
    if (extra_dev) *extra_dev = (const int64_t *)(de + ext_off);
    EncVarArgs a{};
    a.data = (const uint8_t *)data_dev;
    a.parity = (uint8_t *)parity_dev;
    a.sums = (uint8_t *)sums_dev;
    a.items = (const int64_t *)de;
    a.col_off = (const int64_t *)(de + col_off);
    a.order = (const uint32_t *)(de + ord_off);
    a.cols_total = pl.cols_total;
    a.n = (uint32_t)n;
    a.d = ctx->d;
    a.p = ctx->p;
    memcpy(a.key, kMagicHHKey, 32);
    hipError_t he = mec_launch_encode_var(&a, ctx->stream);
    if (he != hipSuccess) {
        set_err("encode_var", he);
        return MEC_ERR_HIP;
    }
    return MEC_OK;
}

mec_status mec_encode_batch_var_dev_async(mec_ctx *ctx, int n,
                                          const void *data_dev,
                                          const int64_t *block_lens,
                                          void *parity_dev, int bitrot_algo,
                                          void *sums_dev) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status st = var_check_locked(ctx, n, data_dev, block_lens, parity_dev,
                                     bitrot_algo, sums_dev);
    if (st != MEC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    return var_launch_locked(ctx, data_dev, parity_dev, sums_dev);
}

mec_status mec_encode_batch_var_dev(mec_ctx *ctx, int n, const void *data_dev,
                                    const int64_t *block_lens,
                                    void *parity_dev, int bitrot_algo,
                                    void *sums_dev) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status st = var_check_locked(ctx, n, data_dev, block_lens, parity_dev,
                                     bitrot_algo, sums_dev);
    if (st != MEC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    st = var_launch_locked(ctx, data_dev, parity_dev, sums_dev);
    if (st != MEC_OK) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_encode_batch_var(mec_ctx *ctx, int n, const uint8_t *data,
                                const int64_t *block_lens, uint8_t *parity,
                                int bitrot_algo, uint8_t *sums) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status st = var_check_locked(ctx, n, data, block_lens, parity,
                                     bitrot_algo, sums);
    if (st != MEC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    const mec::VarPlan &pl = ctx->vplan;
    const int d = ctx->d, p = ctx->p;
    const size_t data_bytes = (size_t)d * pl.rows_total;
    const size_t par_bytes = (size_t)p * pl.rows_total;
    const size_t sum_bytes = sums ? (size_t)n * (d + p) * 32 : 0;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, data_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure(&ctx->dev_b, &ctx->cap_b, par_bytes)) != MEC_OK)
        return st;
    if (sums &&
        (st = ctx->ensure(&ctx->dev_c, &ctx->cap_c, sum_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(data_bytes > par_bytes + sum_bytes
                                  ? data_bytes
                                  : par_bytes + sum_bytes)) != MEC_OK)
        return st;

    /* Split scatter into pinned staging, then a plain unchunked upload, as
     * mec_reconstruct_batch_mixed. */
    uint8_t *pinb = (uint8_t *)ctx->pin;
    var_scatter_host(pl, d, data, block_lens, pinb);
    HIP_TRY(hipMemcpyAsync(ctx->dev_a, pinb, data_bytes, hipMemcpyHostToDevice,
                           ctx->stream));
    st = var_launch_locked(ctx, ctx->dev_a, ctx->dev_b,
                           sums ? ctx->dev_c : nullptr);
    if (st != MEC_OK) return st;
    HIP_TRY(hipMemcpyAsync(pinb, ctx->dev_b, par_bytes, hipMemcpyDeviceToHost,
                           ctx->stream));
    if (sums)
        HIP_TRY(hipMemcpyAsync(pinb + par_bytes, ctx->dev_c, sum_bytes,
                               hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    /* gather parity packed: item b's p rows of S_b bytes */
    uint8_t *out = parity;
    for (int b = 0; b < n; b++) {
        const int64_t S = pl.items[(size_t)b].shard_len;
        const int64_t stride = (S + 63) & ~int64_t(63);
        const uint8_t *rows = pinb + (size_t)p * pl.items[(size_t)b].row_off;
        for (int t = 0; t < p; t++, out += S)
            memcpy(out, rows + (size_t)t * stride, (size_t)S);
    }
    if (sums) memcpy(sums, pinb + par_bytes, sum_bytes);
    return MEC_OK;
}

/* ---- batch encode into on-disk [hash||shard] frames, length PER ITEM ---- */

mec_status mec_frame_offsets(int d, int64_t block_size, int n,
                             const int64_t *block_lens, int64_t *frame_off) {
    return mec::frame_offsets(d, block_size, n, block_lens, frame_off)
               ? MEC_OK
               : MEC_ERR_INVALID_ARG;
}

/* Everything that can be refused is refused here, before anything is
 * launched or written; on MEC_OK ctx->vplan and ctx->fplan hold the call's
 * plan. */
static mec_status frames_check_locked(mec_ctx *ctx, int n, const void *data,
                                      const int64_t *block_lens,
                                      const void *frames, int algo) {
    if (n <= 0 || !data || !block_lens || !frames) return MEC_ERR_INVALID_ARG;
    /* a frame's digest is HighwayHash-256 with the magic key; both ids name
     * that function */
    if (algo != MEC_BITROT_HIGHWAYHASH256S && algo != MEC_BITROT_HIGHWAYHASH256)
        return MEC_ERR_INVALID_ARG;
    if (var_geometry_check(ctx) != MEC_OK) return MEC_ERR_INVALID_ARG;
    if (!mec::build_frames_plan(ctx->d, ctx->d + ctx->p, ctx->block_size, n,
                                block_lens, &ctx->vplan, &ctx->fplan))
        return MEC_ERR_INVALID_ARG;
    return MEC_OK;
}

/* The encode's two launches into context scratch, then the pack.  Never
 * synchronizes the stream (but see var_launch_locked on the pinned slots). */
static mec_status frames_launch_locked(mec_ctx *ctx, const void *data_dev,
                                       void *frames_dev) {
    const mec::VarPlan &pl = ctx->vplan;
    const int d = ctx->d, p = ctx->p;
    const size_t n = pl.items.size();
    /* R_n is a multiple of 64, so the sums table starts aligned */
    const size_t par_bytes = (size_t)p * pl.rows_total;
    const size_t need = par_bytes + n * (size_t)(d + p) * 32;
    /* growing dev_f frees the old buffer, which waits for the kernels
     * still using it; grow with a quarter of slack so that stays rare (the
     * buffer is p/d of the input, so not doubled as the tables are) */
    if (ctx->cap_f < need) {
        mec_status st =
            ctx->ensure(&ctx->dev_f, &ctx->cap_f, need + need / 4);
        if (st != MEC_OK) return st;
    }
    uint8_t *parity = (uint8_t *)ctx->dev_f;
    uint8_t *sums = parity + par_bytes;
    const int64_t *f_dev = nullptr;
    mec_status st = var_launch_locked(ctx, data_dev, parity, sums,
                                      &ctx->fplan.frame_off, &f_dev);
    if (st != MEC_OK) return st;

    FramesPackArgs a{};
    a.data = (const uint8_t *)data_dev;
    a.parity = parity;
    a.sums = sums;
    a.out = (uint8_t *)frames_dev;
    a.items = (const int64_t *)ctx->dev_e;
    a.frame_off = f_dev;
    a.fn = ctx->fplan.frame_off[n];
    a.bytes = ctx->fplan.frames_bytes;
    a.a0 = (uint32_t)((uintptr_t)frames_dev & 15);
    a.granules = ((int64_t)a.a0 + a.bytes + 15) >> 4;
    a.n = (uint32_t)n;
    a.d = d;
    a.p = p;
    hipError_t he = mec_launch_frames_pack(&a, ctx->stream);
    if (he != hipSuccess) {
        set_err("frames_pack", he);
        return MEC_ERR_HIP;
    }
    return MEC_OK;
}

mec_status mec_encode_frames_batch_var_dev_async(mec_ctx *ctx, int n,
                                                 const void *data_dev,
                                                 const int64_t *block_lens,
                                                 void *frames_dev,
                                                 int bitrot_algo) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status st = frames_check_locked(ctx, n, data_dev, block_lens,
                                        frames_dev, bitrot_algo);
    if (st != MEC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    return frames_launch_locked(ctx, data_dev, frames_dev);
}

mec_status mec_encode_frames_batch_var_dev(mec_ctx *ctx, int n,
                                           const void *data_dev,
                                           const int64_t *block_lens,
                                           void *frames_dev,
                                           int bitrot_algo) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status st = frames_check_locked(ctx, n, data_dev, block_lens,
                                        frames_dev, bitrot_algo);
    if (st != MEC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    st = frames_launch_locked(ctx, data_dev, frames_dev);
    if (st != MEC_OK) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_encode_frames_batch_var(mec_ctx *ctx, int n,
                                       const uint8_t *data,
                                       const int64_t *block_lens,
                                       uint8_t *frames, int bitrot_algo) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status st =
        frames_check_locked(ctx, n, data, block_lens, frames, bitrot_algo);
    if (st != MEC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    const mec::VarPlan &pl = ctx->vplan;
    const size_t data_bytes = (size_t)ctx->d * pl.rows_total;
    const size_t out_bytes = (size_t)ctx->fplan.frames_bytes;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, data_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure(&ctx->dev_d, &ctx->cap_d, out_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(data_bytes)) != MEC_OK) return st;
    /* Split scatter into pinned staging, one plain upload (no overlapped
     * ingest), the device path, one D2H of every row stream */
    uint8_t *pinb = (uint8_t *)ctx->pin;
    var_scatter_host(pl, ctx->d, data, block_lens, pinb);
    HIP_TRY(hipMemcpyAsync(ctx->dev_a, pinb, data_bytes, hipMemcpyHostToDevice,
                           ctx->stream));
    st = frames_launch_locked(ctx, ctx->dev_a, ctx->dev_d);
    if (st != MEC_OK) return st;
    HIP_TRY(hipMemcpyAsync(frames, ctx->dev_d, out_bytes,
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

/* ---- batch reconstruct ------------------------------------------------- */

static mec_status reconstruct_dev_locked(mec_ctx *ctx, int n,
                                         void *shards_dev,
                                         const uint8_t *present,
                                         int64_t shard_len, int data_only) {
    if (n <= 0 || shard_len <= 0 || shard_len > ctx->stride)
        return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const int d = ctx->d, p = ctx->p, total = d + p;
    int src_idx[mec::kMaxShards], dst_idx[mec::kMaxShards], n_dst = 0;
    std::vector<uint8_t> dec((size_t)total * d);
    /* all present -> nothing to do (Reconstruct fast path) */
    int n_present = 0;
    for (int i = 0; i < total; i++)
        if (present[i]) n_present++;
    if (n_present == total) return MEC_OK;
    if (n_present < d) return MEC_ERR_TOO_FEW_SHARDS;
    if (!mec::build_decode_plan(ctx->enc_matrix.data(), d, p, present,
                                data_only, src_idx, dst_idx, &n_dst,
                                dec.data()))
        return MEC_ERR_TOO_FEW_SHARDS;
    if (n_dst == 0) return MEC_OK;

    for (int t0 = 0; t0 < n_dst; t0 += MEC_KMAX_E) {
        int e = n_dst - t0 > MEC_KMAX_E ? MEC_KMAX_E : n_dst - t0;
        GfMatmulArgs a{};
        a.src = (const uint8_t *)shards_dev;
        a.dst = (uint8_t *)shards_dev;
        a.src_item_stride = (int64_t)total * ctx->stride;
        a.dst_item_stride = (int64_t)total * ctx->stride;
        a.row_stride = ctx->stride;
        a.shard_len = shard_len;
        a.d = d;
        for (int k = 0; k < d; k++) a.src_rows[k] = (uint8_t)src_idx[k];
        for (int i = 0; i < e; i++) a.dst_rows[i] = (uint8_t)dst_idx[t0 + i];
        for (int i = 0; i < e; i++)
            for (int k = 0; k < d; k++)
                a.mat[i * MEC_KMAX_D + k] = dec[(size_t)(t0 + i) * d + k];
        mec_status st = bs_masks_dev(ctx, a.mat, e, d, &a.bs_masks);
        if (st != MEC_OK) return st;
        HIP_TRY(mec_launch_gf_matmul(&a, e, n, ctx->stream));
    }
    return MEC_OK;
}

mec_status mec_reconstruct_batch_dev_async(mec_ctx *ctx, int n,
                                           void *shards_dev,
                                           const uint8_t *present,
                                           int64_t shard_len, int data_only) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return reconstruct_dev_locked(ctx, n, shards_dev, present, shard_len,
                                  data_only);
}

mec_status mec_reconstruct_batch_dev(mec_ctx *ctx, int n, void *shards_dev,
                                     const uint8_t *present,
                                     int64_t shard_len, int data_only) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status s = reconstruct_dev_locked(ctx, n, shards_dev, present,
                                          shard_len, data_only);
    if (s != MEC_OK) return s;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_reconstruct_batch(mec_ctx *ctx, int n, uint8_t *shards,
                                 const uint8_t *present, int64_t shard_len,
                                 int data_only) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (n <= 0 || shard_len <= 0 || shard_len > ctx->stride)
        return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const int total = ctx->d + ctx->p;
    const int64_t stride = ctx->stride;
    size_t bytes = (size_t)n * total * stride;
    mec_status st;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(bytes)) != MEC_OK) return st;
    uint8_t *pinb = (uint8_t *)ctx->pin;
    /* overlapped ingest (parallelReader-style): the batch is
     * fed to the GPU reconstruct queue in chunks — chunk c+1's host pack
     * and PCIe upload (stream2) run while chunk c's decode kernels run
     * (stream); the event handshake keeps kernel c after upload c. */
    const int64_t chunk = (n > 128) ? ((n + 3) / 4) : n;
    for (int64_t b0 = 0; b0 < n; b0 += chunk) {
        const int64_t nc = (b0 + chunk <= n) ? chunk : (n - b0);
        uint8_t *pc = pinb + (size_t)b0 * total * stride;
        for (int64_t b = 0; b < nc; b++)
            for (int s = 0; s < total; s++)
                memcpy(pc + ((size_t)b * total + s) * stride,
                       shards + ((size_t)(b0 + b) * total + s) * shard_len,
                       (size_t)shard_len);
        HIP_TRY(hipMemcpyAsync((uint8_t *)ctx->dev_a +
                                   (size_t)b0 * total * stride,
                               pc, (size_t)nc * total * stride,
                               hipMemcpyHostToDevice, ctx->stream2));
        HIP_TRY(hipEventRecord(ctx->ev_h, ctx->stream2));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_h, 0));
        st = reconstruct_dev_locked(
            ctx, (int)nc,
            (uint8_t *)ctx->dev_a + (size_t)b0 * total * stride, present,
            shard_len, data_only);
        if (st != MEC_OK) return st;
        HIP_TRY(hipMemcpyAsync(pc,
                               (uint8_t *)ctx->dev_a +
                                   (size_t)b0 * total * stride,
                               (size_t)nc * total * stride,
                               hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < n; b++)
        for (int s = 0; s < total; s++) {
            if (present[s]) continue; /* only missing rows were rebuilt */
            if (data_only && s >= ctx->d) continue;
            memcpy(shards + ((size_t)b * total + s) * shard_len,
                   pinb + ((size_t)b * total + s) * stride,
                   (size_t)shard_len);
        }
    return MEC_OK;
}

/* ---- batch reconstruct, one erasure pattern per item ------------------- */

/* Plans the call into ctx->plan.  With item_status NULL an unrecoverable
 * item fails the whole call here, before anything is launched. */
static mec_status mixed_plan_locked(mec_ctx *ctx, int n,
                                    const uint8_t *present, int data_only,
                                    uint8_t *item_status) {
    if (!mec::build_reconstruct_plan(ctx->enc_matrix.data(), ctx->d, ctx->p,
                                     n, present, data_only, &ctx->plan))
        return MEC_ERR_INTERNAL;
    if (ctx->plan.n_too_few && !item_status) return MEC_ERR_TOO_FEW_SHARDS;
    if (item_status) memcpy(item_status, ctx->plan.status.data(), (size_t)n);
    return MEC_OK;
}

/* Uploads ctx->plan and launches one kernel per output-row count in use.
 * Never synchronizes the stream; the only host wait is on the copy that
 * last read the pinned slot being refilled (two calls back).
 * With items_dev (the per-item-length read): the rows are in ctx->vplan's
 * packed layout, items_dev is its item table on the device, shard_len is
 * unused, and ctx->vtiles, the tile prefixes of the work lists, are staged
 * behind them for gf_matmul_bs_mixed_var_kernel. */
static mec_status mixed_launch_locked(mec_ctx *ctx, void *shards_dev,
                                      int64_t shard_len,
                                      const int64_t *items_dev = nullptr) {
    const mec::ReconPlan &pl = ctx->plan;
    if (pl.entries.empty()) return MEC_OK;
    auto al16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t ent_bytes = pl.entries.size() * sizeof(mec::ReconPlanEntry);
    const size_t mask_off = al16(ent_bytes);
    const size_t mask_bytes = pl.masks.size() * sizeof(uint32_t);
    size_t work_off[MEC_KMAX_E + 1];
    size_t end = al16(mask_off + mask_bytes);
    for (int e = 1; e <= MEC_KMAX_E; e++) {
        work_off[e] = end;
        end = al16(end + pl.work[e].size() * sizeof(mec::ReconWork));
    }
    size_t tile_off[MEC_KMAX_E + 1] = {0};
    if (items_dev)
        for (int e = 1; e <= MEC_KMAX_E; e++) {
            tile_off[e] = end;
            if (!pl.work[e].empty())
                end = al16(end + ctx->vtiles[e].size() * sizeof(int64_t));
        }

    const int slot = ctx->x_idx & 1;
    ctx->x_idx ^= 1;
    if (!ctx->ev_x[slot])
        HIP_TRY(hipEventCreateWithFlags(&ctx->ev_x[slot],
                                        hipEventDisableTiming));
    else
        HIP_TRY(hipEventSynchronize(ctx->ev_x[slot]));
    if (ctx->cap_pin_x[slot] < end) {
        if (ctx->pin_x[slot]) (void)hipHostFree(ctx->pin_x[slot]);
        ctx->pin_x[slot] = nullptr;
        ctx->cap_pin_x[slot] = 0;
        HIP_TRY(hipHostMalloc(&ctx->pin_x[slot], end * 2));
        ctx->cap_pin_x[slot] = end * 2;
    }
    /* growing dev_x frees the old buffer, which waits for the kernels
     * still reading it; grow with slack so that stays rare */
    if (ctx->cap_x < end) {
        mec_status st = ctx->ensure(&ctx->dev_x, &ctx->cap_x, end * 2);
        if (st != MEC_OK) return st;
    }
    uint8_t *pinb = (uint8_t *)ctx->pin_x[slot];
    memcpy(pinb, pl.entries.data(), ent_bytes);
    memcpy(pinb + mask_off, pl.masks.data(), mask_bytes);
    for (int e = 1; e <= MEC_KMAX_E; e++)
        if (!pl.work[e].empty())
            memcpy(pinb + work_off[e], pl.work[e].data(),
                   pl.work[e].size() * sizeof(mec::ReconWork));
    if (items_dev)
        for (int e = 1; e <= MEC_KMAX_E; e++)
            if (!pl.work[e].empty())
                memcpy(pinb + tile_off[e], ctx->vtiles[e].data(),
                       ctx->vtiles[e].size() * sizeof(int64_t));
    HIP_TRY(hipMemcpyAsync(ctx->dev_x, pinb, end, hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev_x[slot], ctx->stream));

    const uint8_t *dx = (const uint8_t *)ctx->dev_x;
    if (items_dev) {
        GfMixedVarArgs v{};
        v.shards = (uint8_t *)shards_dev;
        v.items = items_dev;
        v.entries = (const uint32_t *)dx;
        v.masks = (const uint32_t *)(dx + mask_off);
        v.d = ctx->d;
        v.total = ctx->d + ctx->p;
        for (int e = 1; e <= MEC_KMAX_E; e++) {
            if (pl.work[e].empty()) continue;
            v.work = (const uint32_t *)(dx + work_off[e]);
            v.tiles = (const int64_t *)(dx + tile_off[e]);
            v.n_work = (uint32_t)pl.work[e].size();
            v.tiles_total = ctx->vtiles[e].back();
            HIP_TRY(mec_launch_gf_matmul_mixed_var(&v, e, ctx->stream));
        }
        return MEC_OK;
    }
    GfMixedArgs a{};
    a.shards = (uint8_t *)shards_dev;
    a.item_stride = (int64_t)(ctx->d + ctx->p) * ctx->stride;
    a.row_stride = ctx->stride;
    a.shard_len = shard_len;
    a.entries = (const uint32_t *)dx;
    a.masks = (const uint32_t *)(dx + mask_off);
    a.d = ctx->d;
    for (int e = 1; e <= MEC_KMAX_E; e++) {
        if (pl.work[e].empty()) continue;
        a.work = (const uint32_t *)(dx + work_off[e]);
        a.n_work = (uint32_t)pl.work[e].size();
        HIP_TRY(mec_launch_gf_matmul_mixed(&a, e, ctx->stream));
    }
    return MEC_OK;
}

static mec_status mixed_dev_locked(mec_ctx *ctx, int n, void *shards_dev,
                                   const uint8_t *present, int64_t shard_len,
                                   int data_only, uint8_t *item_status) {
    if (n <= 0 || !shards_dev || !present || shard_len <= 0 ||
        shard_len > ctx->stride)
        return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    mec_status st = mixed_plan_locked(ctx, n, present, data_only, item_status);
    if (st != MEC_OK) return st;
    return mixed_launch_locked(ctx, shards_dev, shard_len);
}

mec_status mec_reconstruct_batch_mixed_dev_async(
    mec_ctx *ctx, int n, void *shards_dev, const uint8_t *present,
    int64_t shard_len, int data_only, uint8_t *item_status) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return mixed_dev_locked(ctx, n, shards_dev, present, shard_len, data_only,
                            item_status);
}

mec_status mec_reconstruct_batch_mixed_dev(mec_ctx *ctx, int n,
                                           void *shards_dev,
                                           const uint8_t *present,
                                           int64_t shard_len, int data_only,
                                           uint8_t *item_status) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status s = mixed_dev_locked(ctx, n, shards_dev, present, shard_len,
                                    data_only, item_status);
    if (s != MEC_OK) return s;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_reconstruct_batch_mixed(mec_ctx *ctx, int n, uint8_t *shards,
                                       const uint8_t *present,
                                       int64_t shard_len, int data_only,
                                       uint8_t *item_status) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (n <= 0 || !shards || !present || shard_len <= 0 ||
        shard_len > ctx->stride)
        return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    mec_status st = mixed_plan_locked(ctx, n, present, data_only, item_status);
    if (st != MEC_OK) return st;
    if (ctx->plan.entries.empty()) return MEC_OK; /* nothing to rebuild */
    const int d = ctx->d, total = ctx->d + ctx->p;
    const int64_t stride = ctx->stride;
    const size_t bytes = (size_t)n * total * stride;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(bytes)) != MEC_OK) return st;
    uint8_t *pinb = (uint8_t *)ctx->pin;
    /* plain unchunked upload (the uniform call's overlapped ingest is a
     * follow-up for this path) */
    for (int64_t b = 0; b < n; b++)
        for (int s = 0; s < total; s++)
            memcpy(pinb + ((size_t)b * total + s) * stride,
                   shards + ((size_t)b * total + s) * shard_len,
                   (size_t)shard_len);
    HIP_TRY(hipMemcpyAsync(ctx->dev_a, pinb, bytes, hipMemcpyHostToDevice,
                           ctx->stream));
    if ((st = mixed_launch_locked(ctx, ctx->dev_a, shard_len)) != MEC_OK)
        return st;
    HIP_TRY(hipMemcpyAsync(pinb, ctx->dev_a, bytes, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    /* only rebuilt rows go back: unrecoverable and complete items, present
     * rows, and (data_only) parity rows keep the caller's bytes */
    for (int64_t b = 0; b < n; b++) {
        if (ctx->plan.status[b] != mec::kPlanOk) continue;
        const uint8_t *pr = present + (size_t)b * total;
        for (int s = 0; s < (data_only ? d : total); s++) {
            if (pr[s]) continue;
            memcpy(shards + ((size_t)b * total + s) * shard_len,
                   pinb + ((size_t)b * total + s) * stride,
                   (size_t)shard_len);
        }
    }
    return MEC_OK;
}

/* ---- verified batch read: bitrot check on device, then reconstruct ------ */

/* The reference does both in one operation: streamingBitrotReader.ReadAt
 * (cmd/bitrot-streaming.go:161-200) returns errFileCorrupt for a block
 * whose hash does not match, parallelReader.Read
 * (cmd/erasure-decode.go:127-235) drops that row and reads another, and
 * Decode/Heal reconstruct from what verified.
 *
 * Verifies the rows read_mask names, plans on read_mask & ok, launches the
 * mixed kernels and, with rehash, the digests of the rebuilt rows.  One
 * stream synchronise (the host needs the verdicts to plan); the caller
 * does the final one.  On return ctx->vpresent is the verified mask and,
 * with want_rebuilt, ctx->vlist the ids of the rows that were rebuilt. */
static mec_status verify_recon_locked(mec_ctx *ctx, int n, void *shards_dev,
                                      void *sums_dev,
                                      const uint8_t *read_mask,
                                      int64_t shard_len, int data_only,
                                      int rehash, bool want_rebuilt,
                                      uint8_t *present_out,
                                      uint8_t *item_status) {
    const int d = ctx->d, p = ctx->p, total = d + p;
    uint32_t count;
    if (!mec::verify_chain_count(n, total, &count)) return MEC_ERR_INVALID_ARG;
    if (!mec::build_verify_list(n, total, read_mask, &ctx->vlist))
        return MEC_ERR_INVALID_ARG;
    const size_t n_list = ctx->vlist.size();

    /* [list, room for every chain | ok bytes]: the size depends on the
     * call's dimensions only, not on its masks */
    const size_t ok_off = ((size_t)count * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t need = ok_off + count;
    mec_status st;
    if ((st = ctx->ensure(&ctx->dev_v, &ctx->cap_v, need)) != MEC_OK)
        return st;
    if (ctx->cap_pin_v < need) {
        if (ctx->pin_v) (void)hipHostFree(ctx->pin_v);
        ctx->pin_v = nullptr;
        ctx->cap_pin_v = 0;
        HIP_TRY(hipHostMalloc(&ctx->pin_v, need));
        ctx->cap_pin_v = need;
    }
    uint8_t *pinb = (uint8_t *)ctx->pin_v;
    uint8_t *dv = (uint8_t *)ctx->dev_v;

    HashListArgs h{};
    h.shards = (const uint8_t *)shards_dev;
    h.sums = (uint8_t *)sums_dev;
    h.ok = dv + ok_off;
    h.list = (const uint32_t *)dv;
    h.row_stride = ctx->stride;
    h.msg_len = shard_len;
    memcpy(h.key, kMagicHHKey, 32);

    if (n_list) {
        memcpy(pinb, ctx->vlist.data(), n_list * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(dv, pinb, n_list * sizeof(uint32_t),
                               hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipMemsetAsync(dv + ok_off, 0, count, ctx->stream));
    h.n_list = (uint32_t)n_list;
    HIP_TRY(mec_launch_hash_list(&h, 1, ctx->stream));
    HIP_TRY(hipMemcpyAsync(pinb + ok_off, dv + ok_off, count,
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));

    ctx->vpresent.resize(count);
    mec::merge_verified(count, read_mask, pinb + ok_off,
                        ctx->vpresent.data());
    if (present_out) memcpy(present_out, ctx->vpresent.data(), count);

    st = mixed_plan_locked(ctx, n, ctx->vpresent.data(), data_only,
                           item_status);
    if (st != MEC_OK) return st;
    if ((st = mixed_launch_locked(ctx, shards_dev, shard_len)) != MEC_OK)
        return st;

    ctx->vlist.clear();
    if ((rehash || want_rebuilt) && !ctx->plan.entries.empty())
        mec::build_rehash_list(ctx->plan, d, p, n, ctx->vpresent.data(),
                               data_only, &ctx->vlist);
    if (rehash && !ctx->vlist.empty()) {
        /* the verify kernel and the list upload are done (synchronised
         * above), so both list buffers can be refilled */
        const size_t nb = ctx->vlist.size() * sizeof(uint32_t);
        memcpy(pinb, ctx->vlist.data(), nb);
        HIP_TRY(hipMemcpyAsync(dv, pinb, nb, hipMemcpyHostToDevice,
                               ctx->stream));
        h.n_list = (uint32_t)ctx->vlist.size();
        HIP_TRY(mec_launch_hash_list(&h, 0, ctx->stream));
    }
    return MEC_OK;
}

static bool verify_recon_args_ok(mec_ctx *ctx, int n, const void *shards,
                                 const void *sums, const uint8_t *read_mask,
                                 int64_t shard_len, int bitrot_algo) {
    /* only the streaming format has per-block digests; both ids name the
     * same keyed function */
    if (bitrot_algo != MEC_BITROT_HIGHWAYHASH256S &&
        bitrot_algo != MEC_BITROT_HIGHWAYHASH256)
        return false;
    return n > 0 && shards && sums && read_mask && shard_len > 0 &&
           shard_len <= ctx->stride;
}

mec_status mec_verify_reconstruct_batch_dev(
    mec_ctx *ctx, int n, void *shards_dev, void *sums_dev,
    const uint8_t *read_mask, int64_t shard_len, int bitrot_algo,
    int data_only, int rehash, uint8_t *present_out, uint8_t *item_status) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (!verify_recon_args_ok(ctx, n, shards_dev, sums_dev, read_mask,
                              shard_len, bitrot_algo))
        return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    mec_status st = verify_recon_locked(ctx, n, shards_dev, sums_dev,
                                        read_mask, shard_len, data_only,
                                        rehash, false, present_out,
                                        item_status);
    if (st != MEC_OK) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_verify_reconstruct_batch(
    mec_ctx *ctx, int n, uint8_t *shards, uint8_t *sums,
    const uint8_t *read_mask, int64_t shard_len, int bitrot_algo,
    int data_only, int rehash, uint8_t *present_out, uint8_t *item_status) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (!verify_recon_args_ok(ctx, n, shards, sums, read_mask, shard_len,
                              bitrot_algo))
        return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const int total = ctx->d + ctx->p;
    uint32_t count;
    if (!mec::verify_chain_count(n, total, &count)) return MEC_ERR_INVALID_ARG;
    const int64_t stride = ctx->stride;
    /* rows, then digests, in one device buffer: one upload */
    const size_t row_bytes = (size_t)count * stride;
    const size_t sum_bytes = (size_t)count * 32;
    mec_status st;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, row_bytes + sum_bytes)) !=
        MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(row_bytes + sum_bytes)) != MEC_OK) return st;
    uint8_t *pinb = (uint8_t *)ctx->pin;
    uint8_t *dev_rows = (uint8_t *)ctx->dev_a;
    uint8_t *dev_sums = dev_rows + row_bytes;
    /* only rows that were read are packed; the others' device bytes are
     * whatever the buffer held, which nothing reads */
    for (uint32_t c = 0; c < count; c++)
        if (read_mask[c])
            memcpy(pinb + (size_t)c * stride, shards + (size_t)c * shard_len,
                   (size_t)shard_len);
    memcpy(pinb + row_bytes, sums, sum_bytes);
    HIP_TRY(hipMemcpyAsync(dev_rows, pinb, row_bytes + sum_bytes,
                           hipMemcpyHostToDevice, ctx->stream));
    st = verify_recon_locked(ctx, n, dev_rows, dev_sums, read_mask, shard_len,
                             data_only, rehash, true, present_out,
                             item_status);
    if (st != MEC_OK) return st;
    if (ctx->vlist.empty()) { /* nothing was rebuilt */
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return MEC_OK;
    }
    HIP_TRY(hipMemcpyAsync(pinb, dev_rows,
                           row_bytes + (rehash ? sum_bytes : 0),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    /* only rebuilt rows go back, with their fresh digests under rehash */
    for (uint32_t c : ctx->vlist) {
        memcpy(shards + (size_t)c * shard_len, pinb + (size_t)c * stride,
               (size_t)shard_len);
        if (rehash)
            memcpy(sums + (size_t)c * 32, pinb + row_bytes + (size_t)c * 32,
                   32);
    }
    return MEC_OK;
}

/* ---- verified batch read, one shard length PER ITEM --------------------- */

/* parallelReader.Read shortens shardSize for the last block of an object
 * (cmd/erasure-decode.go:138-139), so a GET or heal batch across objects
 * has a shard length per item.  Everything that can be refused is refused
 * here, before anything is launched or written; on MEC_OK ctx->vplan holds
 * the call's item table and hash order. */
static mec_status read_var_check_locked(mec_ctx *ctx, int n,
                                        const void *shards, const void *sums,
                                        const int64_t *block_lens,
                                        const uint8_t *read_mask,
                                        int bitrot_algo) {
    if (n <= 0 || !shards || !sums || !block_lens || !read_mask)
        return MEC_ERR_INVALID_ARG;
    if (bitrot_algo != MEC_BITROT_HIGHWAYHASH256S &&
        bitrot_algo != MEC_BITROT_HIGHWAYHASH256)
        return MEC_ERR_INVALID_ARG;
    /* also refuses n*(d+p) past 32 bits (chain ids) */
    if (!mec::build_var_plan(ctx->d, ctx->d + ctx->p, ctx->block_size, n,
                             block_lens, &ctx->vplan))
        return MEC_ERR_INVALID_ARG;
    return MEC_OK;
}

/* verify_recon_locked with ctx->vplan's packed rows: the lists are in the
 * plan's hash order, the item table travels with the first list, and the
 * mixed launch takes the tile prefixes along.  Same synchronisation: one
 * before planning, the caller does the final one. */
static mec_status verify_recon_var_locked(mec_ctx *ctx, int n,
                                          void *shards_dev, void *sums_dev,
                                          const uint8_t *read_mask,
                                          int data_only, int rehash,
                                          bool want_rebuilt,
                                          uint8_t *present_out,
                                          uint8_t *item_status) {
    const int d = ctx->d, p = ctx->p, total = d + p;
    const mec::VarPlan &vp = ctx->vplan;
    uint32_t count;
    if (!mec::verify_chain_count(n, total, &count)) return MEC_ERR_INVALID_ARG;
    mec::build_verify_list_ordered(vp, total, read_mask, &ctx->vlist);
    const size_t n_list = ctx->vlist.size();

    /* [list, room for every chain | ok bytes | item table] */
    auto al16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t ok_off = al16((size_t)count * sizeof(uint32_t));
    const size_t item_off = al16(ok_off + count);
    const size_t item_bytes = (size_t)n * sizeof(mec::VarItem);
    const size_t need = item_off + item_bytes;
    mec_status st;
    if ((st = ctx->ensure(&ctx->dev_v, &ctx->cap_v, need)) != MEC_OK)
        return st;
    if (ctx->cap_pin_v < need) {
        if (ctx->pin_v) (void)hipHostFree(ctx->pin_v);
        ctx->pin_v = nullptr;
        ctx->cap_pin_v = 0;
        HIP_TRY(hipHostMalloc(&ctx->pin_v, need));
        ctx->cap_pin_v = need;
    }
    uint8_t *pinb = (uint8_t *)ctx->pin_v;
    uint8_t *dv = (uint8_t *)ctx->dev_v;
    const int64_t *items_dev = (const int64_t *)(dv + item_off);

    HashListVarArgs h{};
    h.shards = (const uint8_t *)shards_dev;
    h.sums = (uint8_t *)sums_dev;
    h.ok = dv + ok_off;
    h.list = (const uint32_t *)dv;
    h.items = items_dev;
    h.total = (uint32_t)total;
    memcpy(h.key, kMagicHHKey, 32);

    memcpy(pinb + item_off, vp.items.data(), item_bytes);
    HIP_TRY(hipMemcpyAsync(dv + item_off, pinb + item_off, item_bytes,
                           hipMemcpyHostToDevice, ctx->stream));
    if (n_list) {
        memcpy(pinb, ctx->vlist.data(), n_list * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(dv, pinb, n_list * sizeof(uint32_t),
                               hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipMemsetAsync(dv + ok_off, 0, count, ctx->stream));
    h.n_list = (uint32_t)n_list;
    HIP_TRY(mec_launch_hash_list_var(&h, 1, ctx->stream));
    HIP_TRY(hipMemcpyAsync(pinb + ok_off, dv + ok_off, count,
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));

    ctx->vpresent.resize(count);
    mec::merge_verified(count, read_mask, pinb + ok_off,
                        ctx->vpresent.data());
    if (present_out) memcpy(present_out, ctx->vpresent.data(), count);

    st = mixed_plan_locked(ctx, n, ctx->vpresent.data(), data_only,
                           item_status);
    if (st != MEC_OK) return st;
    for (int e = 1; e <= MEC_KMAX_E; e++)
        if (!ctx->plan.work[e].empty() &&
            !mec::build_tile_prefix(vp, ctx->plan.work[e], &ctx->vtiles[e]))
            return MEC_ERR_INTERNAL;
    if ((st = mixed_launch_locked(ctx, shards_dev, 0, items_dev)) != MEC_OK)
        return st;

    ctx->vlist.clear();
    if ((rehash || want_rebuilt) && !ctx->plan.entries.empty())
        mec::build_rehash_list_ordered(vp, ctx->plan, d, p,
                                       ctx->vpresent.data(), data_only,
                                       &ctx->vlist);
    if (rehash && !ctx->vlist.empty()) {
        /* the verify kernel and the list upload are done (synchronised
         * above), so both list buffers can be refilled */
        const size_t nb = ctx->vlist.size() * sizeof(uint32_t);
        memcpy(pinb, ctx->vlist.data(), nb);
        HIP_TRY(hipMemcpyAsync(dv, pinb, nb, hipMemcpyHostToDevice,
                               ctx->stream));
        h.n_list = (uint32_t)ctx->vlist.size();
        HIP_TRY(mec_launch_hash_list_var(&h, 0, ctx->stream));
    }
    return MEC_OK;
}

mec_status mec_verify_reconstruct_batch_var_dev(
    mec_ctx *ctx, int n, void *shards_dev, void *sums_dev,
    const int64_t *block_lens, const uint8_t *read_mask, int bitrot_algo,
    int data_only, int rehash, uint8_t *present_out, uint8_t *item_status) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status st = read_var_check_locked(ctx, n, shards_dev, sums_dev,
                                          block_lens, read_mask, bitrot_algo);
    if (st != MEC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    st = verify_recon_var_locked(ctx, n, shards_dev, sums_dev, read_mask,
                                 data_only, rehash, false, present_out,
                                 item_status);
    if (st != MEC_OK) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_verify_reconstruct_batch_var(
    mec_ctx *ctx, int n, uint8_t *shards, uint8_t *sums,
    const int64_t *block_lens, const uint8_t *read_mask, int bitrot_algo,
    int data_only, int rehash, uint8_t *present_out, uint8_t *item_status) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    mec_status st = read_var_check_locked(ctx, n, shards, sums, block_lens,
                                          read_mask, bitrot_algo);
    if (st != MEC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    const mec::VarPlan &vp = ctx->vplan;
    const int total = ctx->d + ctx->p;
    const uint32_t count = (uint32_t)((int64_t)n * total);
    /* rows, then digests, in one device buffer: one upload */
    const size_t row_bytes = (size_t)total * vp.rows_total;
    const size_t sum_bytes = (size_t)count * 32;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, row_bytes + sum_bytes)) !=
        MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(row_bytes + sum_bytes)) != MEC_OK) return st;
    uint8_t *pinb = (uint8_t *)ctx->pin;
    uint8_t *dev_rows = (uint8_t *)ctx->dev_a;
    uint8_t *dev_sums = dev_rows + row_bytes;
    /* the caller's rows are packed at S_i: item i's rows start at
     * total * sum_{j<i} S_j */
    std::vector<int64_t> &hoff = ctx->vhost_off;
    hoff.resize((size_t)n);
    int64_t acc = 0;
    for (int i = 0; i < n; i++) {
        hoff[(size_t)i] = acc;
        acc += vp.items[(size_t)i].shard_len;
    }
    /* only rows that were read are packed; the others' device bytes are
     * whatever the buffer held, which nothing reads */
    for (int i = 0; i < n; i++) {
        const int64_t S = vp.items[(size_t)i].shard_len;
        const int64_t stride = (S + 63) & ~int64_t(63);
        const uint8_t *src = shards + (size_t)total * hoff[(size_t)i];
        uint8_t *dst = pinb + (size_t)total * vp.items[(size_t)i].row_off;
        for (int s = 0; s < total; s++)
            if (read_mask[(size_t)i * total + s])
                memcpy(dst + (size_t)s * stride, src + (size_t)s * S,
                       (size_t)S);
    }
    memcpy(pinb + row_bytes, sums, sum_bytes);
    HIP_TRY(hipMemcpyAsync(dev_rows, pinb, row_bytes + sum_bytes,
                           hipMemcpyHostToDevice, ctx->stream));
    st = verify_recon_var_locked(ctx, n, dev_rows, dev_sums, read_mask,
                                 data_only, rehash, true, present_out,
                                 item_status);
    if (st != MEC_OK) return st;
    if (ctx->vlist.empty()) { /* nothing was rebuilt */
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return MEC_OK;
    }
    HIP_TRY(hipMemcpyAsync(pinb, dev_rows,
                           row_bytes + (rehash ? sum_bytes : 0),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    /* only rebuilt rows go back, with their fresh digests under rehash */
    for (uint32_t c : ctx->vlist) {
        const uint32_t i = c / (uint32_t)total, s = c - i * (uint32_t)total;
        const int64_t S = vp.items[i].shard_len;
        const int64_t stride = (S + 63) & ~int64_t(63);
        memcpy(shards + (size_t)total * hoff[i] + (size_t)s * S,
               pinb + (size_t)total * vp.items[i].row_off +
                   (size_t)s * stride,
               (size_t)S);
        if (rehash)
            memcpy(sums + (size_t)c * 32, pinb + row_bytes + (size_t)c * 32,
                   32);
    }
    return MEC_OK;
}

/* ---- batch hashing / verification -------------------------------------- */

mec_status mec_bitrot_sum_batch_dev(mec_ctx *ctx, int algo, int n,
                                    const void *msgs_dev, int64_t msg_len,
                                    int64_t msg_stride, void *sums_dev) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (n <= 0 || msg_len < 0 || !hash_size(algo)) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    HashArgs h{};
    h.data = (const uint8_t *)msgs_dev;
    h.parity = nullptr;
    h.sums = (uint8_t *)sums_dev;
    h.row_stride = msg_stride;
    h.msg_len = msg_len;
    h.n_chains = n;
    memcpy(h.key, kMagicHHKey, 32);
    HIP_TRY(mec_launch_hash(algo, &h, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_bitrot_sum_batch(mec_ctx *ctx, int algo, int n,
                                const uint8_t *msgs, int64_t msg_len,
                                int64_t msg_stride, uint8_t *sums) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (n <= 0 || msg_len < 0 || !hash_size(algo)) return MEC_ERR_INVALID_ARG;
    const int hsz = hash_size(algo);
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    int64_t dstride = (msg_len + 63) & ~int64_t(63);
    if (dstride == 0) dstride = 64;
    size_t in_bytes = (size_t)n * dstride;
    size_t out_bytes = (size_t)n * hsz;
    mec_status st;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, in_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure(&ctx->dev_c, &ctx->cap_c, out_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(in_bytes > out_bytes ? in_bytes : out_bytes)) !=
        MEC_OK)
        return st;
    uint8_t *pinb = (uint8_t *)ctx->pin;
    /* overlapped ingest: chunk c+1's host pack + PCIe
     * upload (stream2) overlap chunk c's hash kernel (stream) — the
     * GPU-side analogue of parallelReader's overlapped shard reads
     * feeding verify-on-read (cmd/erasure-decode.go:127-235). */
    const int64_t chunk = (n > 512) ? ((n + 3) / 4) : n;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t nc = (i0 + chunk <= n) ? chunk : (n - i0);
        uint8_t *pc = pinb + (size_t)i0 * dstride;
        for (int64_t i = 0; i < nc; i++)
            memcpy(pc + (size_t)i * dstride,
                   msgs + (size_t)(i0 + i) * msg_stride, (size_t)msg_len);
        HIP_TRY(hipMemcpyAsync((uint8_t *)ctx->dev_a + (size_t)i0 * dstride,
                               pc, (size_t)nc * dstride,
                               hipMemcpyHostToDevice, ctx->stream2));
        HIP_TRY(hipEventRecord(ctx->ev_h, ctx->stream2));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_h, 0));
        HashArgs h{};
        h.data = (const uint8_t *)ctx->dev_a + (size_t)i0 * dstride;
        h.parity = nullptr;
        h.sums = (uint8_t *)ctx->dev_c + (size_t)i0 * hsz;
        h.row_stride = dstride;
        h.msg_len = msg_len;
        h.n_chains = nc;
        memcpy(h.key, kMagicHHKey, 32);
        HIP_TRY(mec_launch_hash(algo, &h, ctx->stream));
    }
    HIP_TRY(hipMemcpyAsync(pinb, ctx->dev_c, out_bytes, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(sums, pinb, out_bytes);
    return MEC_OK;
}

mec_status mec_bitrot_verify_batch(mec_ctx *ctx, int algo, int n,
                                   const uint8_t *msgs, int64_t msg_len,
                                   int64_t msg_stride, const uint8_t *want,
                                   uint8_t *ok_out) {
    const int hsz = hash_size(algo);
    if (!hsz) return MEC_ERR_INVALID_ARG;
    std::vector<uint8_t> got((size_t)n * hsz);
    mec_status st = mec_bitrot_sum_batch(ctx, algo, n, msgs, msg_len,
                                         msg_stride, got.data());
    if (st != MEC_OK) return st;
    for (int i = 0; i < n; i++)
        ok_out[i] = memcmp(got.data() + (size_t)i * hsz,
                           want + (size_t)i * hsz, (size_t)hsz) == 0;
    return MEC_OK;
}

/* ---- batch scrub -------------------------------------------------------- */

mec_status mec_scrub_file_offsets(int n, const int64_t *file_sizes,
                                  int64_t *file_off) {
    return mec::scrub_file_offsets(n, file_sizes, file_off)
               ? MEC_OK
               : MEC_ERR_INVALID_ARG;
}

/* Hash ctx->splan's chains over files_dev and reduce: the tables go up in
 * one copy, at most two launches, the ok bytes come back in one copy, one
 * stream synchronise. */
static mec_status scrub_run_locked(mec_ctx *ctx, const void *files_dev,
                                   uint8_t *file_status, int64_t *first_bad) {
    const mec::ScrubPlan &pl = ctx->splan;
    const size_t n = pl.files.size();
    const size_t na = pl.aligned.size(), ns = pl.sheared.size();
    const size_t count = na + ns;
    const uint8_t *ok = nullptr;
    if (count) {
        /* [file table | aligned list | sheared list | ok bytes] */
        auto al16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        const size_t tab_bytes = n * sizeof(mec::ScrubFile);
        const size_t list_off = al16(tab_bytes);
        const size_t ok_off = al16(list_off + count * sizeof(mec::ScrubChain));
        const size_t need = ok_off + count;
        mec_status st;
        if ((st = ctx->ensure(&ctx->dev_v, &ctx->cap_v, need)) != MEC_OK)
            return st;
        if (ctx->cap_pin_v < need) {
            if (ctx->pin_v) (void)hipHostFree(ctx->pin_v);
            ctx->pin_v = nullptr;
            ctx->cap_pin_v = 0;
            HIP_TRY(hipHostMalloc(&ctx->pin_v, need));
            ctx->cap_pin_v = need;
        }
        uint8_t *pinb = (uint8_t *)ctx->pin_v;
        uint8_t *dv = (uint8_t *)ctx->dev_v;
        memcpy(pinb, pl.files.data(), tab_bytes);
        if (na)
            memcpy(pinb + list_off, pl.aligned.data(),
                   na * sizeof(mec::ScrubChain));
        if (ns)
            memcpy(pinb + list_off + na * sizeof(mec::ScrubChain),
                   pl.sheared.data(), ns * sizeof(mec::ScrubChain));
        HIP_TRY(hipMemcpyAsync(dv, pinb, ok_off, hipMemcpyHostToDevice,
                               ctx->stream));
        HashFramesArgs h{};
        h.files = (const uint8_t *)files_dev;
        h.table = (const int64_t *)dv;
        memcpy(h.key, kMagicHHKey, 32);
        h.list = (const uint32_t *)(dv + list_off);
        h.ok = dv + ok_off;
        h.n_list = (uint32_t)na;
        HIP_TRY(mec_launch_hash_frames(&h, 0, ctx->stream));
        h.list += 2 * na;
        h.ok += na;
        h.n_list = (uint32_t)ns;
        HIP_TRY(mec_launch_hash_frames(&h, 1, ctx->stream));
        HIP_TRY(hipMemcpyAsync(pinb + ok_off, dv + ok_off, count,
                               hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ok = pinb + ok_off;
    }
    ctx->scorrupt.resize(n);
    mec::reduce_scrub(pl, ok, ctx->scorrupt.data(), first_bad);
    for (size_t f = 0; f < n; f++)
        file_status[f] =
            ctx->scorrupt[f] ? (uint8_t)MEC_ERR_FILE_CORRUPT : (uint8_t)MEC_OK;
    return MEC_OK;
}

mec_status mec_bitrot_verify_files_dev(
    mec_ctx *ctx, int n, const void *files_dev, int64_t files_bytes,
    const int64_t *file_off, const int64_t *file_sizes,
    const int64_t *part_sizes, const int64_t *shard_sizes, int bitrot_algo,
    uint8_t *file_status, int64_t *first_bad) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (n <= 0 || !files_dev || !file_status ||
        bitrot_algo != MEC_BITROT_HIGHWAYHASH256S)
        return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!mec::build_scrub_plan(n, file_off, file_sizes, part_sizes,
                               shard_sizes, files_bytes,
                               (unsigned)((uintptr_t)files_dev & 7),
                               &ctx->splan))
        return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return scrub_run_locked(ctx, files_dev, file_status, first_bad);
}

mec_status mec_bitrot_verify_files(mec_ctx *ctx, int n,
                                   const uint8_t *const *files,
                                   const int64_t *file_sizes,
                                   const int64_t *part_sizes,
                                   const int64_t *shard_sizes,
                                   int bitrot_algo, uint8_t *file_status,
                                   int64_t *first_bad) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    if (n <= 0 || !files || !file_sizes || !file_status ||
        bitrot_algo != MEC_BITROT_HIGHWAYHASH256S)
        return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::vector<int64_t> &off = ctx->shost_off;
    off.resize((size_t)n + 1);
    if (!mec::scrub_file_offsets(n, file_sizes, off.data()))
        return MEC_ERR_INVALID_ARG;
    for (int f = 0; f < n; f++)
        if (file_sizes[f] > 0 && !files[f]) return MEC_ERR_INVALID_ARG;
    /* the staging buffers are 64-byte aligned and so is every offset */
    if (!mec::build_scrub_plan(n, off.data(), file_sizes, part_sizes,
                               shard_sizes, off[(size_t)n], 0, &ctx->splan))
        return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    /* nothing to hash: the verdicts are all early ones */
    if (ctx->splan.aligned.empty() && ctx->splan.sheared.empty())
        return scrub_run_locked(ctx, nullptr, file_status, first_bad);
    const size_t bytes = (size_t)off[(size_t)n];
    mec_status st;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a, bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure_pin(bytes)) != MEC_OK) return st;
    uint8_t *pinb = (uint8_t *)ctx->pin;
    /* a file with an early verdict is never read on the device: only the
     * files that are hashed are packed */
    for (int f = 0; f < n; f++)
        if (ctx->splan.files[(size_t)f].frames)
            memcpy(pinb + off[(size_t)f], files[f], (size_t)file_sizes[f]);
    HIP_TRY(hipMemcpyAsync(ctx->dev_a, pinb, bytes, hipMemcpyHostToDevice,
                           ctx->stream));
    return scrub_run_locked(ctx, ctx->dev_a, file_status, first_bad);
}

/* ---- device memory + timing helpers ------------------------------------ */

mec_status mec_dev_alloc(mec_ctx *ctx, size_t bytes, void **out) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMalloc(out, bytes));
    return MEC_OK;
}

void mec_dev_free(mec_ctx *ctx, void *ptr) {
    (void)hipSetDevice(ctx->device);
    (void)hipFree(ptr);
}

mec_status mec_memcpy_h2d(mec_ctx *ctx, void *dst_dev, const void *src,
                          size_t bytes) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_memcpy_d2h(mec_ctx *ctx, void *dst, const void *src_dev,
                          size_t bytes) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_memset_dev(mec_ctx *ctx, void *dst_dev, int value,
                          size_t bytes) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_stream_sync(mec_ctx *ctx) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MEC_OK;
}

mec_status mec_timer_start(mec_ctx *ctx) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    return MEC_OK;
}

/* GPU-side streaming-format assembly for the full-block phase of
 * mec_encode_stream: upload packed object bytes once,
 * scatter to shard rows on device, fused encode+hash, interleave the
 * per-drive [hash||shard]* streams on device, copy one stream per drive
 * out.  Layout matches cmd/bitrot-streaming.go:57-75 bit-for-bit (pinned
 * by the stream round-trip tests). */
mec_status mec_encode_stream_gpu(mec_ctx *ctx, const uint8_t *src,
                                 int64_t n_full, int algo,
                                 uint8_t *const *drive_bufs,
                                 int64_t drive_off) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const int d = ctx->d, p = ctx->p, total = d + p;
    const int64_t bs = ctx->block_size, S = ctx->S, stride = ctx->stride;
    const int64_t pitch = 32 + S;
    const size_t src_bytes = (size_t)n_full * bs;
    const size_t row_bytes = (size_t)n_full * d * stride;
    const size_t par_bytes = (size_t)n_full * p * stride;
    const size_t sum_bytes = (size_t)n_full * total * 32;
    const size_t out_bytes = (size_t)total * n_full * pitch;
    /* shard rows live after the stream-out region; rows must keep the 64-B
     * base alignment the row kernels' uint4 accesses assume, and out_bytes
     * is odd whenever pitch (32+S) is (ragged S, e.g. EC12+4) */
    const size_t out_aligned = (out_bytes + 63) & ~(size_t)63;
    mec_status st;
    if ((st = ctx->ensure(&ctx->dev_a, &ctx->cap_a,
                          row_bytes > src_bytes ? row_bytes : src_bytes)) !=
        MEC_OK)
        return st;
    if ((st = ctx->ensure(&ctx->dev_b, &ctx->cap_b, par_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure(&ctx->dev_c, &ctx->cap_c, sum_bytes)) != MEC_OK)
        return st;
    if ((st = ctx->ensure(&ctx->dev_d, &ctx->cap_d,
                          out_aligned + row_bytes)) != MEC_OK)
        return st;
    /* dev_d holds [stream out | shard rows]; dev_a stages the packed src */
    uint8_t *dev_rows = (uint8_t *)ctx->dev_d + out_aligned;
    HIP_TRY(hipMemcpyAsync(ctx->dev_a, src, src_bytes, hipMemcpyHostToDevice,
                           ctx->stream));
    ScatterArgs sa{};
    sa.src = (const uint8_t *)ctx->dev_a;
    sa.rows = dev_rows;
    sa.block_len = bs;
    sa.S = S;
    sa.row_stride = stride;
    sa.n = n_full;
    sa.d = d;
    HIP_TRY(mec_launch_scatter_rows(&sa, ctx->stream));
    st = encode_dev_locked(ctx, (int)n_full, dev_rows, bs, ctx->dev_b, algo,
                           ctx->dev_c);
    if (st != MEC_OK) return st;
    InterleaveArgs ia{};
    ia.data = dev_rows;
    ia.parity = (const uint8_t *)ctx->dev_b;
    ia.sums = (const uint8_t *)ctx->dev_c;
    ia.out = (uint8_t *)ctx->dev_d;
    ia.S = S;
    ia.row_stride = stride;
    ia.n = n_full;
    ia.d = d;
    ia.p = p;
    HIP_TRY(mec_launch_stream_interleave(&ia, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < total; s++)
        HIP_TRY(hipMemcpy(drive_bufs[s] + drive_off,
                          (uint8_t *)ctx->dev_d + (int64_t)s * n_full * pitch,
                          (size_t)(n_full * pitch), hipMemcpyDeviceToHost));
    return MEC_OK;
}

mec_status mec_timer_stop(mec_ctx *ctx, float *ms_out) {
    if (!ctx) return MEC_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev_stop));
    HIP_TRY(hipEventElapsedTime(ms_out, ctx->ev_start, ctx->ev_stop));
    return MEC_OK;
}

} /* extern "C" */
