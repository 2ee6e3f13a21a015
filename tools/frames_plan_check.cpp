/* Stand-alone check of the planner of mec_encode_frames_batch_var*
 * (minio_amd/csrc/frames_plan.cpp) and of the granule mapping that
 * frames_pack_var_kernel shares with this program
 * (minio_amd/csrc/frames_map.h): the F prefix against a brute-force
 * recomputation, a refusal for each argument error, and an emulation of the
 * kernel on the CPU.  The emulation walks every granule of the output the
 * way the kernel's waves do (consecutive groups of 64, the wave state
 * carried from group to group and compared with a search from scratch),
 * takes each byte from random device images through the shared
 * mapping, and compares the result with a naive assembler that writes frame
 * after frame.  Every emulated load is asserted to lie inside the row stride
 * or the digest it belongs to, every store inside the output; the tables are
 * heap blocks of exactly their size, so the sanitizer sees a read past them.
 * Host code only; meant to be built with -fsanitize=address,undefined and
 * run by tests/test_encode_frames_cpu.py:
 *
 *   g++ -std=c++17 -fsanitize=address,undefined -I minio_amd/csrc \
 *       tools/frames_plan_check.cpp minio_amd/csrc/frames_plan.cpp \
 *       minio_amd/csrc/var_plan.cpp -o frames_plan_check && ./frames_plan_check
 *
 * Prints one line per check group and exits non-zero on the first failure.
 */
#include "frames_map.h"
#include "frames_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

#define REQUIRE(cond, ...)                                                   \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);  \
            fprintf(stderr, __VA_ARGS__);                                    \
            fprintf(stderr, "\n");                                           \
            return false;                                                    \
        }                                                                    \
    } while (0)

struct Lcg {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

constexpr int64_t kMiB = 1 << 20;
constexpr int kGuard = 64;
constexpr uint8_t kMark = 0xA5;

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

/* ---- the F prefix ------------------------------------------------------- */

bool check_offsets() {
    Lcg rng{0x6672616d};
    for (int d : {1, 2, 5, 8, 12, 16}) {
        std::vector<int64_t> lens;
        for (int i = 0; i < 400; i++) {
            const uint32_t r = rng.next();
            lens.push_back(r % 5 == 0   ? 1
                           : r % 5 == 1 ? kMiB
                           : r % 5 == 2 ? 1 + rng.next() % 300
                                        : 1 + rng.next() % kMiB);
        }
        const int n = (int)lens.size();
        std::vector<int64_t> got((size_t)n + 1, -1);
        REQUIRE(mec::frame_offsets(d, kMiB, n, lens.data(), got.data()),
                "d=%d refused", d);
        int64_t F = 0;
        for (int i = 0; i < n; i++) {
            REQUIRE(got[(size_t)i] == F, "d=%d F[%d]", d, i);
            F += 32 + ceil_div(lens[(size_t)i], d);
        }
        REQUIRE(got[(size_t)n] == F, "d=%d F[n]", d);

        mec::VarPlan vp;
        mec::FramesPlan fp;
        REQUIRE(mec::build_frames_plan(d, d + 4, kMiB, n, lens.data(), &vp,
                                       &fp),
                "d=%d plan refused", d);
        REQUIRE(fp.frame_off == got, "d=%d plan prefix", d);
        REQUIRE(fp.frames_bytes == (int64_t)(d + 4) * F, "d=%d bytes", d);
        REQUIRE(vp.items.size() == (size_t)n, "d=%d var plan", d);
    }
    printf("offsets: 6 geometries x 400 lengths ok\n");
    return true;
}

bool check_refusals() {
    const int64_t bs = 4096;
    const int64_t good[3] = {100, 4096, 1};
    int64_t out[4] = {-7, -7, -7, -7};
    auto untouched = [&] {
        for (int64_t v : out)
            if (v != -7) return false;
        return true;
    };
    REQUIRE(!mec::frame_offsets(8, bs, 0, good, out), "n = 0");
    REQUIRE(!mec::frame_offsets(8, bs, -3, good, out), "n < 0");
    REQUIRE(!mec::frame_offsets(0, bs, 3, good, out), "d = 0");
    REQUIRE(!mec::frame_offsets(8, 0, 3, good, out), "block_size = 0");
    REQUIRE(!mec::frame_offsets(8, bs, 3, nullptr, out), "lens null");
    REQUIRE(!mec::frame_offsets(8, bs, 3, good, nullptr), "out null");
    for (int pos = 0; pos < 3; pos++)
        for (int64_t bad : {(int64_t)0, (int64_t)-1, bs + 1, INT64_MIN}) {
            int64_t lens[3] = {good[0], good[1], good[2]};
            lens[pos] = bad;
            REQUIRE(!mec::frame_offsets(8, bs, 3, lens, out),
                    "length %lld at %d accepted", (long long)bad, pos);
            mec::VarPlan vp;
            mec::FramesPlan fp;
            REQUIRE(!mec::build_frames_plan(8, 12, bs, 3, lens, &vp, &fp),
                    "plan: length %lld at %d accepted", (long long)bad, pos);
        }
    REQUIRE(untouched(), "a refusal wrote frame_off");
    /* F_n past int64 */
    {
        const int64_t huge[2] = {INT64_MAX, INT64_MAX};
        REQUIRE(!mec::frame_offsets(1, INT64_MAX, 2, huge, out), "overflow");
        REQUIRE(untouched(), "the overflow refusal wrote frame_off");
    }
    /* n*(d+p) past 32 bits: refused before the lengths are read */
    {
        mec::VarPlan vp;
        mec::FramesPlan fp;
        REQUIRE(!mec::build_frames_plan(8, 12, bs, (int64_t)1 << 29, good,
                                        &vp, &fp),
                "chain ids past 32 bits accepted");
        REQUIRE(!mec::build_frames_plan(8, 12, bs, 0, good, &vp, &fp), "n=0");
        REQUIRE(!mec::build_frames_plan(8, 12, bs, 3, nullptr, &vp, &fp),
                "null lens");
    }
    REQUIRE(mec::frame_offsets(8, bs, 3, good, out), "good refused");
    REQUIRE(out[0] == 0 && out[1] == 32 + 13 && out[2] == 64 + 13 + 512 &&
                out[3] == 96 + 13 + 512 + 1,
            "good offsets");
    printf("refusals: ok\n");
    return true;
}

/* ---- the kernel, emulated ----------------------------------------------- */

struct Images {
    int d, p;
    mec::VarPlan vp;
    mec::FramesPlan fp;
    /* heap blocks of exactly the device sizes */
    std::vector<uint8_t> data, parity, sums;
    std::vector<int64_t> items; /* 2 per item, as the kernel reads them */
};

bool make_images(int d, int p, const std::vector<int64_t> &lens, uint64_t seed,
                 Images *im) {
    im->d = d;
    im->p = p;
    const int64_t n = (int64_t)lens.size();
    REQUIRE(mec::build_frames_plan(d, d + p, kMiB, n, lens.data(), &im->vp,
                                   &im->fp),
            "plan refused");
    Lcg rng{seed};
    /* random everywhere, the rows' [S, stride) included: no output byte may
     * come from there */
    im->data.resize((size_t)d * im->vp.rows_total);
    im->parity.resize((size_t)p * im->vp.rows_total);
    im->sums.resize((size_t)n * (d + p) * 32);
    for (auto *v : {&im->data, &im->parity, &im->sums})
        for (auto &b : *v) b = (uint8_t)rng.next();
    im->items.resize(2 * (size_t)n);
    for (int64_t i = 0; i < n; i++) {
        im->items[2 * (size_t)i] = im->vp.items[(size_t)i].row_off;
        im->items[2 * (size_t)i + 1] = im->vp.items[(size_t)i].shard_len;
    }
    return true;
}

/* frame after frame, straight from the layout's definition */
std::vector<uint8_t> naive(const Images &im) {
    const int d = im.d, p = im.p, total = d + p;
    const int64_t n = (int64_t)im.vp.items.size();
    const int64_t Fn = im.fp.frame_off[(size_t)n];
    std::vector<uint8_t> out((size_t)total * Fn);
    for (int s = 0; s < total; s++)
        for (int64_t i = 0; i < n; i++) {
            const int64_t R = im.vp.items[(size_t)i].row_off;
            const int64_t S = im.vp.items[(size_t)i].shard_len;
            const int64_t stride = (S + 63) & ~int64_t(63);
            uint8_t *f = out.data() + (int64_t)s * Fn + im.fp.frame_off[(size_t)i];
            memcpy(f, im.sums.data() + (i * total + s) * 32, 32);
            const uint8_t *row =
                s < d ? im.data.data() + (int64_t)d * R + s * stride
                      : im.parity.data() + (int64_t)p * R + (s - d) * stride;
            memcpy(f + 32, row, (size_t)S);
        }
    return out;
}

struct Counts {
    int64_t body = 0, boundary = 0, waves_one = 0, waves = 0, sheared = 0;
};

/* The kernel at frames address % 16 == a0, every wave taking per_wave_in
 * consecutive groups of 64 granules (0: one wave takes them all). */
bool emulate(const Images &im, uint32_t a0, int per_wave_in,
             const std::vector<uint8_t> &want, Counts *cn, const char *name) {
    const int64_t n = (int64_t)im.vp.items.size();
    const int64_t *F = im.fp.frame_off.data();
    mec::FmGeom g;
    g.fn = F[n];
    g.bytes = im.fp.frames_bytes;
    g.n = (uint32_t)n;
    g.d = (uint32_t)im.d;
    g.p = (uint32_t)im.p;
    g.a0 = a0;
    const int64_t G = mec::fm_granules(g);
    /* the 16-aligned memory around the output: granule q at mem + 16q, the
     * buffer at mem + a0 of a block with guards on both sides */
    std::vector<uint8_t> block((size_t)(kGuard + 16 * G + kGuard), kMark);
    std::vector<uint8_t> written((size_t)g.bytes, 0);
    uint8_t *mem = block.data() + kGuard;
    auto store = [&](int64_t q, int i, uint8_t v) {
        const int64_t o = 16 * q + i - (int64_t)a0;
        if (o < 0 || o >= g.bytes) return false;
        mem[16 * q + i] = v;
        written[(size_t)o]++;
        return true;
    };

    const int64_t groups = (G + mec::kFmWave - 1) / mec::kFmWave;
    const int64_t per_wave = per_wave_in > 0 ? per_wave_in : groups;
    for (int64_t grp0 = 0; grp0 < groups; grp0 += per_wave) {
        mec::FmWave w{};
        for (int64_t grp = grp0; grp < grp0 + per_wave && grp < groups;
             grp++) {
            const int64_t q0 = grp * mec::kFmWave;
            w = grp == grp0 ? mec::fm_wave_first(g, F, q0)
                            : mec::fm_wave_next(g, F, q0, w);
            /* whatever way the wave got here, it stands where a search
             * from scratch would put it */
            const mec::FmWave ref = mec::fm_wave_first(g, F, q0);
            REQUIRE(w.row == ref.row && w.first == ref.first &&
                        w.o0 == ref.o0 && w.r0 == ref.r0 && w.fs == ref.fs &&
                        w.fe == ref.fe && w.one == ref.one,
                    "%s: group %lld: carried state differs", name,
                    (long long)grp);
            cn->waves++;
            cn->waves_one += w.one;
            for (int64_t q = q0; q < q0 + mec::kFmWave && q < G; q++) {
                const mec::FmGran m = mec::fm_granule(g, F, w, q);
                REQUIRE(m.item < g.n && m.row < g.d + g.p,
                        "%s: granule %lld maps to frame (%u,%u)", name,
                        (long long)q, m.row, m.item);
                const int64_t R = im.items[2 * (size_t)m.item];
                const int64_t S = im.items[2 * (size_t)m.item + 1];
                REQUIRE(S == m.fe - m.fs - 32, "%s: S of item %u", name,
                        m.item);
                const int64_t row_lo = mec::fm_row_off(g, m.row, R, S);
                const int64_t stride = mec::fm_stride(S);
                const std::vector<uint8_t> &rowbuf =
                    m.row < g.d ? im.data : im.parity;
                REQUIRE(row_lo >= 0 &&
                            row_lo + stride <= (int64_t)rowbuf.size(),
                        "%s: row (%u,%u) outside its buffer", name, m.row,
                        m.item);
                if (m.body) {
                    cn->body++;
                    const mec::FmBody b = mec::fm_body(g, m, R);
                    cn->sheared += b.sh != 0;
                    uint32_t x[8], o[4];
                    for (int half = 0; half < 2; half++) {
                        const int64_t src = half ? b.src1 : b.src0;
                        REQUIRE(src % 16 == 0 && src >= row_lo &&
                                    src + 16 <= row_lo + stride,
                                "%s: granule %lld load %d at %lld leaves row "
                                "[%lld,+%lld)",
                                name, (long long)q, half, (long long)src,
                                (long long)row_lo, (long long)stride);
                        memcpy(x + 4 * half, rowbuf.data() + src, 16);
                    }
                    mec::fm_shear(x, b.sh, o);
                    uint8_t bytes[16];
                    memcpy(bytes, o, 16);
                    for (int i = 0; i < 16; i++)
                        REQUIRE(store(q, i, bytes[i]),
                                "%s: body granule %lld stores outside", name,
                                (long long)q);
                } else {
                    cn->boundary++;
                    const mec::FmBoundary b = mec::fm_boundary(g, m, R);
                    REQUIRE(b.edge >= 1, "%s: edge", name);
                    const int nb = m.hi_b - m.lo_b;
                    REQUIRE(nb >= 1 && nb <= 16, "%s: granule %lld is empty",
                            name, (long long)q);
                    for (int rel = 0; rel < nb; rel++) {
                        const mec::FmByte s = mec::fm_byte(b, rel);
                        uint8_t v;
                        if (s.where == mec::kFmSums) {
                            const int64_t lo = rel >= b.edge ? b.b_sum
                                                             : b.a_sum;
                            REQUIRE(s.off >= lo && s.off < lo + 32 &&
                                        lo + 32 <= (int64_t)im.sums.size(),
                                    "%s: digest byte at %lld", name,
                                    (long long)s.off);
                            v = im.sums[(size_t)s.off];
                        } else {
                            REQUIRE((s.where == mec::kFmParity) ==
                                        (m.row >= g.d),
                                    "%s: wrong row buffer", name);
                            REQUIRE(s.off >= row_lo && s.off < row_lo + S,
                                    "%s: shard byte at %lld outside "
                                    "[%lld,+%lld)",
                                    name, (long long)s.off, (long long)row_lo,
                                    (long long)S);
                            v = rowbuf[(size_t)s.off];
                        }
                        REQUIRE(store(q, m.lo_b + rel, v),
                                "%s: boundary granule %lld stores outside",
                                name, (long long)q);
                    }
                }
            }
        }
    }
    for (int64_t o = 0; o < g.bytes; o++)
        REQUIRE(written[(size_t)o] == 1, "%s: byte %lld written %d times",
                name, (long long)o, (int)written[(size_t)o]);
    REQUIRE(memcmp(mem + a0, want.data(), (size_t)g.bytes) == 0,
            "%s: a0=%u per_wave=%d: output differs from the naive assembler",
            name, a0, per_wave_in);
    for (int64_t i = 0; i < (int64_t)block.size(); i++) {
        const int64_t o = i - kGuard - (int64_t)a0;
        if (o < 0 || o >= g.bytes)
            REQUIRE(block[(size_t)i] == kMark, "%s: guard byte %lld", name,
                    (long long)o);
    }
    return true;
}

bool run_set(const char *name, int d, int p, const std::vector<int64_t> &lens,
             const std::vector<uint32_t> &phases, uint64_t seed) {
    Images im;
    if (!make_images(d, p, lens, seed, &im)) return false;
    const std::vector<uint8_t> want = naive(im);
    Counts cn;
    /* 0: one wave carries its state through every group; 1: none does */
    const int per_wave[4] = {0, 1, 3, 7};
    int k = 0;
    for (uint32_t a0 : phases)
        if (!emulate(im, a0, per_wave[k++ % 4], want, &cn, name))
            return false;
    printf("emulate %s: ec%d+%d n=%zu bytes=%lld phases=%zu body=%lld "
           "(sheared %lld) boundary=%lld one-frame waves=%lld/%lld ok\n",
           name, d, p, lens.size(), (long long)im.fp.frames_bytes,
           phases.size(), (long long)cn.body, (long long)cn.sheared,
           (long long)cn.boundary, (long long)cn.waves_one,
           (long long)cn.waves);
    return true;
}

bool check_emulation() {
    std::vector<uint32_t> all16;
    for (uint32_t a = 0; a < 16; a++) all16.push_back(a);
    Lcg rng{0x656d756c};

    /* one frame of 33 bytes: granule 0 is also the last */
    if (!run_set("single-33", 8, 4, {1}, all16, 1)) return false;
    /* 33-byte frames only, and fewer than 32 of them per row stream: a
     * wave spans many row streams */
    if (!run_set("rows-in-a-wave", 2, 2, {1, 2, 1}, all16, 2)) return false;
    {
        std::vector<int64_t> lens(700, 1);
        if (!run_set("all-33", 8, 4, lens, all16, 3)) return false;
    }
    {
        /* every S in 1..130: each frame size against each phase */
        std::vector<int64_t> lens;
        for (int S = 1; S <= 130; S++) lens.push_back(8 * S - (S % 7));
        if (!run_set("S-1..130", 8, 4, lens, all16, 4)) return false;
    }
    {
        /* S a multiple of 64: the last source window ends at the stride */
        std::vector<int64_t> lens = {8 * 64, 8 * 128, 8 * 64, 8 * 4096,
                                     8 * 192, 5};
        if (!run_set("S-mod-64", 8, 4, lens, all16, 5)) return false;
    }
    {
        /* a long frame behind short ones inside one wave's lookup, and the
         * ragged S = 87382 of EC12+4 */
        std::vector<int64_t> lens;
        for (int i = 0; i < 40; i++) lens.push_back(1 + rng.next() % 96);
        lens.push_back(kMiB);
        for (int i = 0; i < 40; i++) lens.push_back(1 + rng.next() % 96);
        if (!run_set("tiny-long-tiny", 12, 4, lens, {0, 1, 7, 8, 15}, 6))
            return false;
    }
    for (int geo = 0; geo < 4; geo++) {
        const int ds[4] = {2, 4, 12, 16}, ps[4] = {2, 2, 4, 4};
        std::vector<int64_t> lens;
        for (int i = 0; i < 60; i++) {
            const uint32_t r = rng.next() % 4;
            lens.push_back(r == 0   ? 1 + rng.next() % 64
                           : r == 1 ? 1 + rng.next() % 4096
                                    : 1 + rng.next() % 65536);
        }
        char name[32];
        snprintf(name, sizeof name, "random-%d", geo);
        if (!run_set(name, ds[geo], ps[geo], lens, {0, 3, 4, 9, 12, 13},
                     7 + (uint64_t)geo))
            return false;
    }
    return true;
}

} // namespace

int main() {
    if (!check_offsets() || !check_refusals() || !check_emulation()) return 1;
    printf("PASS\n");
    return 0;
}
