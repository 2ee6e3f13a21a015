/* Stand-alone check of the batch-scrub planner
 * (minio_amd/csrc/scrub_plan.cpp): every frame of every size-consistent
 * file in exactly one chain list, split by its address modulo 8; the
 * descending-length order with stable ties; the early verdicts; the
 * reduction back to one status and the lowest failing frame per file; the
 * offsets helper; and a refusal for each argument error.  Host code only;
 * meant to be built with -fsanitize=address,undefined and run by
 * tests/test_scrub_cpu.py:
 *
 *   g++ -std=c++17 -fsanitize=address,undefined -I minio_amd/csrc \
 *       tools/scrub_plan_check.cpp minio_amd/csrc/scrub_plan.cpp \
 *       -o scrub_plan_check && ./scrub_plan_check
 *
 * Prints one line per check group and exits non-zero on the first failure.
 */
#include "scrub_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
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

/* the four tables of one call */
struct Batch {
    std::vector<int64_t> off, size, part, shard;
    int64_t bytes = 0;
    int n() const { return (int)off.size(); }
    /* append a file at `gap` bytes behind the previous one; delta is added
     * to the size the part and shard sizes call for */
    void add(int64_t gap, int64_t part_, int64_t shard_, int64_t delta = 0) {
        int64_t want = mec::scrub_shard_file_size(part_, shard_) + delta;
        if (want < 0) want = 0;
        off.push_back(bytes + gap);
        size.push_back(want);
        part.push_back(part_);
        shard.push_back(shard_);
        bytes += gap + want;
    }
};

bool plan(const Batch &b, unsigned base_mod8, mec::ScrubPlan *pl,
          uint64_t max_frames = mec::kScrubMaxFrames) {
    return mec::build_scrub_plan(b.n(), b.off.data(), b.size.data(),
                                 b.part.data(), b.shard.data(), b.bytes,
                                 base_mod8, pl, max_frames);
}

/* Brute force: the frames each file should contribute and their lengths,
 * the list each belongs to by its own address arithmetic, and the order. */
bool check_plan(const Batch &b, unsigned base_mod8, const mec::ScrubPlan &pl,
                const char *name, size_t *n_aligned, size_t *n_sheared) {
    const int n = b.n();
    REQUIRE(pl.files.size() == (size_t)n && pl.early.size() == (size_t)n,
            "%s: table sizes", name);
    /* (file, frame) -> 0 aligned, 1 sheared */
    std::map<std::pair<uint32_t, uint32_t>, int> want;
    std::map<std::pair<uint32_t, uint32_t>, int64_t> want_len;
    for (int f = 0; f < n; f++) {
        const int64_t S = b.shard[f], part = b.part[f];
        const int64_t frames = (part + S - 1) / S;
        const bool size_ok = b.size[f] == frames * 32 + part;
        const mec::ScrubFile &sf = pl.files[(size_t)f];
        if (!size_ok) {
            REQUIRE(pl.early[(size_t)f] == mec::kScrubBadSize && !sf.frames,
                    "%s: file %d not refused for its size", name, f);
            continue;
        }
        if (part == 0) {
            REQUIRE(pl.early[(size_t)f] == mec::kScrubEmpty && !sf.frames,
                    "%s: empty file %d", name, f);
            continue;
        }
        REQUIRE(pl.early[(size_t)f] == mec::kScrubHashed, "%s: file %d early",
                name, f);
        REQUIRE(sf.off == b.off[f] && sf.shard == S &&
                    sf.frames == (uint32_t)frames &&
                    sf.last == part - (frames - 1) * S,
                "%s: table row %d", name, f);
        for (int64_t k = 0; k < frames; k++) {
            const int64_t addr = (int64_t)base_mod8 + b.off[f] + k * (32 + S);
            const auto key = std::make_pair((uint32_t)f, (uint32_t)k);
            want[key] = (addr + 32) % 8 != 0;
            want_len[key] = k == frames - 1 ? part - k * S : S;
            /* the frame lies inside the file */
            REQUIRE(k * (32 + S) + 32 + want_len[key] <= b.size[f],
                    "%s: frame %d/%lld outside its file", name, f,
                    (long long)k);
        }
    }
    size_t seen = 0;
    int which = 0;
    for (const std::vector<mec::ScrubChain> *list :
         {&pl.aligned, &pl.sheared}) {
        for (size_t i = 0; i < list->size(); i++) {
            const auto key =
                std::make_pair((*list)[i].file, (*list)[i].frame);
            const auto it = want.find(key);
            REQUIRE(it != want.end(), "%s: chain (%u,%u) not wanted or twice",
                    name, key.first, key.second);
            REQUIRE(it->second == which, "%s: chain (%u,%u) in list %d", name,
                    key.first, key.second, which);
            want.erase(it);
            seen++;
            if (i == 0) continue;
            const auto prev =
                std::make_pair((*list)[i - 1].file, (*list)[i - 1].frame);
            const int64_t lp = want_len[prev], lc = want_len[key];
            REQUIRE(lp > lc || (lp == lc && prev < key),
                    "%s: order at %zu of list %d", name, i, which);
        }
        which++;
    }
    REQUIRE(want.empty(), "%s: %zu frames in no list", name, want.size());
    *n_aligned = pl.aligned.size();
    *n_sheared = pl.sheared.size();
    return seen == *n_aligned + *n_sheared;
}

/* ok bytes in list order from a set of bad (file, frame) pairs */
std::vector<uint8_t> ok_bytes(
    const mec::ScrubPlan &pl,
    const std::vector<std::pair<uint32_t, uint32_t>> &bad) {
    std::vector<uint8_t> ok;
    for (const std::vector<mec::ScrubChain> *list :
         {&pl.aligned, &pl.sheared})
        for (const mec::ScrubChain &c : *list) {
            uint8_t good = 1;
            for (const auto &b : bad)
                if (b.first == c.file && b.second == c.frame) good = 0;
            ok.push_back(good);
        }
    return ok;
}

bool test_small() {
    Batch b;
    b.add(0, 100, 32);      /* 0: frames 32,32,32,4; pitch 64: all aligned */
    b.add(3, 70, 33);       /* 1: off 231; frames 33,33,4; pitch 65 */
    b.add(0, 0, 16);        /* 2: empty */
    b.add(1, 64, 16, +1);   /* 3: one byte too long */
    b.add(0, 5, 16, -1);    /* 4: one byte short */
    b.add(5, 10, 64);       /* 5: one short frame */
    mec::ScrubPlan pl;
    REQUIRE(plan(b, 0, &pl), "small plan refused");
    size_t na, ns;
    if (!check_plan(b, 0, pl, "small", &na, &ns)) return false;
    REQUIRE(na + ns == 4 + 3 + 1, "small: %zu chains", na + ns);
    REQUIRE(pl.aligned.size() >= 4, "small: file 0 is aligned throughout");
    /* the same files behind a buffer at address 5 mod 8 */
    mec::ScrubPlan pl5;
    REQUIRE(plan(b, 5, &pl5), "small plan at base 5 refused");
    if (!check_plan(b, 5, pl5, "small@5", &na, &ns)) return false;

    /* reduction: nothing bad */
    std::vector<uint8_t> corrupt(6, 9);
    std::vector<int64_t> fb(6, 77);
    std::vector<uint8_t> ok = ok_bytes(pl, {});
    mec::reduce_scrub(pl, ok.data(), corrupt.data(), fb.data());
    const uint8_t want0[6] = {0, 0, 0, 1, 1, 0};
    for (int f = 0; f < 6; f++)
        REQUIRE(corrupt[f] == want0[f] && fb[f] == -1,
                "small: clean reduce, file %d: %d %lld", f, corrupt[f],
                (long long)fb[f]);
    /* two bad frames in one file give the lower index, whatever the list
     * order; a bad last frame; the neighbours stay clean */
    ok = ok_bytes(pl, {{0, 3}, {0, 1}, {1, 2}});
    mec::reduce_scrub(pl, ok.data(), corrupt.data(), fb.data());
    const uint8_t want1[6] = {1, 1, 0, 1, 1, 0};
    const int64_t fb1[6] = {1, 2, -1, -1, -1, -1};
    for (int f = 0; f < 6; f++)
        REQUIRE(corrupt[f] == want1[f] && fb[f] == fb1[f],
                "small: reduce, file %d: %d %lld", f, corrupt[f],
                (long long)fb[f]);
    /* first_bad may be NULL */
    std::vector<uint8_t> corrupt2(6, 9);
    mec::reduce_scrub(pl, ok.data(), corrupt2.data(), nullptr);
    REQUIRE(corrupt2 == corrupt, "small: reduce without first_bad");
    printf("small: ok\n");
    return true;
}

bool test_random(uint64_t seed, int n, const char *name) {
    Lcg r{seed};
    static const int64_t shards[] = {1, 7, 31, 32, 33, 87382, 131072, 1000};
    Batch b;
    for (int f = 0; f < n; f++) {
        const int64_t S = shards[r.next() % 8];
        int64_t part = S <= 33 ? r.next() % 200 : r.next() % (3 * S + 2);
        if (r.next() % 11 == 0) part = (1 + r.next() % 3) * S; /* exact */
        const int64_t delta = r.next() % 13 == 0 ? (r.next() % 2 ? 1 : -1) : 0;
        b.add(r.next() % 9, part, S, delta);
    }
    const unsigned base = r.next() % 8;
    mec::ScrubPlan pl;
    REQUIRE(plan(b, base, &pl), "%s: plan refused", name);
    size_t na, ns;
    if (!check_plan(b, base, pl, name, &na, &ns)) return false;

    /* reduction against a direct count, with a tenth of the chains bad */
    std::vector<uint8_t> ok(na + ns, 1);
    std::vector<int64_t> want_fb((size_t)n, -1);
    std::vector<uint8_t> want_c((size_t)n, 0);
    for (int f = 0; f < n; f++)
        want_c[(size_t)f] = pl.early[(size_t)f] == mec::kScrubBadSize;
    size_t slot = 0, n_bad = 0;
    for (const std::vector<mec::ScrubChain> *list :
         {&pl.aligned, &pl.sheared})
        for (const mec::ScrubChain &c : *list) {
            if (r.next() % 10 == 0) {
                ok[slot] = 0;
                n_bad++;
                want_c[c.file] = 1;
                if (want_fb[c.file] < 0 || c.frame < want_fb[c.file])
                    want_fb[c.file] = c.frame;
            }
            slot++;
        }
    std::vector<uint8_t> corrupt((size_t)n, 9);
    std::vector<int64_t> fb((size_t)n, 77);
    mec::reduce_scrub(pl, ok.data(), corrupt.data(), fb.data());
    REQUIRE(corrupt == want_c && fb == want_fb, "%s: reduce", name);
    printf("%s: n=%d aligned=%zu sheared=%zu bad=%zu ok\n", name, n, na, ns,
           n_bad);
    return true;
}

bool test_offsets() {
    const int64_t sizes[5] = {0, 1, 64, 65, 87414};
    int64_t off[6];
    REQUIRE(mec::scrub_file_offsets(5, sizes, off), "offsets refused");
    const int64_t want[6] = {0, 0, 64, 128, 256, 256 + 87424};
    for (int i = 0; i < 6; i++)
        REQUIRE(off[i] == want[i], "offset %d = %lld", i, (long long)off[i]);
    REQUIRE(!mec::scrub_file_offsets(0, sizes, off), "n = 0 accepted");
    REQUIRE(!mec::scrub_file_offsets(5, nullptr, off), "NULL sizes accepted");
    REQUIRE(!mec::scrub_file_offsets(5, sizes, nullptr), "NULL out accepted");
    const int64_t neg[2] = {5, -1};
    REQUIRE(!mec::scrub_file_offsets(2, neg, off), "negative size accepted");
    const int64_t huge[2] = {INT64_MAX - 100, INT64_MAX - 100};
    off[0] = 123;
    REQUIRE(!mec::scrub_file_offsets(2, huge, off) && off[0] == 123,
            "offsets past int64 accepted");
    REQUIRE(mec::scrub_shard_file_size(0, 5) == 0 &&
                mec::scrub_shard_file_size(10, 5) == 74 &&
                mec::scrub_shard_file_size(11, 5) == 107 &&
                mec::scrub_shard_file_size(INT64_MAX, 1) == -1,
            "shard file size");
    printf("offsets: ok\n");
    return true;
}

bool test_refusals() {
    mec::ScrubPlan pl;
    Batch good;
    good.add(0, 100, 32);
    good.add(1, 70, 33);
    REQUIRE(plan(good, 0, &pl), "good batch refused");
#define REFUSED(batch, what)                                                 \
    REQUIRE(!plan(batch, 0, &pl), "accepted: %s", what)
    REQUIRE(!mec::build_scrub_plan(0, good.off.data(), good.size.data(),
                                   good.part.data(), good.shard.data(),
                                   good.bytes, 0, &pl),
            "accepted: n = 0");
    REQUIRE(!mec::build_scrub_plan(-3, good.off.data(), good.size.data(),
                                   good.part.data(), good.shard.data(),
                                   good.bytes, 0, &pl),
            "accepted: n < 0");
    REQUIRE(!mec::build_scrub_plan(2, nullptr, good.size.data(),
                                   good.part.data(), good.shard.data(),
                                   good.bytes, 0, &pl),
            "accepted: NULL file_off");
    REQUIRE(!mec::build_scrub_plan(2, good.off.data(), nullptr,
                                   good.part.data(), good.shard.data(),
                                   good.bytes, 0, &pl),
            "accepted: NULL file_sizes");
    REQUIRE(!mec::build_scrub_plan(2, good.off.data(), good.size.data(),
                                   nullptr, good.shard.data(), good.bytes, 0,
                                   &pl),
            "accepted: NULL part_sizes");
    REQUIRE(!mec::build_scrub_plan(2, good.off.data(), good.size.data(),
                                   good.part.data(), nullptr, good.bytes, 0,
                                   &pl),
            "accepted: NULL shard_sizes");
    Batch b = good;
    b.size[1] = -1;
    REFUSED(b, "negative file size");
    b = good;
    b.part[0] = -1;
    REFUSED(b, "negative part size");
    b = good;
    b.shard[1] = 0;
    REFUSED(b, "shard size 0");
    b = good;
    b.shard[0] = -4;
    REFUSED(b, "negative shard size");
    b = good;
    b.off[0] = -1;
    REFUSED(b, "negative offset");
    b = good;
    b.bytes -= 1;
    REFUSED(b, "last file one byte past the buffer");
    b = good;
    b.off[0] = INT64_MAX - 3;
    REFUSED(b, "offset + size past int64");
    b = good;
    b.bytes = -1;
    REFUSED(b, "negative buffer size");
#undef REFUSED
    /* the frame bound through an injected limit: 4 + 3 frames to hash */
    REQUIRE(plan(good, 0, &pl, 7), "7 frames refused at limit 7");
    REQUIRE(!plan(good, 0, &pl, 6), "7 frames accepted at limit 6");
    /* a file refused for its size brings no frames to the count */
    b = good;
    b.add(0, 1000, 10, +1);
    REQUIRE(plan(b, 0, &pl, 7), "size-refused file counted");
    /* a part size whose file size passes int64 is a size mismatch, not an
     * overflow */
    b = good;
    b.add(0, 0, 1);
    b.part[2] = INT64_MAX;
    REQUIRE(plan(b, 0, &pl) && pl.early[2] == mec::kScrubBadSize,
            "huge part size");
    printf("refusals: ok\n");
    return true;
}

} // namespace

int main() {
    if (!test_small()) return 1;
    if (!test_offsets()) return 1;
    if (!test_random(1, 400, "random a")) return 1;
    if (!test_random(0x5eed, 1500, "random b")) return 1;
    if (!test_random(77, 1, "random c")) return 1;
    if (!test_refusals()) return 1;
    printf("PASS\n");
    return 0;
}
