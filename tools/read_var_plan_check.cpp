/* Stand-alone check of the per-item-length verified-read planner
 * (minio_amd/csrc/read_var_plan.cpp): the ordered hash lists against
 * build_verify_list / build_rehash_list as sets and their order, the tile
 * prefixes against a brute-force recomputation, and the refusals.  Host
 * code only; meant to be built with -fsanitize=address,undefined and run by
 * tests/test_read_var_cpu.py:
 *
 *   g++ -std=c++17 -fsanitize=address,undefined -I minio_amd/csrc \
 *       tools/read_var_plan_check.cpp minio_amd/csrc/read_var_plan.cpp \
 *       minio_amd/csrc/var_plan.cpp minio_amd/csrc/recon_plan.cpp \
 *       minio_amd/csrc/verify_list.cpp minio_amd/csrc/gf_host.cpp \
 *       -o read_var_plan_check && ./read_var_plan_check
 *
 * Prints one line per check group and exits non-zero on the first failure.
 */
#include "gf_host.h"
#include "read_var_plan.h"
#include "recon_plan.h"
#include "var_plan.h"
#include "verify_list.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

/* An ordered list must hold the reference list's ids exactly once each,
 * grouped by item, the items in vp.order's sequence (so by descending S,
 * equal S by ascending index) and the rows of an item ascending. */
bool check_order(const mec::VarPlan &vp, int total,
                 const std::vector<uint32_t> &ordered,
                 std::vector<uint32_t> reference, const char *name) {
    std::vector<uint32_t> sorted = ordered;
    std::sort(sorted.begin(), sorted.end());
    std::sort(reference.begin(), reference.end());
    REQUIRE(sorted == reference, "%s: not the same set (%zu vs %zu ids)", name,
            sorted.size(), reference.size());
    std::vector<uint32_t> rank(vp.order.size());
    for (size_t k = 0; k < vp.order.size(); k++) rank[vp.order[k]] = (uint32_t)k;
    for (size_t k = 1; k < ordered.size(); k++) {
        const uint32_t a = ordered[k - 1], b = ordered[k];
        const uint32_t ia = a / (uint32_t)total, ib = b / (uint32_t)total;
        REQUIRE(rank[ia] < rank[ib] || (ia == ib && a < b),
                "%s: id %u before id %u", name, a, b);
        REQUIRE(vp.items[ia].shard_len >= vp.items[ib].shard_len,
                "%s: S grows from id %u to id %u", name, a, b);
    }
    return true;
}

/* tiles by counting, not by the planner's formula: 2 KiB steps of a row */
int64_t brute_tiles(int64_t S) {
    int64_t t = 0;
    for (int64_t b = 0; b < S; b += 2048) t++;
    return t;
}

bool check_geometry(int d, int p, int n, uint64_t seed, int max_missing,
                    const char *name) {
    const int total = d + p;
    const int64_t bs = 1 << 20;
    Lcg rng{seed};
    std::vector<int64_t> lens((size_t)n);
    for (auto &len : lens) {
        switch (rng.next() % 5) {
        case 0: len = 1 + rng.next() % 64; break;
        case 1: len = 1 + rng.next() % 4096; break;
        case 2: len = 1 + rng.next() % bs; break;
        /* shard lengths on each side of a tile boundary */
        case 3: len = (int64_t)d * (2048 * (1 + rng.next() % 3) +
                                    (int64_t)(rng.next() % 3) - 1); break;
        default: len = bs; break;
        }
        if (len > bs) len = bs;
    }
    mec::VarPlan vp;
    REQUIRE(mec::build_var_plan(d, total, bs, n, lens.data(), &vp),
            "%s: var plan refused", name);

    /* read masks: all rows, a few missing, or too few */
    std::vector<uint8_t> read((size_t)n * total, 1), ok((size_t)n * total, 1);
    for (int i = 0; i < n; i++) {
        const int miss = (int)(rng.next() % (uint32_t)(max_missing + 1));
        for (int m = 0; m < miss; m++)
            read[(size_t)i * total + rng.next() % total] = 0;
        if (rng.next() % 9 == 0) ok[(size_t)i * total + rng.next() % total] = 0;
        if (i % 37 == 5) /* unrecoverable */
            for (int s = 0; s <= p; s++) read[(size_t)i * total + s] = 0;
        if (i % 41 == 7) /* nothing read at all */
            for (int s = 0; s < total; s++) read[(size_t)i * total + s] = 0;
    }
    std::vector<uint32_t> ref, got;
    REQUIRE(mec::build_verify_list(n, total, read.data(), &ref),
            "%s: reference verify list", name);
    got.assign(5, 99u); /* stale content must go */
    mec::build_verify_list_ordered(vp, total, read.data(), &got);
    if (!check_order(vp, total, got, ref, name)) return false;
    const size_t n_verify = got.size();

    std::vector<uint8_t> enc((size_t)total * d);
    REQUIRE(mec::build_encode_matrix(d, p, enc.data()), "%s: matrix", name);
    std::vector<uint8_t> present((size_t)n * total);
    mec::merge_verified((uint32_t)(n * total), read.data(), ok.data(),
                        present.data());
    size_t n_rehash[2] = {0, 0};
    int64_t tiles_sum[2] = {0, 0};
    int too_few = 0;
    for (int data_only = 0; data_only < 2; data_only++) {
        mec::ReconPlan pl;
        REQUIRE(mec::build_reconstruct_plan(enc.data(), d, p, n,
                                            present.data(), data_only, &pl),
                "%s: plan", name);
        too_few = pl.n_too_few;
        mec::build_rehash_list(pl, d, p, n, present.data(), data_only, &ref);
        got.assign(3, 7u);
        mec::build_rehash_list_ordered(vp, pl, d, p, present.data(),
                                       data_only, &got);
        if (!check_order(vp, total, got, ref, name)) return false;
        n_rehash[data_only] = got.size();

        for (int e = 1; e <= mec::kPlanMaxE; e++) {
            std::vector<int64_t> T(2, -5); /* stale content must go */
            REQUIRE(mec::build_tile_prefix(vp, pl.work[e], &T),
                    "%s: prefix E=%d refused", name, e);
            REQUIRE(T.size() == pl.work[e].size() + 1, "%s: prefix size", name);
            int64_t want = 0;
            for (size_t w = 0; w < pl.work[e].size(); w++) {
                REQUIRE(T[w] == want, "%s: E=%d T[%zu] = %lld want %lld", name,
                        e, w, (long long)T[w], (long long)want);
                const int64_t S = vp.items[pl.work[e][w].item].shard_len;
                REQUIRE(brute_tiles(S) == mec::read_var_tiles(S),
                        "%s: tiles of S=%lld", name, (long long)S);
                /* the last tile of the pair holds a live column, and no
                 * column is past the row's stride */
                const int64_t cols = (S + 31) / 32, t = brute_tiles(S);
                REQUIRE((t - 1) * 64 < cols && cols <= t * 64 &&
                            cols * 32 <= ((S + 63) & ~int64_t(63)),
                        "%s: tile cover of S=%lld", name, (long long)S);
                want += t;
            }
            REQUIRE(T.back() == want, "%s: E=%d T[m]", name, e);
            tiles_sum[data_only] += want;
            /* the bound: exactly fitting passes, one less is refused */
            if (want > 0) {
                REQUIRE(mec::build_tile_prefix(vp, pl.work[e], &T, want),
                        "%s: %lld tiles fit in %lld", name, (long long)want,
                        (long long)want);
                REQUIRE(!mec::build_tile_prefix(vp, pl.work[e], &T, want - 1),
                        "%s: %lld tiles accepted with room for %lld", name,
                        (long long)want, (long long)want - 1);
            }
        }
    }
    printf("lists+tiles %s: n=%d verify=%zu rehash=%zu/%zu tiles=%lld/%lld "
           "too_few=%d ok\n",
           name, n, n_verify, n_rehash[0], n_rehash[1],
           (long long)tiles_sum[0], (long long)tiles_sum[1], too_few);
    return true;
}

bool check_seeded() {
    if (!check_geometry(8, 4, 300, 0x72766172ull, 3, "ec8+4")) return false;
    if (!check_geometry(2, 1, 500, 0x72766173ull, 1, "ec2+1")) return false;
    /* more than kPlanMaxE rebuilt rows: two entries per pattern */
    if (!check_geometry(4, 10, 120, 0x72766174ull, 10, "ec4+10")) return false;
    if (!check_geometry(12, 4, 200, 0x72766175ull, 4, "ec12+4")) return false;
    return true;
}

/* hand-made case: lengths, order and prefix written out */
bool check_small() {
    const int d = 2, total = 3;
    /* S = 1, 2049, 64, 2049, 4096 */
    const int64_t lens[5] = {1, 2 * 2049, 128, 2 * 2049 - 1, 8192};
    mec::VarPlan vp;
    REQUIRE(mec::build_var_plan(d, total, 1 << 20, 5, lens, &vp), "small plan");
    const uint32_t want_order[5] = {4, 1, 3, 2, 0};
    for (int k = 0; k < 5; k++)
        REQUIRE(vp.order[k] == want_order[k], "order[%d] = %u", k, vp.order[k]);
    const uint8_t read[15] = {1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0};
    std::vector<uint32_t> got;
    mec::build_verify_list_ordered(vp, total, read, &got);
    const std::vector<uint32_t> want = {12, 13, 3, 4, 5, 10, 11, 0, 2};
    REQUIRE(got == want, "small verify list has %zu ids", got.size());
    const std::vector<mec::ReconWork> work = {{0, 0}, {3, 1}, {4, 1}, {2, 0}};
    std::vector<int64_t> T;
    REQUIRE(mec::build_tile_prefix(vp, work, &T), "small prefix");
    const std::vector<int64_t> want_T = {0, 1, 3, 5, 6};
    REQUIRE(T == want_T, "small prefix ends at %lld", (long long)T.back());
    std::vector<mec::ReconWork> none;
    REQUIRE(mec::build_tile_prefix(vp, none, &T) && T.size() == 1 && T[0] == 0,
            "empty work list");
    printf("small: ok\n");
    return true;
}

bool check_refusals() {
    const int64_t lens[2] = {64, 1 << 20};
    mec::VarPlan vp;
    REQUIRE(mec::build_var_plan(8, 12, 1 << 20, 2, lens, &vp), "plan");
    std::vector<int64_t> T;
    const std::vector<mec::ReconWork> bad = {{0, 0}, {2, 0}};
    REQUIRE(!mec::build_tile_prefix(vp, bad, &T), "item 2 of 2 accepted");
    const std::vector<mec::ReconWork> two = {{1, 0}, {1, 1}};
    REQUIRE(mec::build_tile_prefix(vp, two, &T, 128) && T.back() == 128,
            "2 x 64 tiles fit in 128");
    REQUIRE(!mec::build_tile_prefix(vp, two, &T, 127), "128 tiles in 127");
    REQUIRE(!mec::build_tile_prefix(vp, two, &T, 0), "no room at all");
    REQUIRE(!mec::build_tile_prefix(vp, two, &T, -1), "negative bound");
    REQUIRE(mec::kReadVarMaxTiles <= INT64_MAX / 2048,
            "a tile's byte offset must fit in int64");
    printf("refusals: ok\n");
    return true;
}

} // namespace

int main() {
    if (!check_small() || !check_seeded() || !check_refusals()) return 1;
    printf("PASS\n");
    return 0;
}
