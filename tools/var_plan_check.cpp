/* Stand-alone check of the per-item-length encode planner
 * (minio_amd/csrc/var_plan.cpp): row offsets and column prefixes against a
 * brute-force recomputation, the hash order, the refusals, and the 32-bit
 * and column-count guards.  Host code only; meant to be built with
 * -fsanitize=address,undefined and run by tests/test_encode_var_cpu.py:
 *
 *   g++ -std=c++17 -fsanitize=address,undefined -I minio_amd/csrc \
 *       tools/var_plan_check.cpp minio_amd/csrc/var_plan.cpp \
 *       -o var_plan_check && ./var_plan_check
 *
 * Prints one line per check group and exits non-zero on the first failure.
 */
#include "var_plan.h"

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

/* S by counting, not by the planner's formula: the smallest S with
 * d*S >= len */
int64_t brute_shard(int64_t len, int d) {
    int64_t S = 0;
    while (S * d < len) S++;
    return S;
}

bool check_tables(int d, int p, int64_t block_size,
                  const std::vector<int64_t> &lens, const char *name) {
    const int64_t n = (int64_t)lens.size();
    mec::VarPlan pl;
    /* stale content must go */
    pl.items.assign(3, mec::VarItem{7, 7});
    pl.col_off.assign(9, 5);
    pl.order.assign(2, 1u);
    REQUIRE(mec::build_var_plan(d, d + p, block_size, n, lens.data(), &pl),
            "%s: refused", name);
    REQUIRE((int64_t)pl.items.size() == n && (int64_t)pl.col_off.size() == n + 1 &&
                (int64_t)pl.order.size() == n,
            "%s: table sizes", name);
    int64_t R = 0, C = 0, bytes = 0, shards = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t S = brute_shard(lens[i], d);
        int64_t stride = 0, cols = 0;
        while (stride < S) stride += 64;
        while (cols * 32 < S) cols++;
        REQUIRE(pl.items[i].row_off == R && pl.items[i].shard_len == S,
                "%s: item %lld is (%lld,%lld) want (%lld,%lld)", name,
                (long long)i, (long long)pl.items[i].row_off,
                (long long)pl.items[i].shard_len, (long long)R, (long long)S);
        REQUIRE(pl.col_off[i] == C, "%s: C[%lld] = %lld want %lld", name,
                (long long)i, (long long)pl.col_off[i], (long long)C);
        REQUIRE(R % 64 == 0 && cols >= 1 && cols * 32 <= stride,
                "%s: item %lld breaks the layout", name, (long long)i);
        R += stride;
        C += cols;
        bytes += lens[i];
        shards += S;
    }
    REQUIRE(pl.col_off[n] == C && pl.cols_total == C, "%s: C[n]", name);
    REQUIRE(pl.rows_total == R && pl.bytes_total == bytes &&
                pl.shards_total == shards,
            "%s: totals", name);
    /* the hash order: a permutation, descending S, stable */
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t k = 0; k < n; k++) {
        const uint32_t i = pl.order[k];
        REQUIRE(i < (uint64_t)n && !seen[i], "%s: order[%lld] = %u", name,
                (long long)k, i);
        seen[i] = 1;
        if (k) {
            const uint32_t h = pl.order[k - 1];
            const int64_t Sh = pl.items[h].shard_len, Si = pl.items[i].shard_len;
            REQUIRE(Sh > Si || (Sh == Si && h < i),
                    "%s: order[%lld..] = %u (S=%lld), %u (S=%lld)", name,
                    (long long)k - 1, h, (long long)Sh, i, (long long)Si);
        }
    }
    printf("tables %s: n=%lld rows=%lld cols=%lld ok\n", name, (long long)n,
           (long long)R, (long long)C);
    return true;
}

bool check_seeded() {
    const int geos[][2] = {{2, 2}, {8, 4}, {12, 4}, {16, 4}, {5, 2}};
    for (const auto &g : geos) {
        const int64_t bs = 1 << 20;
        Lcg rng{0x76617200ull + (uint64_t)g[0]};
        std::vector<int64_t> lens;
        for (int i = 0; i < 300; i++) {
            switch (rng.next() % 4) {
            case 0: lens.push_back(1 + rng.next() % 64); break;
            case 1: lens.push_back(1 + rng.next() % 4096); break;
            case 2: lens.push_back(1 + rng.next() % bs); break;
            default: lens.push_back(lens.empty() ? bs : lens.back()); break;
            }
        }
        lens.push_back(1);
        lens.push_back(bs);
        char name[32];
        snprintf(name, sizeof name, "ec%d+%d", g[0], g[1]);
        if (!check_tables(g[0], g[1], bs, lens, name)) return false;
    }
    /* one item; all equal (the order is the identity); ascending (the
     * order is the reverse) */
    if (!check_tables(8, 4, 1 << 20, {700001}, "single")) return false;
    if (!check_tables(8, 4, 1 << 20, std::vector<int64_t>(100, 4096), "equal"))
        return false;
    std::vector<int64_t> up;
    for (int i = 1; i <= 200; i++) up.push_back(8 * 32 * i);
    if (!check_tables(8, 4, 1 << 20, up, "ascending")) return false;
    return true;
}

bool check_refusals() {
    mec::VarPlan pl;
    const int64_t bs = 1 << 20;
    const int64_t ok[3] = {1, 4096, bs};
    REQUIRE(mec::build_var_plan(8, 12, bs, 3, ok, &pl), "valid lengths");
    for (int64_t bad : {(int64_t)0, (int64_t)-1, bs + 1, INT64_MAX, INT64_MIN}) {
        for (int at = 0; at < 3; at++) {
            int64_t lens[3] = {1, 4096, bs};
            lens[at] = bad;
            REQUIRE(!mec::build_var_plan(8, 12, bs, 3, lens, &pl),
                    "length %lld at %d accepted", (long long)bad, at);
        }
    }
    REQUIRE(!mec::build_var_plan(8, 12, bs, 0, ok, &pl), "n = 0");
    REQUIRE(!mec::build_var_plan(8, 12, bs, -1, ok, &pl), "n < 0");
    REQUIRE(!mec::build_var_plan(8, 12, bs, 3, nullptr, &pl), "null lengths");
    REQUIRE(!mec::build_var_plan(0, 4, bs, 3, ok, &pl), "d = 0");
    REQUIRE(!mec::build_var_plan(8, 7, bs, 3, ok, &pl), "total < d");
    REQUIRE(!mec::build_var_plan(8, 12, 0, 3, ok, &pl), "block_size = 0");
    printf("refusals: ok\n");
    return true;
}

bool check_guards() {
    mec::VarPlan pl;
    int64_t one = 1;
    /* n*total must be addressable by a 32-bit chain id; the planner must
     * refuse before it reads the lengths or allocates */
    REQUIRE(!mec::build_var_plan(8, 12, 64, 357913942, &one, &pl),
            "one past the largest n at 12 rows");
    REQUIRE(!mec::build_var_plan(1, 1, 64, 4294967296ll, &one, &pl),
            "2^32 chains");
    REQUIRE(!mec::build_var_plan(8, 12, 64, INT64_MAX, &one, &pl),
            "product overflow");
    /* column-count guard: 3 items of 2, 2 and 1 columns */
    const int64_t lens[3] = {8 * 33, 8 * 64, 8 * 32};
    REQUIRE(mec::build_var_plan(8, 12, 1 << 20, 3, lens, &pl, 5) &&
                pl.cols_total == 5,
            "5 columns fit in 5");
    REQUIRE(!mec::build_var_plan(8, 12, 1 << 20, 3, lens, &pl, 4),
            "5 columns accepted with room for 4");
    REQUIRE(!mec::build_var_plan(8, 12, 1 << 20, 3, lens, &pl, 0),
            "no room at all");
    /* buffer sizes: total*R_n must fit in int64 */
    const int64_t huge = INT64_MAX;
    const int64_t two[2] = {huge, huge};
    REQUIRE(!mec::build_var_plan(1, 2, huge, 2, two, &pl),
            "2 * 2^63 bytes of rows accepted");
    const int64_t big = INT64_MAX / 4;
    const int64_t bigs[2] = {big, big};
    REQUIRE(!mec::build_var_plan(1, 2, huge, 2, bigs, &pl),
            "2 rows * 2 items * 2^61 bytes accepted");
    printf("guards: ok\n");
    return true;
}

} // namespace

int main() {
    if (!check_seeded() || !check_refusals() || !check_guards()) return 1;
    printf("PASS\n");
    return 0;
}
