/* Stand-alone check of the verified-read list builder
 * (minio_amd/csrc/verify_list.cpp): the verify list, the read & ok merge,
 * the rehash list taken from a finished reconstruct plan, and the 32-bit
 * chain-id guard.  Host code only; meant to be built with
 * -fsanitize=address,undefined and run by tests/test_verified_read_cpu.py:
 *
 *   g++ -std=c++17 -fsanitize=address,undefined -I minio_amd/csrc \
 *       tools/verify_list_check.cpp minio_amd/csrc/verify_list.cpp \
 *       minio_amd/csrc/recon_plan.cpp minio_amd/csrc/gf_host.cpp \
 *       -o verify_list_check && ./verify_list_check
 *
 * Prints one line per check group and exits non-zero on the first failure.
 */
#include "gf_host.h"
#include "recon_plan.h"
#include "verify_list.h"

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

/* the verify list is exactly the set bits of read_mask, in order */
bool check_verify_list() {
    const int total = 12;
    for (int n : {0, 1, 5, 1000}) {
        Lcg rng{0x76657269ull + (uint64_t)n};
        std::vector<uint8_t> mask((size_t)n * total);
        /* any non-zero byte counts as read */
        for (auto &m : mask) m = (rng.next() % 3) ? (uint8_t)(1 + rng.next() % 255) : 0;
        std::vector<uint32_t> list(7, 99u); /* stale content must go */
        REQUIRE(mec::build_verify_list(n, total, mask.data(), &list),
                "n=%d refused", n);
        size_t k = 0;
        for (uint32_t c = 0; c < (uint32_t)mask.size(); c++)
            if (mask[c]) {
                REQUIRE(k < list.size() && list[k] == c,
                        "n=%d: entry %zu is not chain %u", n, k, c);
                k++;
            }
        REQUIRE(k == list.size(), "n=%d: %zu listed, %zu read", n,
                list.size(), k);
    }
    /* nothing read, everything read */
    std::vector<uint8_t> none(36, 0), all(36, 1);
    std::vector<uint32_t> list;
    REQUIRE(mec::build_verify_list(3, total, none.data(), &list) &&
                list.empty(),
            "empty mask");
    REQUIRE(mec::build_verify_list(3, total, all.data(), &list) &&
                list.size() == 36 && list[0] == 0 && list[35] == 35,
            "full mask");
    printf("verify list: ok\n");
    return true;
}

/* present = read & ok, as 0/1 bytes, whatever the non-zero values */
bool check_merge() {
    const uint8_t read[8] = {0, 0, 1, 1, 7, 255, 0, 3};
    const uint8_t ok[8] = {0, 1, 0, 1, 1, 9, 200, 0};
    const uint8_t want[8] = {0, 0, 0, 1, 1, 1, 0, 0};
    uint8_t got[8];
    for (auto &g : got) g = 0xee;
    mec::merge_verified(8, read, ok, got);
    for (int i = 0; i < 8; i++)
        REQUIRE(got[i] == want[i], "slot %d: %d want %d", i, got[i], want[i]);
    mec::merge_verified(0, read, ok, got); /* count 0 touches nothing */
    printf("merge: ok\n");
    return true;
}

/* rehash list = the rows build_reconstruct_plan's kernels rebuild */
bool check_rehash(int d, int p, const std::vector<std::vector<int>> &gone,
                  const char *name) {
    const int total = d + p;
    const int n = (int)gone.size();
    std::vector<uint8_t> enc((size_t)total * d);
    REQUIRE(mec::build_encode_matrix(d, p, enc.data()), "%s: matrix", name);
    std::vector<uint8_t> present((size_t)n * total, 1);
    for (int i = 0; i < n; i++)
        for (int s : gone[i]) present[(size_t)i * total + s] = 0;
    for (int data_only = 0; data_only <= 1; data_only++) {
        mec::ReconPlan pl;
        REQUIRE(mec::build_reconstruct_plan(enc.data(), d, p, n,
                                            present.data(), data_only, &pl),
                "%s: plan refused", name);
        std::vector<uint32_t> list(3, 5u);
        mec::build_rehash_list(pl, d, p, n, present.data(), data_only, &list);
        /* expected, from the plan's own work lists: every destination row
         * of every (item, entry) pair */
        std::vector<uint8_t> rebuilt((size_t)n * total, 0);
        size_t n_rebuilt = 0;
        for (int e = 1; e <= mec::kPlanMaxE; e++)
            for (const mec::ReconWork &wk : pl.work[e]) {
                const mec::ReconPlanEntry &ent = pl.entries[wk.entry];
                for (uint32_t t = 0; t < ent.n_dst; t++) {
                    const size_t c = (size_t)wk.item * total + ent.dst_rows[t];
                    REQUIRE(!rebuilt[c], "%s: row rebuilt twice", name);
                    rebuilt[c] = 1;
                    n_rebuilt++;
                }
            }
        REQUIRE(list.size() == n_rebuilt, "%s data_only=%d: %zu listed, %zu "
                "rebuilt", name, data_only, list.size(), n_rebuilt);
        for (size_t k = 0; k < list.size(); k++) {
            REQUIRE(list[k] < rebuilt.size() && rebuilt[list[k]],
                    "%s: chain %u listed but not rebuilt", name, list[k]);
            REQUIRE(k == 0 || list[k - 1] < list[k], "%s: not ascending",
                    name);
            const int i = (int)(list[k] / total), s = (int)(list[k] % total);
            REQUIRE(pl.status[i] == mec::kPlanOk, "%s: TOO_FEW item %d listed",
                    name, i);
            REQUIRE(!present[list[k]], "%s: present row listed", name);
            REQUIRE(!data_only || s < d, "%s: parity row under data_only",
                    name);
        }
        /* a TOO_FEW item contributes nothing, though its rows are missing */
        for (int i = 0; i < n; i++)
            if ((int)gone[i].size() > p)
                REQUIRE(pl.status[i] == mec::kPlanTooFew, "%s: item %d", name,
                        i);
        printf("rehash list %s data_only=%d: %zu rows, too_few=%d ok\n", name,
               data_only, list.size(), pl.n_too_few);
    }
    return true;
}

/* n*total must be addressable by a 32-bit chain id */
bool check_guard() {
    uint32_t c = 0;
    REQUIRE(mec::verify_chain_count(0, 12, &c) && c == 0, "n=0");
    REQUIRE(mec::verify_chain_count(70000, 3, &c) && c == 210000u, "70000x3");
    REQUIRE(mec::verify_chain_count(357913941, 12, &c) && c == 4294967292u,
            "largest n at 12 rows");
    REQUIRE(!mec::verify_chain_count(357913942, 12, &c), "one past");
    REQUIRE(mec::verify_chain_count(4294967295ll, 1, &c) && c == 4294967295u,
            "2^32-1 chains");
    REQUIRE(!mec::verify_chain_count(4294967296ll, 1, &c), "2^32 chains");
    REQUIRE(!mec::verify_chain_count(2147483647, 40, &c), "INT_MAX items");
    REQUIRE(!mec::verify_chain_count(INT64_MAX, 40, &c), "product overflow");
    REQUIRE(!mec::verify_chain_count(-1, 12, &c), "negative n");
    REQUIRE(!mec::verify_chain_count(1, 0, &c), "no rows");
    std::vector<uint32_t> list(2, 1u);
    uint8_t dummy = 1;
    REQUIRE(!mec::build_verify_list(357913942, 12, &dummy, &list) &&
                list.empty(),
            "list builder must refuse before reading the mask");
    printf("32-bit guard: ok\n");
    return true;
}

} // namespace

int main() {
    if (!check_verify_list() || !check_merge() || !check_guard()) return 1;
    /* EC8+4: single and multiple erasures, data and parity, a complete
     * item, an item complete in its data rows, and two TOO_FEW items */
    if (!check_rehash(8, 4,
                      {{0}, {11}, {3, 9}, {}, {8, 9, 10, 11}, {0, 1, 2, 3},
                       {0, 1, 2, 3, 4}, {1, 5, 7}, {2, 4, 6, 8, 10}, {7}},
                      "ec8+4"))
        return 1;
    /* (9,9): nine data rows gone is more than one 8-row entry; all nine
     * parity rows gone; ten rows gone is TOO_FEW */
    if (!check_rehash(9, 9,
                      {{0, 1, 2, 3, 4, 5, 6, 7, 8},
                       {},
                       {9, 10, 11, 12, 13, 14, 15, 16, 17},
                       {0, 1, 2, 3, 4, 5, 6, 7, 8, 9},
                       {0, 2, 4, 6, 8, 10, 12, 14, 16}},
                      "ec9+9"))
        return 1;
    printf("PASS\n");
    return 0;
}
