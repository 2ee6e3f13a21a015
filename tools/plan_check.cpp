/* Stand-alone check of the mixed-pattern reconstruct planner
 * (minio_amd/csrc/recon_plan.cpp) against build_decode_plan, the single
 * pattern planner the uniform calls use.  Host code only; meant to be built
 * with -fsanitize=address,undefined and run by
 * tests/test_reconstruct_plan_cpu.py:
 *
 *   g++ -std=c++17 -fsanitize=address,undefined -I minio_amd/csrc \
 *       tools/plan_check.cpp minio_amd/csrc/recon_plan.cpp \
 *       minio_amd/csrc/gf_host.cpp -o plan_check && ./plan_check
 *
 * Prints one line per check group and exits non-zero on the first failure.
 */
#include "gf_host.h"
#include "recon_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

namespace {

int g_fail = 0;

#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);  \
            fprintf(stderr, __VA_ARGS__);                                    \
            fprintf(stderr, "\n");                                           \
            g_fail++;                                                        \
            return;                                                          \
        }                                                                    \
    } while (0)

/* every mask of `total` rows with exactly `erased` rows missing */
void masks_with_erasures(int total, int erased, std::vector<uint64_t> *out) {
    const uint64_t all = (1ull << total) - 1;
    for (uint64_t m = 0; m <= all; m++)
        if (__builtin_popcountll(all & ~m) == erased) out->push_back(m);
}

/* y = M x over GF(2) for the packed 8x8 bit matrix (byte b = row mask) */
uint8_t apply_bits(const uint32_t w[2], uint8_t x) {
    const uint64_t m = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    uint8_t y = 0;
    for (int b = 0; b < 8; b++) {
        const uint8_t row = (uint8_t)(m >> (8 * b));
        if (__builtin_popcount(row & x) & 1) y |= (uint8_t)(1u << b);
    }
    return y;
}

struct Lcg {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

/* Checks one plan against build_decode_plan, mask by mask.  item_mask[i]
 * is item i's present-bit mask. */
void check_plan(const uint8_t *enc, int d, int p, int data_only,
                const std::vector<uint64_t> &item_mask,
                const mec::ReconPlan &pl) {
    const int total = d + p;
    const int n = (int)item_mask.size();
    const uint64_t all = (1ull << total) - 1;
    const uint64_t data_rows = (1ull << d) - 1;

    /* what the uniform planner says for each distinct mask */
    struct Want {
        bool too_few;
        int n_dst;
        std::vector<int> src, dst;
        std::vector<uint8_t> dec;
    };
    std::map<uint64_t, Want> want;
    for (uint64_t m : item_mask) {
        if (want.count(m)) continue;
        Want w;
        uint8_t present[mec::kPlanMaxTotal];
        for (int s = 0; s < total; s++) present[s] = (m >> s) & 1;
        w.src.resize(mec::kMaxShards);
        w.dst.resize(mec::kMaxShards);
        w.dec.resize((size_t)total * d);
        w.n_dst = 0;
        w.too_few = !mec::build_decode_plan(enc, d, p, present, data_only,
                                            w.src.data(), w.dst.data(),
                                            &w.n_dst, w.dec.data());
        if (w.too_few) w.n_dst = 0;
        want[m] = w;
    }

    /* per-item status */
    CHECK((int)pl.status.size() == n, "status size %zu", pl.status.size());
    int n_too_few = 0;
    for (int i = 0; i < n; i++) {
        const Want &w = want[item_mask[i]];
        const uint8_t ws = w.too_few ? mec::kPlanTooFew : mec::kPlanOk;
        CHECK(pl.status[i] == ws, "item %d mask %llx status %d want %d", i,
              (unsigned long long)item_mask[i], pl.status[i], ws);
        n_too_few += w.too_few;
    }
    CHECK(pl.n_too_few == n_too_few, "n_too_few %d want %d", pl.n_too_few,
          n_too_few);

    /* table: exactly ceil(n_dst/8) consecutive entries per distinct mask
     * that needs work, none for the others, no duplicates */
    CHECK(pl.entries.size() == pl.entry_mask.size(), "entry_mask size");
    std::map<uint64_t, std::vector<uint32_t>> by_mask;
    for (uint32_t e = 0; e < pl.entries.size(); e++)
        by_mask[pl.entry_mask[e]].push_back(e);
    size_t want_entries = 0;
    for (auto &kv : want) {
        const uint64_t m = kv.first;
        const Want &w = kv.second;
        const size_t ne =
            (size_t)(w.n_dst + mec::kPlanMaxE - 1) / mec::kPlanMaxE;
        want_entries += ne;
        const size_t got = by_mask.count(m) ? by_mask[m].size() : 0;
        CHECK(got == ne, "mask %llx: %zu entries, want %zu",
              (unsigned long long)m, got, ne);
        if (m == all) CHECK(ne == 0, "all-present mask has work");
        if (data_only && (m & data_rows) == data_rows)
            CHECK(ne == 0, "data-complete mask has work under data_only");
        /* rows and coefficients, chunk by chunk */
        for (size_t c = 0; c < ne; c++) {
            const uint32_t e = by_mask[m][c];
            CHECK(c == 0 || e == by_mask[m][c - 1] + 1,
                  "mask %llx entries not consecutive", (unsigned long long)m);
            const mec::ReconPlanEntry &ent = pl.entries[e];
            const int t0 = (int)c * mec::kPlanMaxE;
            const int ee = w.n_dst - t0 > mec::kPlanMaxE ? mec::kPlanMaxE
                                                         : w.n_dst - t0;
            CHECK((int)ent.n_dst == ee, "entry %u n_dst %u want %d", e,
                  ent.n_dst, ee);
            for (int k = 0; k < d; k++)
                CHECK(ent.src_rows[k] == w.src[k], "entry %u src[%d]", e, k);
            for (int i = 0; i < ee; i++)
                CHECK(ent.dst_rows[i] == w.dst[t0 + i], "entry %u dst[%d]", e,
                      i);
            CHECK((size_t)ent.mask_off + (size_t)ee * d * 2 <=
                      pl.masks.size(),
                  "entry %u masks out of range", e);
            for (int i = 0; i < ee; i++)
                for (int k = 0; k < d; k++) {
                    const uint32_t *mw =
                        &pl.masks[ent.mask_off + ((size_t)i * d + k) * 2];
                    const uint8_t coef = w.dec[(size_t)(t0 + i) * d + k];
                    for (int x = 0; x < 256; x++)
                        CHECK(apply_bits(mw, (uint8_t)x) ==
                                  mec::gf_mul(coef, (uint8_t)x),
                              "entry %u coef[%d][%d]=%02x x=%02x", e, i, k,
                              coef, x);
                }
        }
    }
    CHECK(pl.entries.size() == want_entries, "table has %zu entries, want %zu",
          pl.entries.size(), want_entries);

    /* E lists: every (recoverable item needing work) x (its entries)
     * exactly once, in the list of the entry's row count; nothing else */
    std::set<std::pair<uint32_t, uint32_t>> seen;
    CHECK(pl.work[0].empty(), "work[0] must stay empty");
    size_t n_pairs = 0;
    for (int e = 1; e <= mec::kPlanMaxE; e++)
        for (const mec::ReconWork &wk : pl.work[e]) {
            CHECK(wk.item < (uint32_t)n, "work item %u out of range", wk.item);
            CHECK(wk.entry < pl.entries.size(), "work entry %u out of range",
                  wk.entry);
            CHECK((int)pl.entries[wk.entry].n_dst == e,
                  "entry %u in list %d has n_dst %u", wk.entry, e,
                  pl.entries[wk.entry].n_dst);
            CHECK(pl.entry_mask[wk.entry] == item_mask[wk.item],
                  "item %u paired with another mask's entry %u", wk.item,
                  wk.entry);
            CHECK(seen.insert({wk.item, wk.entry}).second,
                  "pair (%u,%u) listed twice", wk.item, wk.entry);
            n_pairs++;
        }
    size_t want_pairs = 0;
    for (int i = 0; i < n; i++) {
        const uint64_t m = item_mask[i];
        if (!by_mask.count(m)) continue;
        for (uint32_t e : by_mask[m]) {
            CHECK(seen.count({(uint32_t)i, e}), "pair (%d,%u) missing", i, e);
            want_pairs++;
        }
    }
    CHECK(n_pairs == want_pairs, "%zu pairs listed, want %zu", n_pairs,
          want_pairs);
}

void run_case(const char *name, int d, int p, int data_only,
              const std::vector<uint64_t> &item_mask, mec::ReconPlan *pl) {
    const int total = d + p;
    std::vector<uint8_t> enc((size_t)total * d);
    if (!mec::build_encode_matrix(d, p, enc.data())) {
        fprintf(stderr, "FAIL %s: build_encode_matrix\n", name);
        g_fail++;
        return;
    }
    std::vector<uint8_t> present(item_mask.size() * total);
    for (size_t i = 0; i < item_mask.size(); i++)
        for (int s = 0; s < total; s++)
            /* any non-zero byte counts as present */
            present[i * total + s] = ((item_mask[i] >> s) & 1) ? (uint8_t)(1 + (i & 0x7f)) : 0;
    const int before = g_fail;
    if (!mec::build_reconstruct_plan(enc.data(), d, p, (int)item_mask.size(),
                                     present.data(), data_only, pl)) {
        fprintf(stderr, "FAIL %s: build_reconstruct_plan refused\n", name);
        g_fail++;
        return;
    }
    check_plan(enc.data(), d, p, data_only, item_mask, *pl);
    printf("%s data_only=%d: n=%zu entries=%zu too_few=%d %s\n", name,
           data_only, item_mask.size(), pl->entries.size(), pl->n_too_few,
           g_fail == before ? "ok" : "FAILED");
}

} // namespace

int main() {
    /* EC8+4: all 793 masks of 1..4 erasures, the all-present mask, two
     * masks with 5 erased; each 3 times, shuffled */
    {
        const int d = 8, p = 4, total = 12;
        std::vector<uint64_t> masks;
        for (int e = 1; e <= 4; e++) masks_with_erasures(total, e, &masks);
        if (masks.size() != 793) {
            fprintf(stderr, "FAIL: %zu masks, want 793\n", masks.size());
            return 1;
        }
        const uint64_t all = (1ull << total) - 1;
        masks.push_back(all);
        masks.push_back(all & ~0x01full);  /* rows 0-4 erased */
        masks.push_back(all & ~0xa92ull);  /* rows 1,4,7,9,11 erased */
        std::vector<uint64_t> items;
        for (int r = 0; r < 3; r++)
            items.insert(items.end(), masks.begin(), masks.end());
        Lcg rng{0x6d696e696full};
        for (size_t i = items.size() - 1; i > 0; i--) {
            size_t j = rng.next() % (i + 1);
            std::swap(items[i], items[j]);
        }
        mec::ReconPlan pl;
        for (int data_only = 0; data_only <= 1; data_only++) {
            run_case("ec8+4 all patterns", d, p, data_only, items, &pl);
            if (g_fail) return 1;
            /* 793 masks need work when parity counts too; under data_only
             * the C(4,k) parity-only masks (k=1..4: 15 of them) do not */
            const size_t want = data_only ? 793 - 15 : 793;
            if (pl.entries.size() != want) {
                fprintf(stderr, "FAIL: %zu entries, want %zu\n",
                        pl.entries.size(), want);
                return 1;
            }
            if (pl.n_too_few != 6) {
                fprintf(stderr, "FAIL: %d items TOO_FEW, want 6\n",
                        pl.n_too_few);
                return 1;
            }
        }
    }
    /* (9,9) with all 9 data rows erased: two entries, 8 rows + 1 row, over
     * the same sources */
    {
        const int d = 9, p = 9;
        const uint64_t all = (1ull << 18) - 1;
        std::vector<uint64_t> items(4, all & ~0x1ffull);
        items[2] = all; /* a complete item in between */
        mec::ReconPlan pl;
        for (int data_only = 0; data_only <= 1; data_only++) {
            run_case("ec9+9 nine data rows", d, p, data_only, items, &pl);
            if (g_fail) return 1;
            if (pl.entries.size() != 2 || pl.entries[0].n_dst != 8 ||
                pl.entries[1].n_dst != 1 ||
                memcmp(pl.entries[0].src_rows, pl.entries[1].src_rows,
                       sizeof(pl.entries[0].src_rows)) != 0 ||
                pl.work[8].size() != 3 || pl.work[1].size() != 3) {
                fprintf(stderr, "FAIL: ec9+9 chunking\n");
                return 1;
            }
        }
    }
    /* bad dimensions are refused, n = 0 is an empty plan */
    {
        mec::ReconPlan pl;
        std::vector<uint8_t> enc(64 * 64, 0);
        uint8_t present[64] = {0};
        if (mec::build_reconstruct_plan(enc.data(), 33, 2, 1, present, 0, &pl) ||
            mec::build_reconstruct_plan(enc.data(), 30, 11, 1, present, 0, &pl) ||
            mec::build_reconstruct_plan(enc.data(), 8, 4, -1, present, 0, &pl)) {
            fprintf(stderr, "FAIL: bad dimensions accepted\n");
            return 1;
        }
        std::vector<uint8_t> enc84(12 * 8);
        mec::build_encode_matrix(8, 4, enc84.data());
        if (!mec::build_reconstruct_plan(enc84.data(), 8, 4, 0, present, 0,
                                         &pl) ||
            !pl.entries.empty() || !pl.status.empty()) {
            fprintf(stderr, "FAIL: n=0\n");
            return 1;
        }
        printf("dimension checks: ok\n");
    }
    if (g_fail) return 1;
    printf("PASS\n");
    return 0;
}
