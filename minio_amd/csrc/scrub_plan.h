/* Host planner for mec_bitrot_verify_files*: the batch scrub.
 *
 * xlStorage.VerifyFile -> bitrotVerify (cmd/xl-storage.go:3082-3137,
 * cmd/bitrot.go:164-216) walks one shard file in the on-disk [hash||shard]*
 * format; the scanner's deep scan and healObject run it over every part of
 * every object on a drive.  A batch of such files has a file size, a part
 * size and a shard size per file, and sits in one device buffer at byte
 * offsets of any alignment.
 *
 * For HighwayHash256S a file of part bytes at shard size S has
 * ceil(part/S) frames at pitch 32+S, each 32 digest bytes followed by the
 * message; the last message has part - (frames-1)*S bytes.  The planner
 * turns the call's four tables into
 *
 *  - the device file table, one ScrubFile per file;
 *  - the early verdicts: a file whose size is not
 *    mec_bitrot_shard_file_size(part, S) is corrupt and a file of no part
 *    bytes is intact, neither with a frame hashed;
 *  - two chain lists of (file, frame) pairs, one hash chain per frame of
 *    every other file: `aligned` holds the chains whose message address
 *    base_mod8 + file_off + frame*(32+S) + 32 is a multiple of 8 (the digest
 *    in front of it then is too), `sheared` the rest.  Each list is ordered
 *    by descending message length, ties in ascending (file, frame) order, so
 *    the 16 chains of a wave are of near-equal length (var_plan.h's order);
 *
 * and reduces the per-chain ok bytes, in list order with the aligned list
 * first, back to one status and the lowest failing frame per file.
 *
 * Pure host code, no HIP includes: linked into the library and into the
 * stand-alone checker tools/scrub_plan_check.cpp.
 */
#ifndef MEC_SCRUB_PLAN_H
#define MEC_SCRUB_PLAN_H

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mec {

constexpr int64_t kScrubHashBytes = 32; /* HighwayHash-256 digest */

/* default bound on the frames of one call: chain indices are 32-bit */
constexpr uint64_t kScrubMaxFrames = UINT32_MAX;

/* one file as the kernels see it (hh_frames.hip reads it as 4 qwords) */
struct ScrubFile {
    int64_t off;     /* byte offset of the file in the device buffer */
    int64_t shard;   /* shard size S: message bytes of a full frame */
    int64_t last;    /* message bytes of the last frame, 1..S */
    uint32_t frames; /* 0 for a file with an early verdict */
    uint32_t pad;
};
static_assert(sizeof(ScrubFile) == 32, "ScrubFile is 4 qwords on the device");

struct ScrubChain {
    uint32_t file, frame;
};
static_assert(sizeof(ScrubChain) == 8, "ScrubChain is 2 dwords on the device");

enum ScrubEarly : uint8_t {
    kScrubHashed = 0,  /* the verdict comes from the file's chains */
    kScrubEmpty = 1,   /* part size 0, file size 0: intact */
    kScrubBadSize = 2, /* file size mismatch: corrupt */
};

struct ScrubPlan {
    std::vector<ScrubFile> files; /* n */
    std::vector<uint8_t> early;   /* n, ScrubEarly */
    std::vector<ScrubChain> aligned, sheared;
};

/* bitrotShardFileSize for HighwayHash256S: ceil(part/shard)*32 + part, -1
 * when that does not fit in int64.  part >= 0, shard >= 1. */
int64_t scrub_shard_file_size(int64_t part, int64_t shard);

/* F_0 = 0, F_{f+1} = F_f + align64(sizes[f]), n+1 entries.  False for
 * n <= 0, a NULL pointer, a negative size or an offset past int64. */
bool scrub_file_offsets(int n, const int64_t *sizes, int64_t *off);

/* False, with *pl unspecified, for an argument error: n <= 0, a NULL table,
 * a negative size, shard_sizes[f] < 1, file_off[f] < 0,
 * file_off[f] + file_sizes[f] > files_bytes, or more than max_frames frames
 * to hash.  base_mod8 is the device buffer's own address modulo 8. */
bool build_scrub_plan(int n, const int64_t *file_off,
                      const int64_t *file_sizes, const int64_t *part_sizes,
                      const int64_t *shard_sizes, int64_t files_bytes,
                      unsigned base_mod8, ScrubPlan *pl,
                      uint64_t max_frames = kScrubMaxFrames);

/* ok: aligned.size() + sheared.size() bytes, nonzero where the chain's
 * digest matched.  corrupt[f] = 0/1; first_bad[f] (may be NULL) = lowest
 * failing frame, -1 for an intact file and for a size mismatch. */
void reduce_scrub(const ScrubPlan &pl, const uint8_t *ok, uint8_t *corrupt,
                  int64_t *first_bad);

} // namespace mec
#endif
