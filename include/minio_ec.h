/* minio_ec.h — C-ABI drop-in boundary for MinIO's erasure-coding + bitrot
 * hot path, MI355X (gfx950) native implementation.
 *
 * This is the surface a thin cgo shim binds to satisfy the reference's Go
 * interfaces (see INTEGRATION.md for the shim):
 *
 *  - reedsolomon.Encoder methods used by the reference
 *    (cmd/erasure-coding.go:81 Split, :85 Encode, :106 ReconstructData,
 *     :112 Reconstruct)                       -> mec_encode_batch /
 *                                                mec_reconstruct_batch
 *  - bitrotWriter's per-shard hash step
 *    (cmd/bitrot-streaming.go:57-59)          -> fused into mec_encode_batch
 *                                                (checksums output)
 *  - bitrotReader verify-on-read
 *    (cmd/bitrot-streaming.go:185-197)        -> mec_bitrot_verify_batch
 *  - bitrotVerify / VerifyFile scrub
 *    (cmd/bitrot.go:164-216)                  -> mec_bitrot_verify_stream
 *  - Erasure.Encode block loop + streaming [hash||shard]* on-disk layout
 *    (cmd/erasure-encode.go:76-108, cmd/bitrot-streaming.go:44-75)
 *                                             -> mec_encode_stream
 *  - Erasure.Decode / Heal
 *    (cmd/erasure-decode.go:239-314, :317-364) -> mec_decode_stream /
 *                                                mec_heal_stream
 *  - shard-size math (cmd/erasure-coding.go:116-141, cmd/bitrot.go:156-161)
 *                                             -> mec_shard_size etc.
 *
 * Calls are synchronous and thread-safe per context; a context owns one GPU
 * (one HIP stream + staging buffers).  Batching across objects/blocks is the
 * caller's (shim's) job: the reference API is per-block, GPU efficiency
 * needs hundreds of blocks per call.
 *
 * All functions return mec_status unless documented otherwise.  Status codes
 * map 1:1 onto the Go error values the shim must surface
 * (reedsolomon.ErrInvShardNum etc., cmd/erasure-coding.go:45-49,
 *  errFileCorrupt for bitrot mismatches).
 */
#ifndef MINIO_EC_H
#define MINIO_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mec_ctx mec_ctx;

typedef enum {
    MEC_OK = 0,
    MEC_ERR_INV_SHARD_NUM = 1,  /* reedsolomon.ErrInvShardNum */
    MEC_ERR_MAX_SHARD_NUM = 2,  /* reedsolomon.ErrMaxShardNum */
    MEC_ERR_TOO_FEW_SHARDS = 3, /* reedsolomon.ErrTooFewShards */
    MEC_ERR_SHORT_DATA = 4,     /* reedsolomon.ErrShortData */
    MEC_ERR_FILE_CORRUPT = 5,   /* errFileCorrupt (bitrot mismatch) */
    MEC_ERR_INVALID_ARG = 6,
    MEC_ERR_HIP = 7,            /* HIP runtime failure (message via
                                   mec_last_error) */
    MEC_ERR_NO_GPU = 8,         /* no MI355X visible — the product path
                                   fails loudly, it never falls back */
    MEC_ERR_INTERNAL = 9,       /* invariant violation inside this library
                                   (a bug, not a caller/quorum condition) */
} mec_status;

/* Bitrot algorithm ids — values mirror the reference enum
 * (cmd/xl-storage-format-v1.go:146-153). */
typedef enum {
    MEC_BITROT_SHA256 = 1,
    MEC_BITROT_HIGHWAYHASH256 = 2,
    MEC_BITROT_HIGHWAYHASH256S = 3, /* DefaultBitrotAlgorithm */
    MEC_BITROT_BLAKE2B512 = 4,
} mec_bitrot_algo;

int mec_version(void);
const char *mec_last_error(void); /* thread-local message for MEC_ERR_HIP */
int mec_device_count(void);       /* number of visible GPUs */

/* ---- context ---------------------------------------------------------- */

/* Geometry checks mirror NewErasure (cmd/erasure-coding.go:42-50). */
mec_status mec_ctx_create(int data_shards, int parity_shards,
                          int64_t block_size, int device, mec_ctx **out);
void mec_ctx_destroy(mec_ctx *ctx);
int mec_ctx_d(mec_ctx *ctx);
int mec_ctx_p(mec_ctx *ctx);
int64_t mec_ctx_block_size(mec_ctx *ctx);

/* ---- shard-size math (host, exact int mirrors) ------------------------ */

int64_t mec_shard_size(int64_t block_size, int data_shards); /* ceilFrac */
int64_t mec_shard_file_size(int64_t block_size, int data_shards,
                            int64_t total_length);
int64_t mec_shard_file_offset(int64_t block_size, int data_shards,
                              int64_t start_offset, int64_t length,
                              int64_t total_length);
int64_t mec_bitrot_shard_file_size(int64_t size, int64_t shard_size,
                                   int algo);
/* Device-side stride for one shard (shard_size rounded up to 64 B). */
int64_t mec_shard_stride(int64_t block_size, int data_shards);

/* ---- batch encode (the north-star kernel) ------------------------------
 *
 * n independent blocks, each block_len bytes (1 <= block_len <= block_size).
 * Device layout (the _dev entry points):
 *   data:   n * d * stride bytes; shard k of block b at
 *           data + (b*d + k)*stride, holding
 *           min(max(block_len - k*S, 0), S) valid bytes, zero-padded to S
 *           (Split semantics, cmd/erasure-coding.go:81), bytes S..stride
 *           undefined; S = mec_shard_size, stride = mec_shard_stride.
 *   parity: n * p * stride bytes (output).
 *   sums:   n * (d+p) * hash_size bytes (output; per-shard digest over the
 *           S padded shard bytes, as streamingBitrotWriter hashes them).
 *           May be NULL to skip hashing (encode only).
 * Host-pointer version: data is the packed object bytes, n * block_len
 * contiguous (the Go Split aliasing shape); the library stages/scatters.
 * Runs on the context's stream; synchronous unless noted. */
mec_status mec_encode_batch_dev(mec_ctx *ctx, int n, const void *data_dev,
                                int64_t block_len, void *parity_dev,
                                int bitrot_algo, void *sums_dev);
mec_status mec_encode_batch(mec_ctx *ctx, int n, const uint8_t *data,
                            int64_t block_len, uint8_t *parity,
                            int bitrot_algo, uint8_t *sums);

/* Async variant for bench pipelining: does not synchronize the stream. */
mec_status mec_encode_batch_dev_async(mec_ctx *ctx, int n,
                                      const void *data_dev, int64_t block_len,
                                      void *parity_dev, int bitrot_algo,
                                      void *sums_dev);

/* Pipelined encode: batch t's hash overlaps batch t+1's GF kernel (the
 * hash is latency-bound per chain and leaves most SIMDs idle; independent
 * batches — i.e. different objects — fill them).  CONTRACT: alternate two
 * parity/sums buffer sets in strict round-robin and call mec_pipe_sync
 * before reading results.  Per-call results are identical to
 * mec_encode_batch_dev.  Requires a compiled (d,p) specialization and a
 * HighwayHash algorithm. */
mec_status mec_encode_batch_dev_pipe(mec_ctx *ctx, int n,
                                     const void *data_dev, int64_t block_len,
                                     void *parity_dev, int bitrot_algo,
                                     void *sums_dev);
mec_status mec_pipe_sync(mec_ctx *ctx);

/* ---- batch encode, one block length PER ITEM ----------------------------
 *
 * The calls above take one block_len for the whole batch.  A PUT batch
 * ACROSS objects is not uniform: Erasure.Encode
 * (cmd/erasure-encode.go:76-108) calls EncodeData(buf[:n]) with whatever
 * io.ReadFull returned, so every object of at most one block is a single
 * short block and the last block of every larger object is short too.  The
 * lengths cannot be padded to a common one: the shard size is ceil(len/d)
 * (Split, cmd/erasure-coding.go:81), so another length moves every byte to
 * another shard and column and changes the parity and all d+p digests.
 * Here block_lens[i] (host, n entries, each in [1, block_size]) is item i's
 * own length; the shim's PUT batcher fills it (INTEGRATION.md "Batching
 * PUTs of different sizes").
 *
 * Device layout: packed, defined by the lengths alone.  For item i
 *   S_i = ceil(len_i/d), stride_i = align64(S_i),
 *   R_0 = 0, R_{i+1} = R_i + stride_i   (the row-offsets helper below)
 *   data:   d*R_n bytes; row k of item i at d*R_i + k*stride_i, holding
 *           Split's contents: min(max(len_i - k*S_i, 0), S_i) valid bytes,
 *           zero-padded to S_i.  Bytes [S_i, stride_i) are undefined and
 *           never influence a result.
 *   parity: p*R_n bytes (output); row t of item i at p*R_i + t*stride_i.
 *           Bytes past S_i are scratch.
 *   sums:   n*(d+p)*32 bytes in the fused layout of the uniform calls: the
 *           digest of row s of item i at (i*(d+p)+s)*32, over exactly S_i
 *           bytes.  NULL: encode only, nothing is hashed.  Otherwise
 *           bitrot_algo must be MEC_BITROT_HIGHWAYHASH256S or
 *           MEC_BITROT_HIGHWAYHASH256 (anything else: MEC_ERR_INVALID_ARG).
 * A 4 KiB object at EC8+4 so takes 8 rows of 512 B, not of 128 KiB.
 *
 * The geometry needs a compiled (d,p) specialization, as the pipelined
 * encode does; otherwise MEC_ERR_INVALID_ARG with a message in
 * mec_last_error.  Every argument error (n <= 0, a NULL buffer, a length
 * outside [1, block_size], n*(d+p) past 32 bits, the algorithm, the
 * geometry) is reported before anything is launched or written.  n is not
 * limited to 65535.  Two kernels per call whatever the lengths: the GF
 * kernel runs over one flattened column space, so short items share waves,
 * and the hash kernel takes the items longest first.
 *
 * The row-offsets helper is pure host math: no context, no GPU.  It writes
 * R_0..R_n into row_off (n+1 entries) and returns MEC_ERR_INVALID_ARG for
 * n <= 0, a length outside [1, block_size], or a batch whose chain ids
 * would not fit in 32 bits (it does not know p, so it checks n*d; the
 * encode calls check n*(d+p)).
 * _async does not synchronize the stream (pair with mec_stream_sync);
 * back-to-back _async calls with different length tables need no sync in
 * between.  The host-pointer variant takes data as the blocks concatenated,
 * sum(len_i) bytes, does the Split scatter into pinned staging and one
 * plain upload (no overlapped ingest), and returns parity packed: item i's
 * p rows of S_i bytes each at p*sum_{j<i} S_j; sums in the fused layout. */
mec_status mec_var_row_offsets(int data_shards, int64_t block_size, int n,
                               const int64_t *block_lens, int64_t *row_off);
mec_status mec_encode_batch_var_dev(mec_ctx *ctx, int n, const void *data_dev,
                                    const int64_t *block_lens,
                                    void *parity_dev, int bitrot_algo,
                                    void *sums_dev);
mec_status mec_encode_batch_var_dev_async(mec_ctx *ctx, int n,
                                          const void *data_dev,
                                          const int64_t *block_lens,
                                          void *parity_dev, int bitrot_algo,
                                          void *sums_dev);
mec_status mec_encode_batch_var(mec_ctx *ctx, int n, const uint8_t *data,
                                const int64_t *block_lens, uint8_t *parity,
                                int bitrot_algo, uint8_t *sums);

/* ---- batch encode into on-disk [hash||shard] frames, length PER ITEM -----
 *
 * mec_encode_batch_var* ends with parity rows at a 64-byte stride and the
 * digests in a separate table.  A drive stores neither: it stores
 * streamingBitrotWriter's [hash||shard]* stream
 * (cmd/bitrot-streaming.go:44-75), the format mec_bitrot_verify_files*
 * scrubs.  These calls take the same input as mec_encode_batch_var* and
 * leave, per logical shard row, one contiguous byte stream that is exactly
 * what goes to that row's drive, ready for one D2H or one send.
 *
 * Output layout: defined by the lengths alone.  With S_i = ceil(len_i/d) and
 * total = d+p,
 *   F_0 = 0, F_{i+1} = F_i + 32 + S_i        (mec_frame_offsets)
 *   frames: total*F_n bytes; row s's stream is [s*F_n, (s+1)*F_n); in it
 *           item i's frame at F_i: the 32-byte HighwayHash-256 digest (magic
 *           key) of the S_i shard bytes, then those bytes.  Data rows hold
 *           Split's zero-padded contents, parity rows the encode's.
 * Every byte of frames is defined after the call: no stride, no scratch.
 * Consecutive blocks of one object passed as consecutive items make
 * [F_first, F_{last+1}) of row s that object's shard file for logical row s,
 * byte for byte what mec_encode_stream writes; the shim applies Distribution
 * as for every other call (INTEGRATION.md "Shard distribution").
 *
 * data_dev is mec_encode_batch_var_dev's packed data (d*R_n bytes, R from
 * mec_var_row_offsets) and is never written.  frames_dev may have any byte
 * alignment; exactly total*F_n bytes are written and nothing outside them.
 * Parity, digests and tables live in the context's grow-only buffers.
 * bitrot_algo is MEC_BITROT_HIGHWAYHASH256S or MEC_BITROT_HIGHWAYHASH256;
 * the geometry needs a compiled (d,p) specialization as above.  Every
 * argument error (n <= 0, a NULL pointer, a length outside [1, block_size],
 * n*(d+p) past 32 bits, the algorithm, the geometry) returns
 * MEC_ERR_INVALID_ARG before anything is launched or written.  n is not
 * limited to 65535.  Three kernels per call whatever the lengths.
 *
 * mec_frame_offsets is pure host math: no context, no GPU.  It writes
 * F_0..F_n into frame_off (n+1 entries) and returns MEC_ERR_INVALID_ARG,
 * with nothing written, for n <= 0, a NULL pointer or a length outside
 * [1, block_size].
 * _async does not synchronize the stream (pair with mec_stream_sync);
 * back-to-back _async calls with different length tables and different
 * output buffers need no sync in between: the shared scratch is ordered by
 * the stream.  The host-pointer variant takes data as the blocks
 * concatenated, sum(len_i) bytes, does the Split scatter into pinned
 * staging, one plain upload (no overlapped ingest), and one D2H of
 * total*F_n bytes into frames. */
mec_status mec_frame_offsets(int data_shards, int64_t block_size, int n,
                             const int64_t *block_lens, int64_t *frame_off);
mec_status mec_encode_frames_batch_var_dev(mec_ctx *ctx, int n,
                                           const void *data_dev,
                                           const int64_t *block_lens,
                                           void *frames_dev, int bitrot_algo);
mec_status mec_encode_frames_batch_var_dev_async(mec_ctx *ctx, int n,
                                                 const void *data_dev,
                                                 const int64_t *block_lens,
                                                 void *frames_dev,
                                                 int bitrot_algo);
mec_status mec_encode_frames_batch_var(mec_ctx *ctx, int n,
                                       const uint8_t *data,
                                       const int64_t *block_lens,
                                       uint8_t *frames, int bitrot_algo);

/* ---- batch reconstruct (ReconstructData / Reconstruct / Heal kernel) ---
 *
 * shards_dev: n * (d+p) * stride bytes; present[i] != 0 marks shard row i
 * intact for ALL n items (the erasure pattern of one object's read).
 * Missing rows are reconstructed in place (data rows only when data_only).
 * Matrix inversion happens once on host per call. */
mec_status mec_reconstruct_batch_dev(mec_ctx *ctx, int n, void *shards_dev,
                                     const uint8_t *present,
                                     int64_t shard_len, int data_only);
mec_status mec_reconstruct_batch(mec_ctx *ctx, int n, uint8_t *shards,
                                 const uint8_t *present, int64_t shard_len,
                                 int data_only);
mec_status mec_reconstruct_batch_dev_async(mec_ctx *ctx, int n,
                                           void *shards_dev,
                                           const uint8_t *present,
                                           int64_t shard_len, int data_only);

/* ---- batch reconstruct, one erasure pattern PER ITEM --------------------
 *
 * The calls above hold one pattern for the whole batch, which is one
 * object's read.  A degraded read or heal batched ACROSS objects is not
 * uniform: every object places its shards by its own rotation,
 * Distribution = hashOrder(bucket/object, d+p)
 * (cmd/erasure-metadata-utils.go:178, applied to the drive list by
 * shuffleDisks, cmd/erasure-metadata-utils.go:323), so one dead drive is a different missing logical row in each object, and
 * a bitrot hit (cmd/bitrot-streaming.go:185-197) changes the pattern of a
 * single block.  Here present + i*(d+p) is item i's own mask; the shim
 * fills it per block from the rows it could read and verify
 * (INTEGRATION.md "Shard distribution").
 *
 * Layout and in-place semantics are mec_reconstruct_batch_dev's:
 * n * (d+p) * stride bytes, missing rows rebuilt in their slots from the
 * item's first d present rows (data rows only when data_only); present
 * rows are never written.  Per item:
 *   - nothing to rebuild (all rows present, or data_only with all data
 *     rows present): skipped;
 *   - fewer than d rows present: unrecoverable.  With item_status non-NULL
 *     item_status[i] = MEC_ERR_TOO_FEW_SHARDS, the item's bytes are left
 *     untouched, every other item is rebuilt with item_status MEC_OK and
 *     the call returns MEC_OK — one unreadable object does not fail the
 *     batch.  With item_status NULL the call returns
 *     MEC_ERR_TOO_FEW_SHARDS before anything is launched or modified.
 * One matrix inversion per DISTINCT mask per call, and one kernel launch
 * per rebuilt-row count in use (at most 8 per call while no pattern
 * rebuilds more than 8 rows), whatever the number of patterns.  n is not
 * limited to 65535.
 * _async does not synchronize the stream (pair with mec_stream_sync);
 * back-to-back _async calls with different masks need no sync in between.
 * The host-pointer variant takes packed n*(d+p)*shard_len bytes, uploads
 * them in one plain unchunked copy (no overlapped ingest yet), and writes
 * back only the rebuilt rows. */
mec_status mec_reconstruct_batch_mixed_dev(mec_ctx *ctx, int n,
                                           void *shards_dev,
                                           const uint8_t *present,
                                           int64_t shard_len, int data_only,
                                           uint8_t *item_status);
mec_status mec_reconstruct_batch_mixed_dev_async(mec_ctx *ctx, int n,
                                                 void *shards_dev,
                                                 const uint8_t *present,
                                                 int64_t shard_len,
                                                 int data_only,
                                                 uint8_t *item_status);
mec_status mec_reconstruct_batch_mixed(mec_ctx *ctx, int n, uint8_t *shards,
                                       const uint8_t *present,
                                       int64_t shard_len, int data_only,
                                       uint8_t *item_status);

/* ---- verified batch read: bitrot check on device, then reconstruct ------
 *
 * The mixed calls above take a mask that is already known: the shim must
 * have bitrot-checked every row before it calls them.  In the reference
 * the two steps are one operation: streamingBitrotReader.ReadAt
 * (cmd/bitrot-streaming.go:161-200) returns errFileCorrupt for a block
 * whose hash does not match, parallelReader.Read
 * (cmd/erasure-decode.go:127-235) triggers d reads, drops a row that
 * failed for that block and reads another, and Decode or Heal
 * (cmd/erasure-decode.go:239-364) reconstructs from what verified.  These
 * calls do the same for a batch across objects whose rows are in HBM:
 *   1. bitrot-check, on the GPU, only the rows that were read;
 *   2. treat a mismatch as a missing row of that item;
 *   3. rebuild in place through the mixed planner and kernels;
 *   4. with rehash, write fresh digests for the rebuilt rows, as
 *      Erasure.Heal does by writing a healed shard through a bitrot writer.
 *
 * shards_dev: mec_reconstruct_batch_mixed_dev's layout, n*(d+p)*stride
 *     bytes, row s of item i at (i*(d+p)+s)*stride, rebuilt in place.
 * sums_dev:   n*(d+p)*32 bytes in the fused sums layout
 *     mec_encode_batch_dev writes, so encode output feeds straight back
 *     in.  On entry the expected digest of every row flagged in read_mask;
 *     other slots are ignored.  Modified only when rehash != 0: the slots
 *     of the rebuilt rows of recoverable items then hold the digests of
 *     the rebuilt bytes; slots of verified rows are never written.
 * read_mask (host, n*(d+p) bytes): nonzero = the row was read from its
 *     drive, so its bytes and digest are there.  Zero = dead drive, row
 *     not fetched yet, or errFileNotFound; such rows are never hashed and
 *     their bytes and digest slots may hold anything.
 * bitrot_algo: MEC_BITROT_HIGHWAYHASH256S or MEC_BITROT_HIGHWAYHASH256 (the
 *     same keyed function; only the streaming format has per-block digests
 *     at all).  Anything else: MEC_ERR_INVALID_ARG.
 * present_out (host, n*(d+p) bytes, may be NULL): 1 where the row was read
 *     and its digest matched, else 0.  read_mask set and present_out 0 is
 *     a bitrot hit: the shim maps it to errFileCorrupt and queues the
 *     heal, as parallelReader does with bitrotHeal
 *     (cmd/erasure-decode.go:197-198, :227-228).
 * item_status, data_only: mec_reconstruct_batch_mixed_dev's semantics,
 *     applied to the verified mask.  Fewer than d verified rows:
 *     item_status[i] = MEC_ERR_TOO_FEW_SHARDS, the item's bytes and digests
 *     stay untouched, the rest of the batch proceeds; the shim reads more
 *     rows of that item and calls again.  With item_status NULL any such
 *     item makes the call return MEC_ERR_TOO_FEW_SHARDS with nothing
 *     modified; present_out is still filled.  Verified rows are never
 *     written; a row that failed verification is rebuilt in its slot when
 *     it is in scope (any row, or data rows only under data_only).
 *
 * n*(d+p) must fit in 32 bits (else MEC_ERR_INVALID_ARG); n is not limited
 * to 65535.  shard_len is one value for the whole call; the _var calls
 * below take a length per item.  The calls are synchronous, since the host
 * needs the verdicts to plan: one stream synchronise before planning, one
 * at the end, and no _async variant.  mec_decode_stream and
 * mec_heal_stream keep their own per-object host grouping.
 * The host-pointer variant takes rows packed at shard_len and digests
 * packed at 32 B, packs only the rows flagged in read_mask, uploads in one
 * plain copy, and writes back only the rebuilt rows (and, with rehash,
 * their digests). */
mec_status mec_verify_reconstruct_batch_dev(
    mec_ctx *ctx, int n, void *shards_dev, void *sums_dev,
    const uint8_t *read_mask, int64_t shard_len, int bitrot_algo,
    int data_only, int rehash, uint8_t *present_out, uint8_t *item_status);
mec_status mec_verify_reconstruct_batch(
    mec_ctx *ctx, int n, uint8_t *shards, uint8_t *sums,
    const uint8_t *read_mask, int64_t shard_len, int bitrot_algo,
    int data_only, int rehash, uint8_t *present_out, uint8_t *item_status);

/* ---- verified batch read, one shard length PER ITEM ---------------------
 *
 * The read-side twin of mec_encode_batch_var.  parallelReader.Read shortens
 * shardSize for the last block of an object (cmd/erasure-decode.go:138-139)
 * and an object of at most one block is only a short block, so every GET or
 * heal batched across objects holds items of different shard lengths; since
 * the shard size is ceil(len/d), rows of different lengths cannot be padded
 * to a common one.  block_lens[i] (host, n entries, each in
 * [1, block_size]) is item i's block length, as for mec_encode_batch_var;
 * only S_i = ceil(len_i/d) matters here, so a caller that knows the shard
 * length alone passes min(S_i*d, block_size), which gives the same S_i
 * (INTEGRATION.md "Batching GETs of different sizes").
 *
 * Device layout, with S_i, stride_i, R_i as defined for
 * mec_encode_batch_var (mec_var_row_offsets computes R_0..R_n for both
 * directions) and total = d+p:
 *   shards_dev: one buffer of total*R_n bytes; row s of item i at
 *       total*R_i + s*stride_i, S_i bytes valid, rebuilt in place.  Bytes
 *       [S_i, stride_i) never influence a result and are scratch after a
 *       rebuild.  Rows not flagged in read_mask may hold anything and are
 *       never hashed.
 *   sums_dev: the fused layout, (i*total+s)*32, exactly what
 *       mec_encode_batch_var_dev writes, so its digests feed straight back
 *       in.
 * read_mask, present_out, item_status, data_only, rehash and bitrot_algo
 * are mec_verify_reconstruct_batch_dev's, unchanged: verified rows are
 * never written; an item with fewer than d verified rows gets
 * MEC_ERR_TOO_FEW_SHARDS in item_status and is left untouched while the
 * rest proceeds; with item_status NULL such an item makes the call return
 * MEC_ERR_TOO_FEW_SHARDS with nothing modified and present_out filled.
 * Every argument error (n <= 0, a NULL buffer, a length outside
 * [1, block_size], the algorithm, n*(d+p) past 32 bits) is reported before
 * anything is launched or written.  n is not limited to 65535.  Any (d,p)
 * works: the reconstruct kernels are generic, unlike the encode var call.
 * Synchronous, two stream synchronises, no _async variant.
 *
 * The host-pointer variant takes rows packed at S_i (item i's total rows at
 * total * sum_{j<i} S_j) and digests packed at 32 B, packs only the rows
 * flagged in read_mask into pinned staging, uploads in one plain copy, and
 * writes back only the rebuilt rows (and, with rehash, their digests). */
mec_status mec_verify_reconstruct_batch_var_dev(
    mec_ctx *ctx, int n, void *shards_dev, void *sums_dev,
    const int64_t *block_lens, const uint8_t *read_mask, int bitrot_algo,
    int data_only, int rehash, uint8_t *present_out, uint8_t *item_status);
mec_status mec_verify_reconstruct_batch_var(
    mec_ctx *ctx, int n, uint8_t *shards, uint8_t *sums,
    const int64_t *block_lens, const uint8_t *read_mask, int bitrot_algo,
    int data_only, int rehash, uint8_t *present_out, uint8_t *item_status);

/* ---- batch bitrot hash / verify ----------------------------------------
 * msgs: n messages of msg_len bytes at msg_stride; sums: n * hash_size.
 * verify: ok_out[i]=1 where digest matches want[i] (errFileCorrupt map).
 * The _dev entry is tested for msgs_dev 16-byte aligned and msg_stride a
 * multiple of 16 (SHA-256 and BLAKE2b-512 load 16 bytes at a time). */
mec_status mec_bitrot_sum_batch_dev(mec_ctx *ctx, int algo, int n,
                                    const void *msgs_dev, int64_t msg_len,
                                    int64_t msg_stride, void *sums_dev);
mec_status mec_bitrot_sum_batch(mec_ctx *ctx, int algo, int n,
                                const uint8_t *msgs, int64_t msg_len,
                                int64_t msg_stride, uint8_t *sums);
mec_status mec_bitrot_verify_batch(mec_ctx *ctx, int algo, int n,
                                   const uint8_t *msgs, int64_t msg_len,
                                   int64_t msg_stride, const uint8_t *want,
                                   uint8_t *ok_out);

/* bitrotVerify (cmd/bitrot.go:164-216): one [hash||shard]* stream (or whole
 * file for non-streaming algos).  Returns MEC_OK or MEC_ERR_FILE_CORRUPT. */
mec_status mec_bitrot_verify_stream(mec_ctx *ctx, const uint8_t *stream,
                                    int64_t want_size, int64_t part_size,
                                    int algo, const uint8_t *want_sum,
                                    int64_t shard_size);

/* ---- batch scrub: many on-disk shard files in one call -------------------
 *
 * xlStorage.VerifyFile -> bitrotVerify (cmd/xl-storage.go:3082-3137,
 * cmd/bitrot.go:164-216) over n shard files in the on-disk [hash||shard]*
 * format, each with its own size, part size and shard size: what the
 * scanner's deep scan and healObject run over every part of every object on
 * a drive.  The frames are hashed where they lie; nothing is re-packed.
 *
 *   files_dev   one device buffer of files_bytes bytes, never written.
 *   file_off    host, n: byte offset of file f in files_dev, ANY alignment
 *               (mec_scrub_file_offsets gives a convenient layout).
 *   file_sizes  host, n: bytes actually present (bitrotVerify's wantSize).
 *   part_sizes  host, n: erasure.ShardFileSize(part.Size), >= 0.
 *   shard_sizes host, n: erasure.ShardSize(), >= 1.
 *   bitrot_algo MEC_BITROT_HIGHWAYHASH256S only.
 *   file_status host, n: MEC_OK or MEC_ERR_FILE_CORRUPT per file.
 *   first_bad   host, n, may be NULL: the lowest failing frame index, the
 *               frame the reference stops at; -1 for an intact file.
 *
 * Per file, as bitrotVerify: if file_sizes[f] !=
 * mec_bitrot_shard_file_size(part_sizes[f], shard_sizes[f], HH256S) the file
 * is MEC_ERR_FILE_CORRUPT with first_bad -1 and nothing of it is hashed.
 * Otherwise it has ceil(part/shard) frames at pitch 32 + shard, each 32
 * digest bytes followed by the message, the last message of
 * part - (frames-1)*shard bytes; any mismatching frame makes the file
 * MEC_ERR_FILE_CORRUPT.  part_size 0 is MEC_OK with nothing hashed.  Bytes
 * outside a frame never influence its verdict.
 *
 * The call returns MEC_OK whatever the verdicts are: one corrupt file does
 * not fail the batch.  Argument errors (n <= 0, a NULL required pointer, a
 * negative size, shard_size < 1, file_off < 0,
 * file_off + file_size > files_bytes, another algorithm, more than 2^32-1
 * frames to hash) return MEC_ERR_INVALID_ARG before anything is launched and
 * before file_status or first_bad is written.  Independent of the context's
 * (d,p) and block size; n is not limited to 65535.  Synchronous, one stream
 * synchronise, no _async variant.
 *
 * The host-pointer variant takes one pointer per file (it may be NULL for a
 * file of size 0), packs the files at mec_scrub_file_offsets offsets into
 * pinned staging, uploads them in one plain copy and runs the device path.
 *
 * mec_scrub_file_offsets: pure host math, no context, no GPU.  F_0 = 0,
 * F_{f+1} = F_f + align64(file_sizes[f]); writes n+1 entries.
 * MEC_ERR_INVALID_ARG for n <= 0, a NULL pointer or a negative size. */
mec_status mec_scrub_file_offsets(int n, const int64_t *file_sizes,
                                  int64_t *file_off);
mec_status mec_bitrot_verify_files_dev(
    mec_ctx *ctx, int n, const void *files_dev, int64_t files_bytes,
    const int64_t *file_off, const int64_t *file_sizes,
    const int64_t *part_sizes, const int64_t *shard_sizes, int bitrot_algo,
    uint8_t *file_status, int64_t *first_bad);
mec_status mec_bitrot_verify_files(
    mec_ctx *ctx, int n, const uint8_t *const *files,
    const int64_t *file_sizes, const int64_t *part_sizes,
    const int64_t *shard_sizes, int bitrot_algo, uint8_t *file_status,
    int64_t *first_bad);

/* ---- streaming-format host mirrors (C++ host driver over the kernels) --
 *
 * mec_encode_stream: Erasure.Encode loop (cmd/erasure-encode.go:76-108)
 * fused with streamingBitrotWriter (cmd/bitrot-streaming.go:44-75): encodes
 * src (src_len bytes) into d+p per-drive streams in the on-disk
 * [hash||shard]* layout (HighwayHash256S) or raw shards (whole-file algos;
 * whole_sums then receives the d+p whole-file digests).  drive_bufs[i] must
 * hold mec_bitrot_shard_file_size(mec_shard_file_size(...), S, algo) bytes. */
mec_status mec_encode_stream(mec_ctx *ctx, const uint8_t *src,
                             int64_t src_len, int algo,
                             uint8_t *const *drive_bufs,
                             uint8_t *whole_sums);

/* mec_decode_stream: Erasure.Decode (cmd/erasure-decode.go:239-314) over
 * in-memory drive streams; NULL entries mark missing drives.  Verifies
 * every shard read (streamingBitrotReader.ReadAt), reconstructs when rows
 * are missing, writes [offset, offset+length) of the object into dst
 * (writeDataBlocks, cmd/erasure-utils.go:42-105).
 * whole_sums: for non-streaming algos, the d+p expected whole-file digests
 * (NULL entries skip verification), mirroring wholeBitrotReader. */
mec_status mec_decode_stream(mec_ctx *ctx, const uint8_t *const *drive_bufs,
                             const uint8_t *whole_sums, int algo,
                             int64_t total_length, int64_t offset,
                             int64_t length, uint8_t *dst);

/* mec_heal_stream: Erasure.Heal (cmd/erasure-decode.go:317-364): given any
 * >= d intact drive streams, regenerate the full set of d+p streams for the
 * missing drives (out_bufs[i] may be NULL to skip a drive). */
mec_status mec_heal_stream(mec_ctx *ctx, const uint8_t *const *drive_bufs,
                           int algo, int64_t total_length,
                           uint8_t *const *out_bufs);

/* ---- device memory + timing helpers (bench/test plumbing) ------------- */

mec_status mec_dev_alloc(mec_ctx *ctx, size_t bytes, void **out);
void mec_dev_free(mec_ctx *ctx, void *ptr);
mec_status mec_memcpy_h2d(mec_ctx *ctx, void *dst_dev, const void *src,
                          size_t bytes);
mec_status mec_memcpy_d2h(mec_ctx *ctx, void *dst, const void *src_dev,
                          size_t bytes);
mec_status mec_memset_dev(mec_ctx *ctx, void *dst_dev, int value,
                          size_t bytes);
mec_status mec_stream_sync(mec_ctx *ctx);
/* hipEvent timers on the context's stream (the stream kernels launch on). */
mec_status mec_timer_start(mec_ctx *ctx);
mec_status mec_timer_stop(mec_ctx *ctx, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* MINIO_EC_H */
