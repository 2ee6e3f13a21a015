/* Kernel argument structs shared between ec_abi.cpp (host) and kernels.hip.
 * Internal to the library — the public boundary is include/minio_ec.h. */
#ifndef MEC_KERNELS_H
#define MEC_KERNELS_H

#include <hip/hip_runtime.h>
#include <cstdint>

/* Kernel-side geometry caps: MinIO erasure sets are 2..16 drives
 * (docs/distributed/DESIGN.md:44-52); the self-test sweeps d<=14, p<=8
 * (cmd/erasure-coding.go:152-156).  We allow headroom. */
#define MEC_KMAX_D 32
#define MEC_KMAX_E 8  /* output rows per launch; larger p uses multiple */
#define MEC_KMAX_TOTAL 40

struct GfMatmulArgs {
    const uint8_t *src;      /* batch base of source rows */
    uint8_t *dst;            /* batch base of destination rows */
    int64_t src_item_stride; /* bytes between batch items in src */
    int64_t dst_item_stride;
    int64_t row_stride;      /* bytes between shard rows (64-aligned) */
    int64_t shard_len;       /* valid bytes per shard */
    int d;                   /* number of source rows */
    uint8_t src_rows[MEC_KMAX_D];
    uint8_t dst_rows[MEC_KMAX_E];
    uint8_t mat[MEC_KMAX_E * MEC_KMAX_D]; /* row t: coefficients over src */
    /* bit-sliced path (r2): device pointer to E*d*2 u32 —
     * bs_masks[(t*d+k)*2 + w] = dword w of the 8x8 bit matrix of
     * mat[t][k] (byte b = rowmask(c,b): bit a set iff output bit b of
     * c*x depends on input bit a).  Required: NULL is refused. */
    const uint32_t *bs_masks;
};

/* Mixed-pattern reconstruct (recon_mixed.hip): rows, destinations and bit
 * matrices come per work item from a device-resident plan table instead
 * of the kernel arguments.  Table layouts: recon_plan.h. */
struct GfMixedArgs {
    uint8_t *shards;         /* batch base, rebuilt in place */
    int64_t item_stride;     /* bytes between batch items */
    int64_t row_stride;      /* bytes between shard rows (64-aligned) */
    int64_t shard_len;       /* valid bytes per shard */
    const uint32_t *entries; /* plan table, 12 dwords per entry */
    const uint32_t *masks;   /* packed bit matrices, all entries */
    const uint32_t *work;    /* this launch's list: (item, entry) pairs */
    uint32_t n_work;         /* pairs in the list */
    uint32_t blocks_x;       /* column blocks per pair */
    int d;                   /* number of source rows */
};

/* mode: which shard rows this launch hashes. Sums always land in the
 * fused n x (d+p) x digest layout so a data-only and a parity-only launch
 * together produce exactly the single-launch result. */
enum MecHashMode { MEC_HASH_ALL = 0, MEC_HASH_DATA = 1, MEC_HASH_PARITY = 2 };

struct HashArgs {
    const uint8_t *data;   /* data-shard rows, n*d*row_stride */
    const uint8_t *parity; /* parity rows, n*p*row_stride; NULL => simple
                              strided layout: chain i at data+i*row_stride */
    uint8_t *sums;         /* n * (d+p) * digest_size (fused layout) */
    int64_t row_stride;
    int64_t msg_len;       /* bytes hashed per chain (the padded shard) */
    int64_t n_chains;      /* chains in THIS launch: n*(d+p), n*d or n*p */
    int d, p;
    int mode;              /* MecHashMode */
    uint64_t key[4];       /* HighwayHash key (little-endian words) */
};

/* List-driven HighwayHash-256 (hh_list.hip): the chains to hash are named
 * by a device-resident id list instead of being 0..n_chains-1.  Chain id c
 * is the row at shards + c*row_stride with its digest slot at sums + c*32
 * (the fused n x (d+p) x 32 layout when c = item*(d+p)+row).
 * verify mode compares against the slot and stores ok[c] = 0/1;
 * sum mode writes the digest into the slot. */
struct HashListArgs {
    const uint8_t *shards;
    uint8_t *sums;        /* verify: read only; sum: written */
    uint8_t *ok;          /* verify only: one byte per chain ID */
    const uint32_t *list; /* n_list chain ids */
    uint32_t n_list;
    int64_t row_stride;
    int64_t msg_len;      /* bytes hashed per chain, same for all */
    uint64_t key[4];
};

/* Verified read with a shard length per item (read_var.hip).  The packed
 * layout is var_plan.h's with all d+p rows of an item together: row s of
 * item i at shards + total*R_i + s*align64(S_i).  Tables: read_var_plan.h. */
struct GfMixedVarArgs {
    uint8_t *shards;         /* total*R_n bytes, rebuilt in place */
    const int64_t *items;    /* 2 per item: R_i, S_i (mec::VarItem) */
    const uint32_t *entries; /* plan table, 12 dwords per entry */
    const uint32_t *masks;   /* packed bit matrices, all entries */
    const uint32_t *work;    /* this launch's list: (item, entry) pairs */
    const int64_t *tiles;    /* n_work+1: tile prefix T_0..T_m of the list */
    int64_t tiles_total;     /* T_m */
    uint32_t n_work;         /* pairs in the list */
    int d;                   /* number of source rows */
    int total;               /* d+p */
};

struct HashListVarArgs {
    const uint8_t *shards;
    uint8_t *sums;        /* verify: read only; sum: written */
    uint8_t *ok;          /* verify only: one byte per chain ID */
    const uint32_t *list; /* n_list chain ids, item*total+row */
    const int64_t *items; /* 2 per item: R_i, S_i */
    uint32_t n_list;
    uint32_t total;       /* d+p */
    uint64_t key[4];
};

/* Batch scrub (hh_frames.hip): chains are frames of on-disk shard files,
 * hashed where they lie.  Chain c = list[2c], list[2c+1] = (file, frame);
 * file f's table row is 4 qwords (mec::ScrubFile: off, shard, last,
 * frames).  The frame starts at files + off + frame*(32+shard): 32 digest
 * bytes, then the message.  ok[c] = 1 where the digest matches.  Tables:
 * scrub_plan.h. */
struct HashFramesArgs {
    const uint8_t *files; /* never written */
    const int64_t *table; /* 4 qwords per file */
    const uint32_t *list; /* 2 dwords per chain */
    uint8_t *ok;          /* one byte per chain, in list order */
    uint32_t n_list;
    uint64_t key[4];
};

/* Specialized-encode args (constexpr-matrix kernels) */
struct GfEncArgs {
    const uint8_t *data;
    uint8_t *parity;
    int64_t row_stride;
    int64_t shard_len;
};

/* Encode with a block length per item (encode_var.hip).  The packed layout
 * and the three tables are the planner's: var_plan.h. */
struct EncVarArgs {
    const uint8_t *data;    /* d * R_n */
    uint8_t *parity;        /* p * R_n (output) */
    uint8_t *sums;          /* n * (d+p) * 32 (output); NULL: encode only */
    const int64_t *items;   /* 2 per item: R_i, S_i (mec::VarItem) */
    const int64_t *col_off; /* n+1: prefix of 32-byte column counts */
    const uint32_t *order;  /* n: items by descending S_i (hash order) */
    int64_t cols_total;     /* col_off[n] */
    uint32_t n;
    int d, p;
    uint64_t key[4];
};

/* Pack rows and digests into on-disk [hash||shard] frames
 * (encode_frames.hip).  Input: EncVarArgs' data, parity and sums after
 * mec_launch_encode_var.  Output layout: frames_plan.h; the mapping from an
 * output granule to its source: frames_map.h. */
struct FramesPackArgs {
    const uint8_t *data;      /* d * R_n, 16-aligned */
    const uint8_t *parity;    /* p * R_n, 16-aligned */
    const uint8_t *sums;      /* n * (d+p) * 32 */
    uint8_t *out;             /* (d+p) * F_n bytes, any alignment */
    const int64_t *items;     /* 2 per item: R_i, S_i (mec::VarItem) */
    const int64_t *frame_off; /* n+1: F_0..F_n */
    int64_t fn;               /* F_n */
    int64_t bytes;            /* (d+p) * F_n */
    int64_t granules;         /* ceil((a0 + bytes) / 16) */
    int64_t groups;           /* ceil(granules / 64); the launcher fills it */
    int64_t per_wave;         /* consecutive groups per wave; the launcher's */
    uint32_t n;
    uint32_t a0;              /* out address % 16 */
    int d, p;
};

/* Fused single-pass encode+HighwayHash (fused4.hip) */
struct FusedArgs {
    const uint8_t *data; /* n * d * row_stride */
    uint8_t *parity;     /* n * p * row_stride (output) */
    uint8_t *sums;       /* n * (d+p) * 32 (output) */
    int64_t row_stride;
    int64_t shard_len;
    int64_t n;
    uint64_t key[4];
    int probe; /* 0 normal; perf-isolation bits (results INVALID), set by
                  the launcher from MEC_F4_PROBE: 1 hash waves idle,
                  2 GF waves idle, 4 loader issues nothing */
};

struct ScatterArgs {
    const uint8_t *src;
    uint8_t *rows;
    int64_t block_len;
    int64_t S;
    int64_t row_stride;
    int64_t n;
    int d;
};

struct InterleaveArgs {
    const uint8_t *data;
    const uint8_t *parity;
    const uint8_t *sums;
    uint8_t *out;
    int64_t S;
    int64_t row_stride;
    int64_t n;
    int d, p;
};

extern "C" {
hipError_t mec_launch_scatter_rows(const ScatterArgs *args,
                                   hipStream_t stream);
hipError_t mec_launch_stream_interleave(const InterleaveArgs *args,
                                        hipStream_t stream);
/* one-pass kernel of fused4.hip; hipErrorNotSupported, with nothing
 * launched, when the shape is not eligible or a knob turns it off */
hipError_t mec_launch_fused4_encode_hh(int d, int p, const FusedArgs *args,
                                       hipStream_t stream);
/* fused4 launches by this process so far: lets a test tell the one-pass
 * kernel from the pair, whose results are the same */
uint64_t mec_fused4_launches(void);
hipError_t mec_launch_gf_matmul(const GfMatmulArgs *args, int n_dst, int n,
                                hipStream_t stream);
/* one launch per output-row count n_dst (1..MEC_KMAX_E); fills
 * args->blocks_x itself */
hipError_t mec_launch_gf_matmul_mixed(const GfMixedArgs *args, int n_dst,
                                      hipStream_t stream);
hipError_t mec_launch_gf_encode_spec(int d, int p, const GfEncArgs *args,
                                     int n, hipStream_t stream);
/* 1 when (d,p) has a compiled gf_encode_bs_var_kernel specialization */
int mec_encode_var_supported(int d, int p);
/* gf_encode_bs_var_kernel, then hh256_var_kernel unless args->sums is NULL;
 * hipErrorNotSupported, with nothing launched, for an unspecialized (d,p) */
hipError_t mec_launch_encode_var(const EncVarArgs *args, hipStream_t stream);
/* frames_pack_var_kernel over args->granules output granules */
hipError_t mec_launch_frames_pack(const FramesPackArgs *args,
                                  hipStream_t stream);
hipError_t mec_launch_hash(int algo, const HashArgs *args, hipStream_t stream);
/* HighwayHash-256 over args->list; verify != 0 selects hh256_list_verify,
 * else hh256_list_sum.  n_list == 0 launches nothing. */
hipError_t mec_launch_hash_list(const HashListArgs *args, int verify,
                                hipStream_t stream);
/* gf_matmul_bs_mixed_var_kernel<n_dst> over args->tiles_total tiles;
 * n_work == 0 launches nothing */
hipError_t mec_launch_gf_matmul_mixed_var(const GfMixedVarArgs *args,
                                          int n_dst, hipStream_t stream);
/* hh256_list_var_verify (verify != 0) or hh256_list_var_sum over
 * args->list; n_list == 0 launches nothing */
hipError_t mec_launch_hash_list_var(const HashListVarArgs *args, int verify,
                                    hipStream_t stream);
/* hh256_frames_verify (sheared == 0: every message address of the list is a
 * multiple of 8) or hh256_frames_verify_sheared (none is) over args->list;
 * n_list == 0 launches nothing */
hipError_t mec_launch_hash_frames(const HashFramesArgs *args, int sheared,
                                  hipStream_t stream);
}

#endif
