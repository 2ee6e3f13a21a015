"""GPU parity tests: the HIP path (libminio_ec_hip.so via the C-ABI) must
be bit-exact against the CPU oracle, which is itself pinned to the
reference's golden vectors (test_oracle_golden.py).

Covers (mirroring the reference's own test tables):
 - encode for every self-test geometry (d 2..14, p 1..8; cmd/erasure-coding.go:152)
 - the BASELINE.json config geometries at full shard sizes
 - all 4 bitrot algorithms incl. ragged tails (cmd/bitrot_test.go shapes)
 - reconstruct with every erasure pattern size (cmd/erasure-heal_test.go)
 - streaming [hash||shard]* round trips: encode -> decode/heal/verify
"""
import itertools
import json
import os
import random

import pytest

import minio_amd
import oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x6D696E696F


def rnd(n, seed):
    return oracle.fill_random(n, seed)


def all_geometries():
    out = []
    for total in range(4, 16):
        for d in range(total // 2, total):
            out.append((d, total - d))
    return out


def test_encode_parity_all_geometries_small():
    # block 4 KiB over every self-test geometry; sums checked too
    for d, p in all_geometries():
        bs = 4096
        data = rnd(bs, SEED + d * 31 + p)
        with minio_amd.Erasure(d, p, bs) as e:
            shards, sums = e.encode_batch(data, bs, 1, minio_amd.HIGHWAYHASH256S)
        ors = oracle.RS(d, p)
        oshards = ors.encode_data(data)
        assert shards[0] == oshards, f"d={d} p={p}"
        for s, sh in enumerate(oshards):
            assert sums[0][s] == oracle.bitrot_sum(oracle.HIGHWAYHASH256S, sh), \
                f"sum d={d} p={p} shard {s}"


@pytest.mark.parametrize("d,p,bs,algo", [
    (4, 2, 64 * 1024, minio_amd.HIGHWAYHASH256S),   # config #1 geometry
    (8, 4, 1 << 20, minio_amd.HIGHWAYHASH256S),     # config #2
    (12, 4, 1 << 20, minio_amd.SHA256),             # config #3 (ragged S)
    (16, 4, 4 << 20, minio_amd.HIGHWAYHASH256S),    # config #5
])
def test_encode_parity_baseline_configs(d, p, bs, algo):
    n = 4
    data = rnd(n * bs, SEED + bs + d)
    with minio_amd.Erasure(d, p, bs) as e:
        shards, sums = e.encode_batch(data, bs, n, algo)
    ors = oracle.RS(d, p)
    for b in range(n):
        blk = data[b * bs:(b + 1) * bs]
        oshards = ors.encode_data(blk)
        assert shards[b] == oshards, f"block {b}"
        for s, sh in enumerate(oshards):
            assert sums[b][s] == oracle.bitrot_sum(algo, sh)


def test_encode_ragged_last_block():
    # last block of an object: block_len < block_size -> smaller shard size
    d, p, bs = 8, 4, 1 << 20
    for blen in [1, 13, 4096, 999999]:
        data = rnd(blen, SEED + blen)
        with minio_amd.Erasure(d, p, bs) as e:
            shards, sums = e.encode_batch(data, blen, 1, minio_amd.HIGHWAYHASH256S)
        oshards = oracle.RS(d, p).encode_data(data)
        assert shards[0] == oshards, f"blen={blen}"
        for s, sh in enumerate(oshards):
            assert sums[0][s] == oracle.bitrot_sum(oracle.HIGHWAYHASH256S, sh)


def test_bitrot_sum_batch_all_algos_ragged():
    algos = [minio_amd.SHA256, minio_amd.HIGHWAYHASH256,
             minio_amd.HIGHWAYHASH256S, minio_amd.BLAKE2B512]
    with minio_amd.Erasure(4, 2, 4096) as e:
        # every mod-32 tail residue for the HH algos (UpdateRemainder has
        # distinct packet-builder paths for mod4 and the mod32&16 branch;
        # external ragged vectors are unobtainable offline — see DESIGN.md
        # §2 — so the oracle<->HIP cross-check must cover every residue)
        for mlen in range(64, 96):
            n = 4
            msgs = rnd(n * mlen, SEED * 3 + mlen)
            for algo in (minio_amd.HIGHWAYHASH256, minio_amd.HIGHWAYHASH256S):
                got = e.bitrot_sum_batch(algo, msgs, mlen, mlen, n)
                for i in range(n):
                    m = msgs[i * mlen:(i + 1) * mlen]
                    assert got[i] == oracle.bitrot_sum(algo, m), \
                        f"hh algo={algo} len={mlen} i={i}"
        for algo in algos:
            for mlen in [0, 1, 31, 32, 33, 55, 64, 100, 127, 128, 129,
                         1024, 87382]:
                n = 8
                stride = max(mlen, 1)
                msgs = rnd(n * stride, SEED + mlen + algo)
                got = e.bitrot_sum_batch(algo, msgs, mlen, stride, n)
                for i in range(n):
                    m = msgs[i * stride:i * stride + mlen]
                    assert got[i] == oracle.bitrot_sum(algo, m), \
                        f"algo={algo} len={mlen} i={i}"


def test_bitrot_sum_batch_hh_tail_after_prefetch_block():
    # 512 bytes are one full 16-packet prefetch block: every mod-32 tail
    # residue right after it, then the lengths around each edge of the
    # double-buffered loop (one block, two, three, four)
    lengths = list(range(512, 544)) + [1023, 1025, 1535, 1536, 1537,
                                       2047, 2048, 2049]
    n = 4
    with minio_amd.Erasure(4, 2, 4096) as e:
        for mlen in lengths:
            msgs = rnd(n * mlen, SEED * 5 + mlen)
            for algo in (minio_amd.HIGHWAYHASH256, minio_amd.HIGHWAYHASH256S):
                got = e.bitrot_sum_batch(algo, msgs, mlen, mlen, n)
                for i in range(n):
                    m = msgs[i * mlen:(i + 1) * mlen]
                    assert got[i] == oracle.bitrot_sum(algo, m), \
                        f"hh algo={algo} len={mlen} i={i}"


def test_reconstruct_parity_patterns():
    rng = random.Random(7)
    for d, p in [(4, 2), (8, 4), (12, 4), (6, 6)]:
        bs = 64 * 1024
        data = rnd(bs, SEED + d)
        ors = oracle.RS(d, p)
        oshards = ors.encode_data(data)
        with minio_amd.Erasure(d, p, bs) as e:
            for n_erase in range(1, p + 1):
                for _ in range(4):
                    erased = rng.sample(range(d + p), n_erase)
                    damaged = [None if i in erased else oshards[i]
                               for i in range(d + p)]
                    rec = e.decode_data_and_parity_blocks(damaged)
                    assert rec == oshards, f"d={d} p={p} erased={erased}"
                    damaged = [None if i in erased else oshards[i]
                               for i in range(d + p)]
                    rec = e.decode_data_blocks(damaged)
                    for i in range(d):
                        assert rec[i] == oshards[i]


def test_reconstruct_too_few_shards():
    with minio_amd.Erasure(4, 2, 4096) as e:
        shards = oracle.RS(4, 2).encode_data(rnd(4096, 1))
        damaged = [None, None, None] + shards[3:]
        with pytest.raises(minio_amd.MecError):
            e.decode_data_blocks(damaged)


def test_stream_roundtrip_vs_oracle():
    # encode_stream == oracle streams; decode returns original bytes
    d, p, bs = 4, 2, 4096
    total = 3 * bs + 1234  # ragged last block
    data = rnd(total, SEED + 5)
    with minio_amd.Erasure(d, p, bs) as e:
        streams, _ = e.encode_stream(data, minio_amd.HIGHWAYHASH256S)
        ostreams, _ = oracle.encode_stream(d, p, bs, data, oracle.HIGHWAYHASH256S)
        assert streams == ostreams
        # full read
        assert e.decode_stream(streams, total, 0, total) == data
        # ranged reads incl. cross-block and block-boundary-exact ends
        # (the reference iterates into an empty end block and breaks,
        #  cmd/erasure-decode.go:271-280)
        for off, ln in [(0, 1), (bs - 1, 2), (bs, bs), (100, 3 * bs),
                        (total - 1, 1), (bs + 7, 2 * bs + 100),
                        (0, bs), (0, 2 * bs), (bs, 2 * bs), (7, bs - 7)]:
            assert e.decode_stream(streams, total, off, ln) == data[off:off + ln]
        # with p drives missing
        dmg = list(streams)
        dmg[0] = None
        dmg[d] = None
        assert e.decode_stream(dmg, total, 0, total) == data
        # heal regenerates the exact streams
        healed = e.heal_stream(dmg, total)
        assert healed == streams


def test_stream_corruption_detected():
    d, p, bs = 4, 2, 4096
    total = 2 * bs
    data = rnd(total, SEED + 6)
    with minio_amd.Erasure(d, p, bs) as e:
        streams, _ = e.encode_stream(data)
        # flip one byte inside drive 1's second shard
        s = bytearray(streams[1])
        s[(32 + e.shard_size()) + 32 + 5] ^= 1
        dmg = list(streams)
        dmg[1] = bytes(s)
        # decode still succeeds via reconstruction (corrupt shard dropped)
        assert e.decode_stream(dmg, total, 0, total) == data
        # scrub flags the stream (bitrotVerify, cmd/bitrot.go:164-216)
        part_size = e.shard_file_size(total)
        assert not e.bitrot_verify_stream(bytes(s), part_size,
                                          minio_amd.HIGHWAYHASH256S)
        assert e.bitrot_verify_stream(streams[1], part_size,
                                      minio_amd.HIGHWAYHASH256S)
        # too many corrupt drives -> errFileCorrupt
        dmg2 = [None] * p + streams[p:]
        s2 = bytearray(streams[p])
        s2[40] ^= 255
        dmg2[p] = bytes(s2)
        with pytest.raises(minio_amd.MecError):
            e.decode_stream(dmg2, total, 0, total)


def test_whole_file_bitrot_roundtrip():
    # legacy whole-file algorithms (cmd/bitrot-whole.go)
    d, p, bs = 4, 2, 4096
    total = 2 * bs + 100
    data = rnd(total, SEED + 7)
    for algo in [minio_amd.SHA256, minio_amd.BLAKE2B512]:
        with minio_amd.Erasure(d, p, bs) as e:
            streams, sums = e.encode_stream(data, algo)
            assert e.decode_stream(streams, total, 0, total, algo, sums) == data
            # verify_stream with whole-file digest
            assert e.bitrot_verify_stream(streams[0], len(streams[0]), algo,
                                          want_sum=sums[0])
            bad = bytearray(streams[0]); bad[3] ^= 1
            assert not e.bitrot_verify_stream(bytes(bad), len(streams[0]),
                                              algo, want_sum=sums[0])


def test_bitrot_writer_reader_shapes():
    # mirror of TestAllBitrotAlgorithms (cmd/bitrot_test.go:25-83):
    # length 35, shardSize 10 -> shards 10,10,10,5
    with minio_amd.Erasure(4, 2, 4096) as e:
        msgs = b"a" * 35
        stream = b""
        for off in range(0, 35, 10):
            chunk = msgs[off:off + 10]
            h = oracle.bitrot_sum(oracle.HIGHWAYHASH256S, chunk)
            stream += h + chunk
        assert e.bitrot_verify_stream(stream, 35,
                                      minio_amd.HIGHWAYHASH256S,
                                      shard_size_=10)


def test_pipelined_encode_matches_oracle():
    # mec_encode_batch_dev_pipe (cross-batch overlap) must produce the
    # same parity+sums as the sequential path — the pipeline reorders
    # scheduling across calls, never the work of one call
    import ctypes
    d, p, bs, n = 8, 4, 1 << 20, 8
    lib = minio_amd._lib
    vp = ctypes.c_void_p
    with minio_amd.Erasure(d, p, bs) as e:
        ctx = e._ctx
        S = e.shard_size()
        stride = lib.mec_shard_stride(bs, d)

        def check(st):
            assert st == 0, lib.mec_last_error()

        data = rnd(n * bs, SEED + 99)
        # strided zero-padded layout (d | bs here so it is just packed)
        dev_data, dev_sum = vp(), vp()
        pars = [vp(), vp()]
        sums = [vp(), vp()]
        check(lib.mec_dev_alloc(ctx, n * d * stride, ctypes.byref(dev_data)))
        for i in range(2):
            check(lib.mec_dev_alloc(ctx, n * p * stride, ctypes.byref(pars[i])))
            check(lib.mec_dev_alloc(ctx, n * (d + p) * 32, ctypes.byref(sums[i])))
        check(lib.mec_memcpy_h2d(ctx, dev_data, data, n * d * stride))
        for step in range(4):
            check(lib.mec_encode_batch_dev_pipe(
                ctx, n, dev_data, bs, pars[step % 2], minio_amd.HIGHWAYHASH256S,
                sums[step % 2]))
        check(lib.mec_pipe_sync(ctx))
        ors = oracle.RS(d, p)
        for i in range(2):
            par = ctypes.create_string_buffer(n * p * stride)
            sm = ctypes.create_string_buffer(n * (d + p) * 32)
            check(lib.mec_memcpy_d2h(ctx, par, pars[i], n * p * stride))
            check(lib.mec_memcpy_d2h(ctx, sm, sums[i], n * (d + p) * 32))
            for b in range(n):
                shards = ors.encode_data(data[b * bs:(b + 1) * bs])
                for j in range(p):
                    got = par.raw[(b * p + j) * stride:(b * p + j) * stride + S]
                    assert got == shards[d + j], f"buf {i} blk {b} parity {j}"
                for s_i in range(d + p):
                    got = sm.raw[(b * (d + p) + s_i) * 32:(b * (d + p) + s_i + 1) * 32]
                    assert got == oracle.bitrot_sum(oracle.HIGHWAYHASH256S,
                                                    shards[s_i])


def test_concurrent_contexts_threads():
    # the C-ABI is re-entrant: calls arrive concurrently from many
    # goroutines in the reference — mirror with threads
    # driving two contexts on one device
    import threading
    errs = []

    def worker(seed):
        try:
            data = rnd(64 * 1024, seed)
            with minio_amd.Erasure(4, 2, 64 * 1024) as e:
                for _ in range(5):
                    shards, sums = e.encode_batch(data, 64 * 1024, 1,
                                                  minio_amd.HIGHWAYHASH256S)
                    want = oracle.RS(4, 2).encode_data(data)
                    assert shards[0] == want
        except Exception as ex:  # pragma: no cover
            errs.append(ex)

    ts = [threading.Thread(target=worker, args=(SEED + i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


def test_multiblock_object_stream():
    # a 10.5 MiB object at 1 MiB blocks: 10 full blocks + ragged last,
    # mirroring multipart part shapes (cmd/erasure-multipart.go:656-675)
    d, p, bs = 8, 4, 1 << 20
    total = 10 * bs + 524289
    data = rnd(total, SEED + 11)
    with minio_amd.Erasure(d, p, bs) as e:
        streams, _ = e.encode_stream(data)
        # spot-check stream layout against the oracle for 2 blocks
        ors = oracle.RS(d, p)
        S = e.shard_size()
        for b in (0, 10):
            blk = data[b * bs:(b + 1) * bs]
            oshards = ors.encode_data(blk)
            for s in (0, d, d + p - 1):
                off = b * (32 + S)
                sh = streams[s][off + 32:off + 32 + len(oshards[s])]
                assert sh == oshards[s], f"block {b} shard {s}"
        # ranged decode across the ragged tail
        assert e.decode_stream(streams, total, total - 70000, 70000) == \
            data[-70000:]
        assert e.decode_stream(streams, total, 0, total) == data
        # heal from d survivors only
        dmg = [None] * p + list(streams[p:])
        healed = e.heal_stream(dmg, total)
        assert healed == streams


def test_encode_parity_large_generic_geometries():
    # beyond the specialized list -> generic gf_matmul path (d<=32,
    # total<=40 per MEC_KMAX_*; the reference allows up to 256 shards,
    # deployments cap at 16 drives/set, docs/distributed/DESIGN.md:44-52)
    for d, p in [(20, 6), (32, 8), (17, 5)]:
        bs = 64 * 1024
        data = rnd(2 * bs, SEED + d * 7 + p)
        with minio_amd.Erasure(d, p, bs) as e:
            shards, sums = e.encode_batch(data, bs, 2,
                                          minio_amd.HIGHWAYHASH256S)
            ors = oracle.RS(d, p)
            want = ors.encode_data(data[:bs])
            assert shards[0] == want, f"d={d} p={p}"
            for s, sh in enumerate(want):
                assert sums[0][s] == oracle.bitrot_sum(
                    oracle.HIGHWAYHASH256S, sh)
            # and reconstruct with p erasures through the generic path
            damaged = [None] * p + want[p:]
            rec = e.decode_data_and_parity_blocks(damaged)
            assert rec == want
        # use-after-close must raise, not crash (the segfault this test
        # originally tripped: a NULL ctx reached the C-ABI)
        with pytest.raises(minio_amd.MecError):
            e.decode_data_and_parity_blocks(damaged)


def test_heal_with_corrupt_drive():
    # Heal reads through bitrot readers: a corrupt shard counts as missing
    # (cmd/erasure-decode.go:322 + bitrot-streaming.go:185-197); with >= d
    # intact shards per block the heal output is still exact
    d, p, bs = 4, 2, 4096
    total_len = 3 * bs + 777
    data = rnd(total_len, SEED + 21)
    with minio_amd.Erasure(d, p, bs) as e:
        streams, _ = e.encode_stream(data)
        S = e.shard_size()
        dmg = list(streams)
        dmg[0] = None  # missing drive to heal
        corrupt = bytearray(streams[2])
        corrupt[(32 + S) * 1 + 32 + 3] ^= 0xFF  # block 1 shard of drive 2
        dmg[2] = bytes(corrupt)
        healed = e.heal_stream(dmg, total_len)
        assert healed[0] == streams[0]  # regenerated exactly
        # too much loss in one block -> errFileCorrupt
        dmg2 = list(streams)
        dmg2[0] = None
        dmg2[1] = None
        c2 = bytearray(streams[2])
        c2[32 + 3] ^= 1  # block 0 of drive 2 -> only 3 intact < d
        dmg2[2] = bytes(c2)
        with pytest.raises(minio_amd.MecError):
            e.heal_stream(dmg2, total_len)


def test_decode_random_offsets_fuzz():
    # mirrors the random-offset fuzz at cmd/erasure-decode_test.go:200
    d, p, bs = 8, 4, 64 * 1024
    total_len = 7 * bs + 31415
    data = rnd(total_len, SEED + 22)
    rng = random.Random(99)
    with minio_amd.Erasure(d, p, bs) as e:
        streams, _ = e.encode_stream(data)
        for _ in range(40):
            off = rng.randrange(total_len)
            ln = rng.randrange(1, total_len - off + 1)
            dmg = list(streams)
            for s in rng.sample(range(d + p), rng.randrange(0, p + 1)):
                dmg[s] = None
            assert e.decode_stream(dmg, total_len, off, ln) == \
                data[off:off + ln], f"off={off} len={ln}"


def test_fullsize_roundtrip_batch():
    # full BASELINE shard sizes, encode -> erase p -> reconstruct, batch 16
    for d, p, bs in [(8, 4, 1 << 20), (16, 4, 4 << 20)]:
        n = 16
        data = rnd(n * bs, SEED + 23 + d)
        with minio_amd.Erasure(d, p, bs) as e:
            shards, sums = e.encode_batch(data, bs, n, minio_amd.HIGHWAYHASH256S)
            for b in (0, n - 1):
                damaged = list(shards[b])
                for i in range(p):
                    damaged[d - 1 - i] = None  # erase p rows spanning data
                rec = e.decode_data_and_parity_blocks(damaged)
                assert rec == shards[b]


def test_chunked_overlap_paths_large_batches():
    """The host-pointer reconstruct (n>128) and bitrot-sum (n>512) paths
    chunk the batch and pipeline host pack + PCIe upload under the
    previous chunk's kernels.  Pin bit-exactness across the
    chunk boundaries, including a batch size that is not a multiple of
    the chunk count."""
    import ctypes
    d, p, total = 4, 2, 6
    S = 1024
    n = 203  # > 128 -> chunked; 203 % 4 != 0 -> ragged last chunk
    ors = oracle.RS(d, p)
    blocks = []
    packed = bytearray()
    for b in range(n):
        data = rnd(d * S, SEED + b)
        ds = [data[i * S:(i + 1) * S] for i in range(d)]
        shards = ds + ors.encode_blocks(ds)
        blocks.append(shards)
        for s in range(total):
            packed += shards[s]
    present = bytes([0, 1, 1, 1, 0, 1])  # rows 0 and 4 erased
    buf = ctypes.create_string_buffer(bytes(packed), len(packed))
    for b in range(n):
        for s in range(total):
            if not present[s]:
                off = (b * total + s) * S
                ctypes.memset(ctypes.byref(buf, off), 0, S)
    with minio_amd.Erasure(d, p, d * S) as e:
        minio_amd._check(minio_amd._lib.mec_reconstruct_batch(
            e._ck(), n, buf, present, S, 0))
        out = buf.raw
        for b in range(n):
            for s in range(total):
                off = (b * total + s) * S
                assert out[off:off + S] == blocks[b][s], (b, s)

        # chunked bitrot-sum: 600 ragged messages in a strided layout
        nmsg, mlen, mstride = 600, 549, 576
        msgs = bytearray(nmsg * mstride)
        for i in range(nmsg):
            msgs[i * mstride:i * mstride + mlen] = rnd(mlen, SEED ^ i)
        sums = e.bitrot_sum_batch(minio_amd.HIGHWAYHASH256S, bytes(msgs),
                                  mlen, mstride, nmsg)
        for i in range(nmsg):
            want = oracle.bitrot_sum(
                oracle.HIGHWAYHASH256S,
                bytes(msgs[i * mstride:i * mstride + mlen]))
            assert sums[i] == want, i


def test_stream_boundary_cases():
    """Deterministic edges from the reference's decode table
    (cmd/erasure-decode_test.go:35-85): tiny objects (< one shard, < d
    bytes), exact block-boundary offsets, single-byte reads at both ends,
    and zero-length reads.  Streams are also pinned against the oracle's
    writer byte-for-byte."""
    d, p, bs = 4, 2, 8192
    with minio_amd.Erasure(d, p, bs) as e:
        for total_len in (1, 3, d - 1, d, 37, bs - 1, bs, bs + 1,
                          2 * bs, 2 * bs + 17):
            data = rnd(total_len, SEED ^ total_len)
            streams, _ = e.encode_stream(data)
            ostreams, _ = oracle.encode_stream(d, p, bs, data,
                                               oracle.HIGHWAYHASH256S)
            assert list(streams) == list(ostreams), total_len
            cases = {(0, total_len), (0, 1), (total_len - 1, 1), (0, 0)}
            if total_len > bs:
                cases |= {(bs, total_len - bs), (bs - 1, 2), (bs, 1)}
            for off, ln in sorted(cases):
                got = e.decode_stream(list(streams), total_len, off, ln)
                assert got == data[off:off + ln], (total_len, off, ln)

    # ragged odd-pitch geometries with FULL blocks: odd S makes the
    # per-entry pitch (32+S) odd, so the stream-out region's byte count is
    # not 16-B aligned — the device row buffer placed after it must round
    # up to keep the row kernels' uint4 alignment invariant (regression:
    # scatter/interleave used misaligned uint4 at d=4,p=2,S=10)
    # (3,2,144): S=48 -> stride 64; the interleave's 16-B gather window
    # would read past the row stride on the final units without its
    # base+32<=stride guard
    for (d2, p2, bs2) in ((4, 2, 40), (3, 2, 51), (3, 2, 144)):
        with minio_amd.Erasure(d2, p2, bs2) as e2:
            for nfull in (1, 2, 5):
                total_len = nfull * bs2 + 7
                data = rnd(total_len, SEED ^ (d2 * 131 + total_len))
                streams, _ = e2.encode_stream(data)
                ostreams, _ = oracle.encode_stream(d2, p2, bs2, data,
                                                   oracle.HIGHWAYHASH256S)
                assert list(streams) == list(ostreams), (d2, p2, nfull)
                got = e2.decode_stream(list(streams), total_len, 0, total_len)
                assert got == data, (d2, p2, nfull)


def test_reconstruct_exhaustive_patterns_ec84():
    """Every erasure pattern the EC8+4 geometry can see: all C(12,k)
    combinations for k=1..4 (793 patterns), reconstructed bit-exactly
    (cmd/erasure-heal_test.go covers a sample; the GPU batch path is
    cheap enough to cover them all)."""
    d, p, total = 8, 4, 12
    bs = d * 1024
    data = rnd(bs, SEED + 84)
    ors = oracle.RS(d, p)
    oshards = ors.encode_data(data)
    with minio_amd.Erasure(d, p, bs) as e:
        for k in range(1, p + 1):
            for erased in itertools.combinations(range(total), k):
                damaged = [None if i in erased else oshards[i]
                           for i in range(total)]
                rec = e.decode_data_and_parity_blocks(damaged)
                assert rec == oshards, f"erased={erased}"


def test_empty_object_paths():
    """0-length objects: encode produces empty streams, decode of a
    zero-length range succeeds, heal is a no-op (regression: the
    ragged-last verify used to index block -1 for total_length==0)."""
    d, p = 4, 2
    with minio_amd.Erasure(d, p, 4096) as e:
        streams, _ = e.encode_stream(b"")
        assert all(s == b"" for s in streams)
        assert e.decode_stream(list(streams), 0, 0, 0) == b""
        dmg = list(streams)
        dmg[0] = None
        healed = e.heal_stream(dmg, 0)
        assert healed[0] == b""
        # whole-file algo on an empty object still produces digests
        wstreams, wsums = e.encode_stream(b"", minio_amd.SHA256)
        assert all(s == b"" for s in wstreams)
        assert wsums is not None and len(wsums) == d + p
        assert wsums[0] == oracle.bitrot_sum(oracle.SHA256, b"")


# ---- live and retired knobs (env-latched -> subprocess) -----------------

_KNOB_CHECK = r"""
import os, sys
sys.path.insert(0, os.environ["MEC_TEST_REPO"])
import minio_amd, oracle
SEED = 0x6D696E696F
d, p, bs = 8, 4, 64 * 8 * 1024   # S = 64 KiB: %1024==0 (fused2), >=512 (LDS)
with minio_amd.Erasure(d, p, bs) as e:
    for n, seed in ((7, 1), (32, 2)):
        blocks = [oracle.fill_random(bs, SEED + seed * 100 + b)
                  for b in range(n)]
        shards, sums = e.encode_batch(b"".join(blocks), bs, n,
                                      minio_amd.HIGHWAYHASH256S)
        ors = oracle.RS(d, p)
        for b in range(n):
            osh = ors.encode_data(blocks[b])
            assert shards[b] == osh, b
            for s in range(d + p):
                want = oracle.bitrot_sum(oracle.HIGHWAYHASH256S, osh[s])
                assert sums[b][s] == want, (b, s)
    # ragged message lengths through the knob'd hash kernel too
    msgs = b"".join(oracle.fill_random(577, SEED + i) for i in range(65))
    sums = e.bitrot_sum_batch(minio_amd.HIGHWAYHASH256S, msgs, 577, 577, 65)
    for i in range(65):
        assert sums[i] == oracle.bitrot_sum(
            oracle.HIGHWAYHASH256S, msgs[i * 577:(i + 1) * 577]), i
    # SHA leg (covers the MEC_SHA_* launch variants)
    smsgs = b"".join(oracle.fill_random(2048, SEED * 2 + i) for i in range(40))
    ssums = e.bitrot_sum_batch(minio_amd.SHA256, smsgs, 2048, 2048, 40)
    for i in range(40):
        assert ssums[i] == oracle.bitrot_sum(
            oracle.SHA256, smsgs[i * 2048:(i + 1) * 2048]), i
print("KNOB_OK")
"""


# Run after _KNOB_CHECK in the same process when a retired knob is set: the
# knob must be ignored.  Until commit 762fd47 the presence of an encode
# experiment knob silently sent every batch to the kernel pair; now an
# eligible batch (MEC_F4_MIN is read per context) must still take the one-pass
# kernel, once, and match both the oracle and the pair
# (test_gpu_fused4.encode_case asserts all three).
_KNOB_IGNORED_CHECK = r"""
sys.path.insert(0, os.path.join(os.environ["MEC_TEST_REPO"], "tests"))
os.environ["MEC_F4_MIN"] = "1"
import test_gpu_fused4 as t
t.encode_case(5, t.DP * t.T, t.D * t.DP * t.T, True)
print("KNOB_IGNORED_OK")
"""

# Retired knobs, one per deleted kernel family, with the value
# that used to select the experiment.  The library no longer reads them.
_RETIRED_KNOBS = {
    "MEC_HH_LDS": {"MEC_HH_LDS": "1"},
    "MEC_FUSED2": {"MEC_FUSED2": "1"},
    "MEC_FUSED": {"MEC_FUSED": "1"},
    "MEC_FUSED3": {"MEC_FUSED3": "1"},
    "MEC_HH_WG": {"MEC_HH_WG": "512"},
    "MEC_HH4_OFF": {"MEC_HH4": "0"},
    "MEC_SHA_WG": {"MEC_SHA_WG": "512"},
    "MEC_GF_BS_OFF": {"MEC_GF_BS": "0"},
}


@pytest.mark.parametrize("knob", ["default", "MEC_FUSED4=0",
                                  *_RETIRED_KNOBS])
def test_knob_variants_bit_exact(knob):
    """Knobs are env-latched at first use, so each setting runs in a
    subprocess, started with every MEC_* variable removed: `default` adds
    nothing (what a caller gets: the library's own choice between the
    one-pass kernel and the kernel pair), `MEC_FUSED4=0` takes the kernel
    pair everywhere, and each retired knob is set to the value that used to
    select its experiment.  Every run must be bit-exact vs the oracle, the
    ragged HighwayHash and the SHA launches included; under a retired knob
    the one-pass kernel must in addition still take an eligible batch
    (_KNOB_IGNORED_CHECK), which it did not while the knob was read."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if not k.startswith("MEC_")}
    script, marks = _KNOB_CHECK, ["KNOB_OK"]
    if knob in _RETIRED_KNOBS:
        env.update(_RETIRED_KNOBS[knob])
        script += _KNOB_IGNORED_CHECK
        marks.append("KNOB_IGNORED_OK")
    elif knob != "default":
        name, value = knob.split("=")
        env[name] = value
    env["MEC_TEST_REPO"] = os.path.dirname(HERE)
    r = subprocess.run([os.environ.get("PYTHON", "python3"), "-c", script],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and all(m in r.stdout for m in marks), (
        knob, r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_stream_pipeline_fuzz_geometries():
    """Randomized (deterministic-seed) full-pipeline fuzz across
    geometries the fixed tables don't enumerate: encode_stream -> ranged
    decode -> corruption -> decode-around-corruption -> heal, each
    byte-compared against the oracle or the original data."""
    rng = random.Random(0xF022)
    cases = []
    n_cases = int(os.environ.get("MEC_FUZZ_CASES", "10"))
    for _ in range(n_cases):
        d = rng.randint(2, 16)
        p = rng.randint(1, min(8, d))
        bs = rng.choice([d * rng.randint(100, 5000),
                         rng.choice([4096, 65536, 131072])])
        total_len = rng.randint(1, 3 * bs + rng.randint(0, bs))
        cases.append((d, p, bs, total_len))
    for (d, p, bs, total_len) in cases:
        data = rnd(total_len, SEED ^ (d * 1009 + p * 131 + total_len))
        with minio_amd.Erasure(d, p, bs) as e:
            streams, _ = e.encode_stream(data)
            ostreams, _ = oracle.encode_stream(d, p, bs, data,
                                               oracle.HIGHWAYHASH256S)
            assert list(streams) == list(ostreams), (d, p, bs, total_len)
            for _ in range(3):
                off = rng.randint(0, max(0, total_len - 1))
                ln = rng.randint(0, total_len - off)
                got = e.decode_stream(list(streams), total_len, off, ln)
                assert got == data[off:off + ln], (d, p, bs, total_len, off,
                                                   ln)
            # corrupt up to p-1 drives (flip a byte each), decode whole
            n_bad = rng.randint(0, max(0, p - 1))
            dmg = list(streams)
            for s in rng.sample(range(d + p), n_bad):
                if len(dmg[s]) == 0:
                    continue
                buf = bytearray(dmg[s])
                buf[rng.randrange(len(buf))] ^= 0xFF
                dmg[s] = bytes(buf)
            got = e.decode_stream(dmg, total_len, 0, total_len)
            assert got == data, (d, p, bs, total_len, "corrupt", n_bad)
            # heal one missing drive back to the exact stream
            if total_len > 0:
                miss = rng.randrange(d + p)
                dmg2 = list(streams)
                dmg2[miss] = None
                healed = e.heal_stream(dmg2, total_len)
                assert healed[miss] == streams[miss], (d, p, bs, total_len,
                                                       miss)


def test_encode_linearity_full_size_gpu():
    """Linearity of the HIP encode at the full headline geometry:
    encode(x^y) == encode(x)^encode(y) for EC8+4 at 1 MiB blocks — a
    size-independent property covering the full-size path beyond the
    oracle cross-checks."""
    d, p, bs = 8, 4, 1 << 20
    x = rnd(bs, SEED + 0xA)
    y = rnd(bs, SEED + 0xB)
    xy = bytes(a ^ b for a, b in zip(x, y))
    with minio_amd.Erasure(d, p, bs) as e:
        sx, _ = e.encode_batch(x, bs, 1)
        sy, _ = e.encode_batch(y, bs, 1)
        sxy, _ = e.encode_batch(xy, bs, 1)
    for s in range(d + p):
        want = bytes(a ^ b for a, b in zip(sx[0][s], sy[0][s]))
        assert sxy[0][s] == want, s
