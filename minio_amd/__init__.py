"""minio_amd — MI355X-native implementation of MinIO's erasure-coding +
bitrot hot path.

The product boundary is the C-ABI in include/minio_ec.h, implemented by
libminio_ec_hip.so (HIP/gfx950 kernels + C++ host drivers).  This package is
a thin ctypes veneer over that boundary, mirroring the reference's Go
surfaces 1:1 for tests and benchmarks:

  - Erasure             <-> cmd/erasure-coding.go:35-141 (NewErasure,
                            EncodeData, DecodeDataBlocks,
                            DecodeDataAndParityBlocks, ShardSize,
                            ShardFileSize, ShardFileOffset)
  - Erasure.encode_stream / decode_stream / heal_stream
                        <-> Erasure.Encode / Decode / Heal
                            (cmd/erasure-encode.go:76, erasure-decode.go:239,
                             :317) over the streaming bitrot on-disk layout
                            (cmd/bitrot-streaming.go)
  - Erasure.encode_batch_var, var_row_offsets
                        <-> EncodeData for many blocks in one call, each
                            with its own length (a PUT batch across
                            objects: Erasure.Encode encodes whatever
                            io.ReadFull returned, cmd/erasure-encode.go:
                            76-108; mec_encode_batch_var)
  - Erasure.encode_frames_batch_var, frame_offsets
                        <-> the same batch written as streamingBitrotWriter
                            writes it: one [hash||shard] frame per block in
                            each of the d+p row streams
                            (cmd/bitrot-streaming.go:44-75;
                             mec_encode_frames_batch_var)
  - Erasure.reconstruct_batch
                        <-> DecodeDataBlocks / DecodeDataAndParityBlocks
                            for many blocks in one call, each with its own
                            erasure pattern (a cross-object degraded read
                            or heal; mec_reconstruct_batch_mixed)
  - Erasure.verify_reconstruct_batch
                        <-> streamingBitrotReader.ReadAt + parallelReader.Read
                            + Decode/Heal for many blocks in one call: rows
                            that fail their bitrot check count as missing
                            (cmd/bitrot-streaming.go:161-200,
                             cmd/erasure-decode.go:127-235;
                             mec_verify_reconstruct_batch)
  - Erasure.verify_reconstruct_batch_var
                        <-> the same with a shard length per item: the last
                            block of every object is short
                            (cmd/erasure-decode.go:138-139;
                             mec_verify_reconstruct_batch_var)
  - bitrot_verify       <-> bitrotVerify (cmd/bitrot.go:164-216)

No CPU fallback exists: constructing an Erasure on a machine without a
visible GPU raises NoGPUError (MEC_ERR_NO_GPU).  The host-side mirrors of
the shard-size math are pure integer functions and work anywhere.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libminio_ec_hip.so")

# Bitrot algorithm ids (cmd/xl-storage-format-v1.go:146-153)
SHA256 = 1
HIGHWAYHASH256 = 2
HIGHWAYHASH256S = 3
BLAKE2B512 = 4
DEFAULT_BITROT_ALGORITHM = HIGHWAYHASH256S

_HASH_SIZE = {SHA256: 32, HIGHWAYHASH256: 32, HIGHWAYHASH256S: 32, BLAKE2B512: 64}

# mec_status values (include/minio_ec.h)
MEC_OK = 0
_STATUS_NAMES = {
    1: "ErrInvShardNum",
    2: "ErrMaxShardNum",
    3: "ErrTooFewShards",
    4: "ErrShortData",
    5: "errFileCorrupt",
    6: "InvalidArgument",
    7: "HIPError",
    8: "NoGPU",
}


class MecError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        name = _STATUS_NAMES.get(status, str(status))
        super().__init__(f"minio_ec: {name}{(': ' + detail) if detail else ''}")


class FileCorruptError(MecError):
    pass


class NoGPUError(MecError):
    pass


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} not built — run `make -C minio_amd/csrc` "
            "(or __graft_entry__.build()).  The product path requires the "
            "HIP extension; there is no fallback."
        )
    lib = ctypes.CDLL(_LIB_PATH)
    c = ctypes
    i64, i32, sz = c.c_int64, c.c_int, c.c_size_t
    u8p, vp = c.c_char_p, c.c_void_p
    lib.mec_last_error.restype = c.c_char_p
    lib.mec_shard_size.restype = i64
    lib.mec_shard_size.argtypes = [i64, i32]
    lib.mec_shard_file_size.restype = i64
    lib.mec_shard_file_size.argtypes = [i64, i32, i64]
    lib.mec_shard_file_offset.restype = i64
    lib.mec_shard_file_offset.argtypes = [i64, i32, i64, i64, i64]
    lib.mec_bitrot_shard_file_size.restype = i64
    lib.mec_bitrot_shard_file_size.argtypes = [i64, i64, i32]
    lib.mec_shard_stride.restype = i64
    lib.mec_shard_stride.argtypes = [i64, i32]
    lib.mec_ctx_create.argtypes = [i32, i32, i64, i32, c.POINTER(vp)]
    lib.mec_ctx_destroy.argtypes = [vp]
    lib.mec_encode_batch.argtypes = [vp, i32, u8p, i64, u8p, i32, u8p]
    lib.mec_encode_batch_dev.argtypes = [vp, i32, vp, i64, vp, i32, vp]
    lib.mec_encode_batch_dev_async.argtypes = [vp, i32, vp, i64, vp, i32, vp]
    lib.mec_encode_batch_dev_pipe.argtypes = [vp, i32, vp, i64, vp, i32, vp]
    lib.mec_pipe_sync.argtypes = [vp]
    i64p = c.POINTER(i64)
    lib.mec_var_row_offsets.argtypes = [i32, i64, i32, i64p, i64p]
    lib.mec_encode_batch_var.argtypes = [vp, i32, u8p, i64p, u8p, i32, u8p]
    lib.mec_encode_batch_var_dev.argtypes = [vp, i32, vp, i64p, vp, i32, vp]
    lib.mec_encode_batch_var_dev_async.argtypes = [vp, i32, vp, i64p, vp, i32, vp]
    lib.mec_frame_offsets.argtypes = [i32, i64, i32, i64p, i64p]
    lib.mec_encode_frames_batch_var.argtypes = [vp, i32, u8p, i64p, u8p, i32]
    lib.mec_encode_frames_batch_var_dev.argtypes = [vp, i32, vp, i64p, vp, i32]
    lib.mec_encode_frames_batch_var_dev_async.argtypes = [
        vp, i32, vp, i64p, vp, i32]
    lib.mec_reconstruct_batch.argtypes = [vp, i32, u8p, u8p, i64, i32]
    lib.mec_reconstruct_batch_dev.argtypes = [vp, i32, vp, u8p, i64, i32]
    lib.mec_reconstruct_batch_dev_async.argtypes = [vp, i32, vp, u8p, i64, i32]
    lib.mec_reconstruct_batch_mixed.argtypes = [vp, i32, u8p, u8p, i64, i32, u8p]
    lib.mec_reconstruct_batch_mixed_dev.argtypes = [vp, i32, vp, u8p, i64, i32, u8p]
    lib.mec_reconstruct_batch_mixed_dev_async.argtypes = [vp, i32, vp, u8p, i64, i32, u8p]
    lib.mec_verify_reconstruct_batch_dev.argtypes = [
        vp, i32, vp, vp, u8p, i64, i32, i32, i32, u8p, u8p]
    lib.mec_verify_reconstruct_batch.argtypes = [
        vp, i32, u8p, u8p, u8p, i64, i32, i32, i32, u8p, u8p]
    lib.mec_verify_reconstruct_batch_var_dev.argtypes = [
        vp, i32, vp, vp, i64p, u8p, i32, i32, i32, u8p, u8p]
    lib.mec_verify_reconstruct_batch_var.argtypes = [
        vp, i32, u8p, u8p, i64p, u8p, i32, i32, i32, u8p, u8p]
    lib.mec_bitrot_sum_batch.argtypes =[vp, i32, i32, u8p, i64, i64, u8p]
    lib.mec_bitrot_sum_batch_dev.argtypes = [vp, i32, i32, vp, i64, i64, vp]
    lib.mec_bitrot_verify_batch.argtypes = [vp, i32, i32, u8p, i64, i64, u8p, u8p]
    lib.mec_bitrot_verify_stream.argtypes = [vp, u8p, i64, i64, i32, u8p, i64]
    lib.mec_scrub_file_offsets.argtypes = [i32, i64p, i64p]
    lib.mec_bitrot_verify_files_dev.argtypes = [
        vp, i32, vp, i64, i64p, i64p, i64p, i64p, i32, u8p, i64p]
    lib.mec_bitrot_verify_files.argtypes = [
        vp, i32, c.POINTER(u8p), i64p, i64p, i64p, i32, u8p, i64p]
    lib.mec_encode_stream.argtypes = [vp, u8p, i64, i32, c.POINTER(u8p), u8p]
    lib.mec_decode_stream.argtypes = [vp, c.POINTER(u8p), u8p, i32, i64, i64, i64, u8p]
    lib.mec_heal_stream.argtypes = [vp, c.POINTER(u8p), i32, i64, c.POINTER(u8p)]
    lib.mec_dev_alloc.argtypes = [vp, sz, c.POINTER(vp)]
    lib.mec_dev_free.argtypes = [vp, vp]
    lib.mec_memcpy_h2d.argtypes = [vp, vp, u8p, sz]
    lib.mec_memcpy_d2h.argtypes = [vp, u8p, vp, sz]
    lib.mec_memset_dev.argtypes = [vp, vp, i32, sz]
    lib.mec_stream_sync.argtypes = [vp]
    lib.mec_timer_start.argtypes = [vp]
    lib.mec_timer_stop.argtypes = [vp, c.POINTER(c.c_float)]
    return lib


_lib = _load()


def _check(status):
    if status == MEC_OK:
        return
    detail = (_lib.mec_last_error() or b"").decode()
    if status == 5:
        raise FileCorruptError(status, detail)
    if status == 8:
        raise NoGPUError(status, detail)
    raise MecError(status, detail)


def device_count() -> int:
    return _lib.mec_device_count()


def hash_size(algo: int) -> int:
    return _HASH_SIZE[algo]


# ---- host-side shard-size math (pure, no GPU) -----------------------------

def shard_size(block_size: int, d: int) -> int:
    return _lib.mec_shard_size(block_size, d)


def shard_file_size(block_size: int, d: int, total_length: int) -> int:
    return _lib.mec_shard_file_size(block_size, d, total_length)


def shard_file_offset(block_size: int, d: int, start: int, length: int,
                      total: int) -> int:
    return _lib.mec_shard_file_offset(block_size, d, start, length, total)


def bitrot_shard_file_size(size: int, shard_size_: int, algo: int) -> int:
    return _lib.mec_bitrot_shard_file_size(size, shard_size_, algo)


def var_row_offsets(d: int, block_size: int, lens) -> list:
    """Row offsets R_0..R_n of the packed per-item-length encode layout
    (mec_var_row_offsets): R_{i+1} = R_i + align64(ceil(lens[i]/d)).  Item
    i's data rows start at d*R_i, its parity rows at p*R_i.  Raises
    MecError(6) for an empty list or a length outside [1, block_size]."""
    n = len(lens)
    arr = (ctypes.c_int64 * max(n, 1))(*lens)
    out = (ctypes.c_int64 * (n + 1))()
    _check(_lib.mec_var_row_offsets(d, block_size, n, arr, out))
    return list(out)


def frame_offsets(d: int, block_size: int, lens) -> list:
    """Frame offsets F_0..F_n of the batch encode into on-disk frames
    (mec_frame_offsets): F_{i+1} = F_i + 32 + ceil(lens[i]/d).  Item i's
    [hash||shard] frame starts at F_i of every row stream, and a row stream
    is F_n bytes.  Raises MecError(6) for an empty list or a length outside
    [1, block_size]."""
    n = len(lens)
    arr = (ctypes.c_int64 * max(n, 1))(*lens)
    out = (ctypes.c_int64 * (n + 1))()
    _check(_lib.mec_frame_offsets(d, block_size, n, arr, out))
    return list(out)


def scrub_file_offsets(sizes) -> list:
    """Offsets F_0..F_n of the batch scrub's convenience layout
    (mec_scrub_file_offsets): F_{f+1} = F_f + align64(sizes[f]).  Raises
    MecError(6) for an empty list or a negative size."""
    n = len(sizes)
    arr = (ctypes.c_int64 * max(n, 1))(*sizes)
    out = (ctypes.c_int64 * (n + 1))()
    _check(_lib.mec_scrub_file_offsets(n, arr, out))
    return list(out)


class Erasure:
    """Mirror of the reference Erasure type (cmd/erasure-coding.go:35).

    Requires a visible GPU (raises NoGPUError otherwise)."""

    def __init__(self, data_blocks: int, parity_blocks: int,
                 block_size: int = 1 << 20, device: int = 0):
        self.d = data_blocks
        self.p = parity_blocks
        self.block_size = block_size
        self._ctx = ctypes.c_void_p()
        _check(_lib.mec_ctx_create(data_blocks, parity_blocks, block_size,
                                   device, ctypes.byref(self._ctx)))

    def close(self):
        if self._ctx:
            _lib.mec_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self):
        if not self._ctx:
            raise MecError(6, "context is closed")
        return self._ctx

    # -- size math (instance mirrors) --
    def shard_size(self) -> int:
        return shard_size(self.block_size, self.d)

    def shard_file_size(self, total_length: int) -> int:
        return shard_file_size(self.block_size, self.d, total_length)

    def shard_file_offset(self, start: int, length: int, total: int) -> int:
        return shard_file_offset(self.block_size, self.d, start, length, total)

    # -- EncodeData (cmd/erasure-coding.go:77-89) --
    def encode_data(self, data: bytes, algo: int = None):
        """Split + Encode one block.  Returns (shards, sums):
        shards = d+p bytes objects of ceil(len/d) (data shards zero-padded),
        sums = per-shard bitrot digests when algo given, else None."""
        if len(data) == 0:
            return [b""] * (self.d + self.p), None
        shards, sums = self.encode_batch(data, len(data), 1, algo)
        return ([sh for sh in shards[0]],
                sums[0] if sums is not None else None)

    def encode_batch(self, blocks: bytes, block_len: int, n: int,
                     algo: int = None):
        """n independent blocks packed at block_len stride.  Returns
        (shards, sums): shards[b][s] bytes, sums[b][s] digests or None."""
        S = shard_size(block_len, self.d)
        parity = ctypes.create_string_buffer(n * self.p * S)
        sums_buf = None
        if algo is not None:
            sums_buf = ctypes.create_string_buffer(
                n * (self.d + self.p) * _HASH_SIZE[algo])
        _check(_lib.mec_encode_batch(self._ck(), n, blocks, block_len, parity,
                                     algo or 0, sums_buf))
        out = []
        hs = _HASH_SIZE[algo] if algo is not None else 0
        sums = [] if algo is not None else None
        for b in range(n):
            blk = blocks[b * block_len:(b + 1) * block_len]
            shards = []
            for k in range(self.d):
                sh = blk[k * S:(k + 1) * S]
                shards.append(sh + b"\0" * (S - len(sh)))
            for i in range(self.p):
                off = (b * self.p + i) * S
                shards.append(parity.raw[off:off + S])
            out.append(shards)
            if algo is not None:
                t = self.d + self.p
                sums.append([
                    sums_buf.raw[(b * t + s) * hs:(b * t + s + 1) * hs]
                    for s in range(t)
                ])
        return out, sums

    def encode_batch_var(self, blocks, algo: int = None):
        """Encode many blocks in one call, each with its OWN length in
        [1, block_size] — what a PUT batch across objects produces, since
        Erasure.Encode hands EncodeData whatever io.ReadFull returned
        (cmd/erasure-encode.go:76-108; mec_encode_batch_var).

        blocks: list of bytes.  Returns (shards, sums) in the shape of
        encode_batch: shards[b][s] is ceil(len(blocks[b])/d) bytes (data
        shards zero-padded), sums[b][s] the 32-byte digests or None.  algo
        must be HIGHWAYHASH256S or HIGHWAYHASH256 when given."""
        n = len(blocks)
        if n == 0:
            return [], ([] if algo is not None else None)
        d, p, t = self.d, self.p, self.d + self.p
        lens = (ctypes.c_int64 * n)(*[len(b) for b in blocks])
        sizes = [shard_size(len(b), d) for b in blocks]
        parity = ctypes.create_string_buffer(max(p * sum(sizes), 1))
        sums_buf = None
        if algo is not None:
            sums_buf = ctypes.create_string_buffer(n * t * 32)
        _check(_lib.mec_encode_batch_var(self._ck(), n, b"".join(blocks),
                                         lens, parity, algo or 0, sums_buf))
        praw = parity.raw
        sraw = sums_buf.raw if sums_buf is not None else None
        out, sums, off = [], ([] if algo is not None else None), 0
        for b, (blk, S) in enumerate(zip(blocks, sizes)):
            shards = []
            for k in range(d):
                sh = blk[k * S:(k + 1) * S]
                shards.append(sh + b"\0" * (S - len(sh)))
            for i in range(p):
                shards.append(praw[off:off + S])
                off += S
            out.append(shards)
            if sraw is not None:
                sums.append([sraw[(b * t + s) * 32:(b * t + s + 1) * 32]
                             for s in range(t)])
        return out, sums

    def encode_frames_batch_var(self, blocks, algo: int = None):
        """encode_batch_var straight into the on-disk format
        (mec_encode_frames_batch_var): every block becomes one
        [hash||shard] frame of streamingBitrotWriter
        (cmd/bitrot-streaming.go:44-75) in each of the d+p row streams.

        blocks: list of bytes, each of its own length in [1, block_size].
        Returns (streams, offsets): streams[s] is row s's byte stream, in
        which block i's frame is [offsets[i], offsets[i+1]); consecutive
        blocks of one object make that object's shard file.  algo defaults
        to HIGHWAYHASH256S and must be it or HIGHWAYHASH256."""
        n = len(blocks)
        t = self.d + self.p
        if n == 0:
            return [b""] * t, [0]
        if algo is None:
            algo = HIGHWAYHASH256S
        lens = [len(b) for b in blocks]
        # the library refuses the lengths itself; without offsets there is
        # no buffer to hand it
        off = frame_offsets(self.d, self.block_size, lens)
        buf = ctypes.create_string_buffer(t * off[-1])
        _check(_lib.mec_encode_frames_batch_var(
            self._ck(), n, b"".join(blocks), (ctypes.c_int64 * n)(*lens),
            buf, algo))
        raw = buf.raw
        return [raw[s * off[-1]:(s + 1) * off[-1]] for s in range(t)], off

    # -- DecodeDataBlocks / DecodeDataAndParityBlocks --
    def decode_data_blocks(self, shards):
        """cmd/erasure-coding.go:94-107: None entries = missing; returns the
        list with data shards filled.  No-op when nothing is missing."""
        return self._reconstruct(shards, data_only=True)

    def decode_data_and_parity_blocks(self, shards):
        """cmd/erasure-coding.go:111-113."""
        return self._reconstruct(shards, data_only=False)

    def _reconstruct(self, shards, data_only):
        total = self.d + self.p
        assert len(shards) == total
        missing = [i for i, s in enumerate(shards) if s is None or len(s) == 0]
        if not missing or len(missing) == total:
            return list(shards)
        per = next(len(s) for s in shards if s)
        buf = ctypes.create_string_buffer(total * per)
        present = bytes(0 if (s is None or len(s) == 0) else 1 for s in shards)
        for i, s in enumerate(shards):
            if s:
                buf[i * per:(i + 1) * per] = s
        _check(_lib.mec_reconstruct_batch(self._ck(), 1, buf, present, per,
                                          1 if data_only else 0))
        out = []
        for i in range(total):
            if present[i] or not data_only or i < self.d:
                out.append(buf.raw[i * per:(i + 1) * per])
            else:
                out.append(shards[i])
        return out

    def reconstruct_batch(self, items, data_only=False):
        """Reconstruct many blocks in one call, each with its OWN erasure
        pattern — what a degraded read or heal batched across objects
        produces, since every object rotates its shards by hashOrder
        (cmd/erasure-metadata-utils.go:178).

        items: list of d+p-long lists of equal-length shards, None marking
        a missing shard.  Returns (items_out, statuses): missing shards
        filled in (data shards only when data_only; missing parity then
        stays None), statuses[i] 0 or 3 (ErrTooFewShards).  An
        unrecoverable item comes back unchanged with its status set; it
        does not fail the rest of the batch."""
        total = self.d + self.p
        n = len(items)
        if n == 0:
            return [], []
        for it in items:
            assert len(it) == total
        lens = {len(s) for it in items for s in it if s is not None}
        if not lens:
            return [list(it) for it in items], [3] * n
        assert len(lens) == 1, "all shards of a batch share one length"
        per = lens.pop()
        present = bytes(0 if s is None else 1 for it in items for s in it)
        hole = b"\0" * per
        buf = ctypes.create_string_buffer(
            b"".join(hole if s is None else s for it in items for s in it),
            n * total * per)
        status = ctypes.create_string_buffer(n)
        _check(_lib.mec_reconstruct_batch_mixed(
            self._ck(), n, buf, present, per, 1 if data_only else 0, status))
        statuses = list(status.raw)
        raw = buf.raw
        out = []
        for i, it in enumerate(items):
            if statuses[i] != MEC_OK:
                out.append(list(it))
                continue
            row = []
            for s in range(total):
                if it[s] is None and (s < self.d or not data_only):
                    off = (i * total + s) * per
                    row.append(raw[off:off + per])
                else:
                    row.append(it[s])
            out.append(row)
        return out, statuses

    def verify_reconstruct_batch(self, items, sums, data_only=False,
                                 rehash=False,
                                 algo: int = HIGHWAYHASH256S):
        """Verified batch read (mec_verify_reconstruct_batch): bitrot-check
        the rows that were read, treat a mismatch as a missing row of that
        item, and reconstruct from what verified — streamingBitrotReader.
        ReadAt + parallelReader.Read + Decode/Heal for many blocks at once.

        items: as in reconstruct_batch, None marking a row that was not
        read.  sums[i][s]: the row's expected 32-byte digest, or None (rows
        that were not read need none).  Returns (items_out, sums_out,
        statuses, corrupt): items_out has the missing and the corrupt rows
        that are in scope rebuilt (data rows only when data_only) and every
        other row as given; statuses[i] is 0 or 3 (ErrTooFewShards: fewer
        than d rows verified, item returned unchanged); corrupt[i] lists
        the rows that were read and failed their check.  sums_out is None
        unless rehash: then sums with the rebuilt rows' fresh digests."""
        total = self.d + self.p
        n = len(items)
        if n == 0:
            return [], ([] if rehash else None), [], []
        assert len(sums) == n
        for it, su in zip(items, sums):
            assert len(it) == total and len(su) == total
        lens = {len(s) for it in items for s in it if s is not None}
        if not lens:
            return ([list(it) for it in items],
                    [list(su) for su in sums] if rehash else None,
                    [3] * n, [[] for _ in range(n)])
        assert len(lens) == 1, "all shards of a batch share one length"
        per = lens.pop()
        for it, su in zip(items, sums):
            for s in range(total):
                assert it[s] is None or (su[s] is not None
                                         and len(su[s]) == 32), \
                    "a row that was read needs its 32-byte digest"
        read = bytes(0 if s is None else 1 for it in items for s in it)
        hole, nosum = b"\0" * per, b"\0" * 32
        buf = ctypes.create_string_buffer(
            b"".join(hole if s is None else s for it in items for s in it),
            n * total * per)
        sbuf = ctypes.create_string_buffer(
            b"".join(nosum if h is None else h for su in sums for h in su),
            n * total * 32)
        present = ctypes.create_string_buffer(n * total)
        status = ctypes.create_string_buffer(n)
        _check(_lib.mec_verify_reconstruct_batch(
            self._ck(), n, buf, sbuf, read, per, algo,
            1 if data_only else 0, 1 if rehash else 0, present, status))
        statuses = list(status.raw)
        pres, raw, sraw = present.raw, buf.raw, sbuf.raw
        scope = self.d if data_only else total
        out, sums_out, corrupt = [], ([] if rehash else None), []
        for i, it in enumerate(items):
            corrupt.append([s for s in range(total)
                            if read[i * total + s] and not pres[i * total + s]])
            row, srow = list(it), list(sums[i])
            if statuses[i] == MEC_OK:
                for s in range(scope):
                    c = i * total + s
                    if not pres[c]:
                        row[s] = raw[c * per:(c + 1) * per]
                        srow[s] = sraw[c * 32:(c + 1) * 32]
            out.append(row)
            if rehash:
                sums_out.append(srow)
        return out, sums_out, statuses, corrupt

    def verify_reconstruct_batch_var(self, items, sums, data_only=False,
                                     rehash=False,
                                     algo: int = HIGHWAYHASH256S):
        """verify_reconstruct_batch with a shard length PER ITEM
        (mec_verify_reconstruct_batch_var): what a GET or heal batch across
        objects holds, since parallelReader.Read shortens shardSize for the
        last block of every object (cmd/erasure-decode.go:138-139).

        Arguments and the return shape are verify_reconstruct_batch's; the
        shards of one item share a length S_i, items may differ.  An item's
        block length cannot be recovered from S_i alone and does not need
        to be: the call is given len_i = S_i*d (capped at block_size), which
        yields the same S_i = ceil(len_i/d) and so the same rows and
        digests.  An item with
        every row None comes back unchanged with status 3; it is passed to
        the library with S_i = 1 and an all-zero mask."""
        d, total = self.d, self.d + self.p
        n = len(items)
        if n == 0:
            return [], ([] if rehash else None), [], []
        assert len(sums) == n
        sizes = []
        for it, su in zip(items, sums):
            assert len(it) == total and len(su) == total
            lens = {len(s) for s in it if s is not None}
            assert len(lens) <= 1, "the shards of an item share one length"
            sizes.append(lens.pop() if lens else 1)
            for s in range(total):
                assert it[s] is None or (su[s] is not None
                                         and len(su[s]) == 32), \
                    "a row that was read needs its 32-byte digest"
        read = bytes(0 if s is None else 1 for it in items for s in it)
        nosum = b"\0" * 32
        buf = ctypes.create_string_buffer(
            b"".join(b"\0" * S if s is None else s
                     for it, S in zip(items, sizes) for s in it),
            total * sum(sizes))
        sbuf = ctypes.create_string_buffer(
            b"".join(nosum if h is None else h for su in sums for h in su),
            n * total * 32)
        if max(sizes) > self.shard_size():
            raise MecError(6, "a shard is longer than ceil(block_size/d)")
        # S*d may pass block_size by up to d-1 when d does not divide it
        lens = (ctypes.c_int64 * n)(*[min(S * d, self.block_size)
                                      for S in sizes])
        present = ctypes.create_string_buffer(n * total)
        status = ctypes.create_string_buffer(n)
        _check(_lib.mec_verify_reconstruct_batch_var(
            self._ck(), n, buf, sbuf, lens, read, algo,
            1 if data_only else 0, 1 if rehash else 0, present, status))
        statuses = list(status.raw)
        pres, raw, sraw = present.raw, buf.raw, sbuf.raw
        scope = d if data_only else total
        out, sums_out, corrupt, off = [], ([] if rehash else None), [], 0
        for i, (it, S) in enumerate(zip(items, sizes)):
            corrupt.append([s for s in range(total)
                            if read[i * total + s] and not pres[i * total + s]])
            row, srow = list(it), list(sums[i])
            if statuses[i] == MEC_OK:
                for s in range(scope):
                    c = i * total + s
                    if not pres[c]:
                        row[s] = raw[off + s * S:off + (s + 1) * S]
                        srow[s] = sraw[c * 32:(c + 1) * 32]
            off += total * S
            out.append(row)
            if rehash:
                sums_out.append(srow)
        return out, sums_out, statuses, corrupt

    # -- streaming-format drivers (Erasure.Encode / Decode / Heal) --
    def encode_stream(self, src: bytes, algo: int = HIGHWAYHASH256S):
        """Returns (drive_streams, whole_sums): d+p per-drive on-disk streams
        ([hash||shard]* for HighwayHash256S), whole-file digests for the
        legacy algorithms."""
        total = self.d + self.p
        fsz = bitrot_shard_file_size(
            self.shard_file_size(len(src)), self.shard_size(), algo)
        bufs = [ctypes.create_string_buffer(max(fsz, 1)) for _ in range(total)]
        arr = (ctypes.c_char_p * total)(*[
            ctypes.cast(b, ctypes.c_char_p) for b in bufs])
        ws = None
        if algo != HIGHWAYHASH256S:
            ws = ctypes.create_string_buffer(total * _HASH_SIZE[algo])
        _check(_lib.mec_encode_stream(self._ck(), src, len(src), algo, arr, ws))
        streams = [b.raw[:fsz] for b in bufs]
        sums = None
        if ws is not None:
            hs = _HASH_SIZE[algo]
            sums = [ws.raw[i * hs:(i + 1) * hs] for i in range(total)]
        return streams, sums

    def decode_stream(self, drive_streams, total_length: int, offset: int,
                      length: int, algo: int = HIGHWAYHASH256S,
                      whole_sums=None):
        """drive_streams: list of d+p streams (None = missing drive)."""
        total = self.d + self.p
        arr = (ctypes.c_char_p * total)(*[
            s if s is not None else None for s in drive_streams])
        ws = None
        if whole_sums is not None:
            ws = b"".join(s if s else b"\0" * _HASH_SIZE[algo]
                          for s in whole_sums)
        dst = ctypes.create_string_buffer(max(length, 1))
        _check(_lib.mec_decode_stream(self._ck(), arr, ws, algo, total_length,
                                      offset, length, dst))
        return dst.raw[:length]

    def heal_stream(self, drive_streams, total_length: int,
                    algo: int = HIGHWAYHASH256S):
        """Regenerate missing drives' streams (Erasure.Heal).  Returns the
        full list with reconstructed entries for drives that were None."""
        total = self.d + self.p
        fsz = bitrot_shard_file_size(
            self.shard_file_size(total_length), self.shard_size(), algo)
        arr = (ctypes.c_char_p * total)(*[
            s if s is not None else None for s in drive_streams])
        outs = []
        outp = (ctypes.c_char_p * total)()
        for i, s in enumerate(drive_streams):
            if s is None:
                b = ctypes.create_string_buffer(max(fsz, 1))
                outs.append(b)
                outp[i] = ctypes.cast(b, ctypes.c_char_p)
            else:
                outs.append(None)
                outp[i] = None
        _check(_lib.mec_heal_stream(self._ck(), arr, algo, total_length, outp))
        return [
            drive_streams[i] if drive_streams[i] is not None
            else outs[i].raw[:fsz]
            for i in range(total)
        ]

    # -- batch hashing --
    def bitrot_sum_batch(self, algo: int, msgs: bytes, msg_len: int,
                         msg_stride: int, n: int):
        hs = _HASH_SIZE[algo]
        out = ctypes.create_string_buffer(max(n * hs, 1))
        _check(_lib.mec_bitrot_sum_batch(self._ck(), algo, n, msgs, msg_len,
                                         msg_stride, out))
        return [out.raw[i * hs:(i + 1) * hs] for i in range(n)]

    def bitrot_verify_stream(self, stream: bytes, part_size: int, algo: int,
                             want_sum: bytes = None,
                             shard_size_: int = None) -> bool:
        """bitrotVerify (cmd/bitrot.go:164-216).  True = intact."""
        ss = shard_size_ if shard_size_ is not None else self.shard_size()
        try:
            _check(_lib.mec_bitrot_verify_stream(
                self._ck(), stream, len(stream), part_size, algo, want_sum, ss))
            return True
        except FileCorruptError:
            return False

    def bitrot_verify_files(self, files, part_sizes, shard_sizes):
        """Batch scrub (mec_bitrot_verify_files): bitrotVerify for
        HighwayHash256S over many on-disk [hash||shard]* shard files in one
        call.  files[f] is the file's bytes as present on the drive,
        part_sizes[f] its erasure.ShardFileSize(part.Size), shard_sizes[f]
        its erasure.ShardSize().  Returns (status, first_bad): status[f] is
        0 or 5 (file corrupt), first_bad[f] the lowest failing frame, -1
        for an intact file and for a file of the wrong size."""
        n = len(files)
        i64n = ctypes.c_int64 * max(n, 1)
        ptrs = (ctypes.c_char_p * max(n, 1))(*files)
        sizes = i64n(*[len(f) for f in files])
        status = ctypes.create_string_buffer(max(n, 1))
        first_bad = i64n()
        _check(_lib.mec_bitrot_verify_files(
            self._ck(), n, ptrs, sizes, i64n(*part_sizes),
            i64n(*shard_sizes), HIGHWAYHASH256S, status, first_bad))
        return list(status.raw[:n]), list(first_bad)[:n]
