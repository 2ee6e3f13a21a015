"""GPU kernels against shard files that a reference server wrote to disk.

tests/golden/reference_shards/ (see tools/extract_reference_shards.py and
tests/reference_shards.py) holds whole objects as they lay on the drives:
per row the 32-byte HighwayHash256S digest followed by the shard, plus the
erasure geometry and the object's MD5 etag.  Every expected value in this
file is a fixture byte or an etag; no oracle call sits in one.  Each object
is a single short block of a 1 MiB-block Erasure(d, p), which is what a
small-object PUT or GET is.

  object                    geometry  size    shard S  S % 32  rows stored
  merge-hosts-228-* (two)   EC2+2     228     114      18      all 4
  merge-hosts-19113-null    EC2+2     19113   9557     21      all 4
  inline-notinline-file-*   EC2+2     132096  66048    0       1 and 2
  cicd-testobj-644520       EC3+2     644520  214840   24      all 5

What runs here, by kernel:
  hh256_batch4_kernel<true>/<false>    test_plain_hash*  (S % 32 != 0 / == 0)
  specialised encode + its hash        test_encode_batch, test_encode_stream
  gf_encode_bs_var_kernel,
  hh256_var_kernel                     test_encode_var_*
  hh256_frames_verify, _sheared        test_scrub_*
  hh256_list_verify/_sum,
  gf_matmul_bs_mixed_kernel            test_verified_read*
  hh256_list_var_*,
  gf_matmul_bs_mixed_var_kernel        test_verified_read_var
  gf_matmul_bs_kernel                  test_uniform_reconstruct, test_streams*

The one-pass kernel (fused4.hip) takes only EC8+4 shapes whose shard length
is a multiple of its 512-byte step, which none of these objects has.  It
stays pinned through test_gpu_fused4.py against the kernel pair, and the
pair is pinned here.

The partial object has only one data row and one parity row on disk, so its
bytes exist only after a decode: it is decoded on the GPU, the MD5 is
compared with the etag, and from then on those bytes stand for the object.
"""
import ctypes
import itertools

import pytest

import minio_amd
import reference_shards as refs

pytestmark = pytest.mark.gpu

lib = minio_amd._lib
HHS = minio_amd.HIGHWAYHASH256S
HH = minio_amd.HIGHWAYHASH256
CORRUPT = 5
MARK = 0xA5

EC22 = [o for o in refs.OBJECTS if (o.d, o.p) == (2, 2)]
OTHER = [o for o in refs.OBJECTS if (o.d, o.p) != (2, 2)]


def check(st):
    assert st == 0, (st, lib.mec_last_error())


def align64(x):
    return (x + 63) & ~63


def i64arr(v):
    return (ctypes.c_int64 * max(len(v), 1))(*v)


def flip(b, at, bit=0):
    return b[:at] + bytes([b[at] ^ (1 << bit)]) + b[at + 1:]


@pytest.fixture(scope="module")
def ctxs():
    """One Erasure per geometry of the manifest, 1 MiB blocks."""
    made = {}
    for o in refs.OBJECTS:
        key = (o.d, o.p, o.block_size)
        if key not in made:
            made[key] = minio_amd.Erasure(*key, device=0)
    yield lambda o: made[(o.d, o.p, o.block_size)]
    for e in made.values():
        e.close()


_bytes = {}


def object_bytes(ctxs, obj):
    """The object's bytes, MD5-checked against its etag: joined data rows
    for a complete object, a GPU decode of the stored rows otherwise."""
    if obj.name not in _bytes:
        if obj.complete:
            data = obj.data()
        else:
            data = ctxs(obj).decode_stream(obj.bins, obj.size, 0, obj.size)
        assert refs.md5hex(data) == obj.etag, obj
        _bytes[obj.name] = data
    return _bytes[obj.name]


def assert_stored(obj, shards, sums, what):
    """Every row that the reference stored equals what was computed."""
    for i in obj.stored:
        assert shards[i] == obj.shards[i], (what, obj, "row", i)
        assert sums[i] == obj.digests[i], (what, obj, "digest", i)


# ---- plain hash kernel ------------------------------------------------------

@pytest.mark.parametrize("algo", [HHS, HH])
@pytest.mark.parametrize("obj", refs.OBJECTS, ids=repr)
def test_plain_hash(ctxs, obj, algo):
    """bitrot_sum_batch over the stored shards: once as they are (a partial
    wave), once repeated past 64 chains so that a second workgroup hashes
    them too."""
    e = ctxs(obj)
    rows = [obj.shards[i] for i in obj.stored]
    want = [obj.digests[i] for i in obj.stored]
    got = e.bitrot_sum_batch(algo, b"".join(rows), obj.S, obj.S, len(rows))
    assert got == want
    reps = 64 // len(rows) + 1
    got = e.bitrot_sum_batch(algo, b"".join(rows) * reps, obj.S, obj.S,
                             reps * len(rows))
    assert len(got) > 64 and got == want * reps


@pytest.mark.parametrize("obj", refs.OBJECTS, ids=repr)
def test_plain_hash_dev_stride(ctxs, obj):
    """mec_bitrot_sum_batch_dev at the device row stride align64(S); the
    bytes between a row's end and the next row hold a marker."""
    e = ctxs(obj)
    rows = [obj.shards[i] for i in obj.stored]
    n, stride = len(rows), align64(obj.S)
    img = b"".join(r + bytes([MARK]) * (stride - obj.S) for r in rows)
    msgs, sums = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.mec_dev_alloc(e._ctx, n * stride, ctypes.byref(msgs)))
    check(lib.mec_dev_alloc(e._ctx, n * 32, ctypes.byref(sums)))
    try:
        check(lib.mec_memcpy_h2d(e._ctx, msgs, img, len(img)))
        check(lib.mec_bitrot_sum_batch_dev(e._ctx, HHS, n, msgs, obj.S,
                                           stride, sums))
        out = ctypes.create_string_buffer(n * 32)
        check(lib.mec_memcpy_d2h(e._ctx, out, sums, n * 32))
    finally:
        lib.mec_dev_free(e._ctx, msgs)
        lib.mec_dev_free(e._ctx, sums)
    assert [out.raw[i * 32:(i + 1) * 32] for i in range(n)] == \
        [obj.digests[i] for i in obj.stored]


# ---- encode, kernel pair ----------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("obj", refs.OBJECTS, ids=repr)
def test_encode_batch(ctxs, obj, n):
    """Parity rows and all d+p digests of one block, and of the same block
    three times in one call (blockIdx.y > 0)."""
    data = object_bytes(ctxs, obj)
    shards, sums = ctxs(obj).encode_batch(data * n, obj.size, n, HHS)
    assert len(shards) == n
    for b in range(n):
        assert_stored(obj, shards[b], sums[b], f"block {b} of {n}")


@pytest.mark.parametrize("obj", refs.OBJECTS, ids=repr)
def test_encode_stream(ctxs, obj):
    """Every drive's stream equals the stored file, byte for byte."""
    streams, _ = ctxs(obj).encode_stream(object_bytes(ctxs, obj), HHS)
    assert len(streams) == obj.total
    for i in obj.stored:
        assert streams[i] == obj.bins[i], (obj, i)


# ---- encode with a length per item -----------------------------------------

def test_encode_var_ec22(ctxs):
    """Every EC2+2 object as one batch: lengths 19113, 228, 228 and 132096
    side by side."""
    assert len({o.size for o in EC22}) >= 2
    blocks = [object_bytes(ctxs, o) for o in EC22]
    shards, sums = ctxs(EC22[0]).encode_batch_var(blocks, HHS)
    for o, sh, su in zip(EC22, shards, sums):
        assert_stored(o, sh, su, "var")


@pytest.mark.parametrize("obj", OTHER, ids=repr)
def test_encode_var_with_copy(ctxs, obj):
    """An object of another geometry in a call of its own, with a copy."""
    data = object_bytes(ctxs, obj)
    shards, sums = ctxs(obj).encode_batch_var([data, data], HH)
    for sh, su in zip(shards, sums):
        assert_stored(obj, sh, su, "var")


# ---- scrub ------------------------------------------------------------------

class ScrubImage:
    """Every stored .bin eight times, copy c at file_off = c (mod 8), so
    that the aligned and the sheared kernel both hash reference-written
    frames where they lie.  A marker fills the gaps."""

    def __init__(self, objs):
        self.files, self.offs, self.parts, self.shards = [], [], [], []
        cur = 0
        for o in objs:
            for i in o.stored:
                for phase in range(8):
                    cur += (phase - cur) % 8
                    self.offs.append(cur)
                    self.files.append(o.bins[i])
                    self.parts.append(o.S)
                    self.shards.append(-(-o.block_size // o.d))
                    cur += len(o.bins[i])
        self.n = len(self.files)

    def run_dev(self, e):
        sizes = [len(f) for f in self.files]
        nbytes = self.offs[-1] + sizes[-1]
        img = bytearray([MARK]) * (nbytes + 256)
        for off, f in zip(self.offs, self.files):
            img[off:off + len(f)] = f
        img = bytes(img)
        dev = ctypes.c_void_p()
        check(lib.mec_dev_alloc(e._ctx, len(img), ctypes.byref(dev)))
        try:
            check(lib.mec_memcpy_h2d(e._ctx, dev, img, len(img)))
            status = ctypes.create_string_buffer(b"\x77" * self.n, self.n)
            fb = i64arr([-9] * self.n)
            check(lib.mec_bitrot_verify_files_dev(
                e._ctx, self.n, dev, nbytes, i64arr(self.offs),
                i64arr(sizes), i64arr(self.parts), i64arr(self.shards), HHS,
                status, fb))
        finally:
            lib.mec_dev_free(e._ctx, dev)
        return list(status.raw), list(fb)[:self.n]


def test_scrub_every_phase(ctxs):
    im = ScrubImage(refs.OBJECTS)
    assert {o % 8 for o in im.offs} == set(range(8))
    status, fb = im.run_dev(ctxs(refs.OBJECTS[0]))
    bad = [(f, im.offs[f] % 8, im.parts[f]) for f in range(im.n)
           if status[f] != 0 or fb[f] != -1]
    assert not bad, bad[:10]


def test_scrub_two_flips(ctxs):
    """One bit flipped in one copy's message and one in another copy's
    digest: exactly those two files are corrupt, at frame 0.  The two
    copies lie at an odd and at an aligned offset."""
    im = ScrubImage(refs.OBJECTS)
    a, b = 3, im.n - 8
    assert im.offs[a] % 8 == 3 and im.offs[b] % 8 == 0
    im.files[a] = flip(im.files[a], 32 + im.parts[a] - 1, bit=6)
    im.files[b] = flip(im.files[b], 17, bit=2)
    status, fb = im.run_dev(ctxs(refs.OBJECTS[0]))
    assert [f for f in range(im.n) if status[f] != 0] == [a, b]
    assert status[a] == CORRUPT and status[b] == CORRUPT
    assert [fb[f] for f in range(im.n)] == \
        [0 if f in (a, b) else -1 for f in range(im.n)]


@pytest.mark.parametrize("obj", refs.OBJECTS, ids=repr)
def test_scrub_host_and_stream(ctxs, obj):
    """bitrot_verify_files (host pointers) and bitrot_verify_stream on each
    stored file, then with the last file's last message byte flipped."""
    e = ctxs(obj)
    files = [obj.bins[i] for i in obj.stored]
    n = len(files)
    ss = e.shard_size()
    status, fb = e.bitrot_verify_files(files, [obj.S] * n, [ss] * n)
    assert status == [0] * n and fb == [-1] * n
    for f in files:
        assert e.bitrot_verify_stream(f, obj.S, HHS)
    files[-1] = flip(files[-1], len(files[-1]) - 1)
    status, fb = e.bitrot_verify_files(files, [obj.S] * n, [ss] * n)
    assert status == [0] * (n - 1) + [CORRUPT]
    assert fb == [-1] * (n - 1) + [0]
    assert not e.bitrot_verify_stream(files[-1], obj.S, HHS)


# ---- verified read ----------------------------------------------------------

def read_items(obj):
    """One item per erasure pattern of 1..p rows, then one with every row
    read and a byte flipped in data row d-1.  Returns (items, sums,
    want_corrupt, lost)."""
    items, sums, want_corrupt, lost_of = [], [], [], []
    for lost in obj.patterns():
        items.append(obj.without(lost))
        sums.append(obj.without(lost, obj.digests))
        want_corrupt.append([])
        lost_of.append(set(lost))
    hit = obj.d - 1
    rows = list(obj.shards)
    rows[hit] = flip(rows[hit], obj.S // 2, bit=5)
    items.append(rows)
    sums.append(list(obj.digests))
    want_corrupt.append([hit])
    lost_of.append({hit})
    return items, sums, want_corrupt, lost_of


def assert_read(obj, lost, data_only, out, sums_out, what):
    """Rows in scope equal the stored rows, rebuilt ones included, and so
    do their digests; a lost parity row stays None under data_only."""
    for s in range(obj.total):
        if data_only and s >= obj.d and s in lost:
            assert out[s] is None, (what, obj, s)
            continue
        assert out[s] == obj.shards[s], (what, obj, "row", s, lost)
        assert sums_out[s] == obj.digests[s], (what, obj, "digest", s, lost)


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("obj", refs.COMPLETE, ids=repr)
def test_verified_read(ctxs, obj, data_only):
    items, sums, want_corrupt, lost_of = read_items(obj)
    assert len(items) == {(2, 2): 10, (3, 2): 15}[(obj.d, obj.p)] + 1
    out, sums_out, statuses, corrupt = ctxs(obj).verify_reconstruct_batch(
        items, sums, data_only=data_only, rehash=True)
    assert statuses == [0] * len(items)
    assert corrupt == want_corrupt
    for i, lost in enumerate(lost_of):
        assert_read(obj, lost, data_only, out[i], sums_out[i], i)


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("obj", refs.PARTIAL, ids=repr)
def test_verified_read_partial(ctxs, obj, data_only):
    """The rows that exist, read and verified, rebuild an object whose MD5
    is the etag; the same with one of them also given a wrong digest is
    too few rows."""
    e = ctxs(obj)
    bad = list(obj.digests)
    bad[obj.stored[0]] = flip(bad[obj.stored[0]], 31)
    out, _, statuses, corrupt = e.verify_reconstruct_batch(
        [list(obj.shards), list(obj.shards)], [list(obj.digests), bad],
        data_only=data_only, rehash=True)
    assert statuses == [0, 3]
    assert corrupt == [[], [obj.stored[0]]]
    for i in obj.stored:
        assert out[0][i] == obj.shards[i]
    assert refs.md5hex(b"".join(out[0][:obj.d])[:obj.size]) == obj.etag


@pytest.mark.parametrize("data_only", [False, True])
def test_verified_read_var(ctxs, data_only):
    """Every EC2+2 object times every pattern in one call: shard lengths
    9557, 114 and 66048 side by side.  The partial object has its one
    possible pattern."""
    items, sums, want_corrupt, owner = [], [], [], []
    for o in EC22:
        if o.complete:
            it, su, wc, lost_of = read_items(o)
        else:
            it, su, wc = [list(o.shards)], [list(o.digests)], [[]]
            lost_of = [set(range(o.total)) - set(o.stored)]
        items += it
        sums += su
        want_corrupt += wc
        owner += [(o, lost) for lost in lost_of]
    assert len({o.S for o, _ in owner}) >= 2
    out, sums_out, statuses, corrupt = \
        ctxs(EC22[0]).verify_reconstruct_batch_var(
            items, sums, data_only=data_only, rehash=True)
    assert statuses == [0] * len(items)
    assert corrupt == want_corrupt
    for i, (o, lost) in enumerate(owner):
        if o.complete:
            assert_read(o, lost, data_only, out[i], sums_out[i], i)
        else:
            for s in o.stored:
                assert out[i][s] == o.shards[s]
                assert sums_out[i][s] == o.digests[s]
            assert refs.md5hex(b"".join(out[i][:o.d])[:o.size]) == o.etag


# ---- uniform reconstruct ----------------------------------------------------

@pytest.mark.parametrize("obj", refs.COMPLETE, ids=repr)
def test_uniform_reconstruct(ctxs, obj):
    e = ctxs(obj)
    for lost in obj.patterns():
        rec = e.decode_data_and_parity_blocks(obj.without(lost))
        assert rec == obj.shards, (obj, lost)
        rec = e.decode_data_blocks(obj.without(lost))
        assert rec[:obj.d] == obj.shards[:obj.d], (obj, lost)


# ---- streams ----------------------------------------------------------------

@pytest.mark.parametrize("obj", refs.OBJECTS, ids=repr)
def test_streams_decode(ctxs, obj):
    """decode_stream over the stored files placed by row returns the
    object; three ranged reads equal its slices: the first byte, a span
    across the first shard boundary, and the tail."""
    e = ctxs(obj)
    data = object_bytes(ctxs, obj)
    assert e.decode_stream(obj.bins, obj.size, 0, obj.size) == data
    if obj.complete:  # the same from the last d rows alone
        few = obj.without(set(range(obj.p)), obj.bins)
        assert refs.md5hex(e.decode_stream(few, obj.size, 0, obj.size)) \
            == obj.etag
    for off, ln in ((0, 1), (obj.S - 3, 7), (obj.size - 5, 5)):
        assert e.decode_stream(obj.bins, obj.size, off, ln) == \
            data[off:off + ln], (obj, off, ln)


@pytest.mark.parametrize("obj", refs.COMPLETE, ids=repr)
def test_streams_heal(ctxs, obj):
    """heal_stream from every d-subset of rows returns all d+p files."""
    e = ctxs(obj)
    for keep in itertools.combinations(range(obj.total), obj.d):
        lost = set(range(obj.total)) - set(keep)
        healed = e.heal_stream(obj.without(lost, obj.bins), obj.size)
        assert healed == obj.bins, (obj, keep)
