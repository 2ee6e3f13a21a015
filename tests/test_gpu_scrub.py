"""GPU tests of mec_bitrot_verify_files*: the batch scrub, bitrotVerify
(cmd/bitrot.go:164-216) over many on-disk [hash||shard]* shard files in one
call.  Files are built on the host, one oracle.bitrot_sum(HH256S, ...) per
frame, and placed at byte offsets of every alignment in a buffer prefilled
with a marker, with a guard behind it.  The marker must never influence a
verdict and the buffer must come back unchanged."""
import ctypes
import functools

import numpy as np
import pytest

import minio_amd
import oracle

pytestmark = pytest.mark.gpu

lib = minio_amd._lib
HH = minio_amd.HIGHWAYHASH256S
CORRUPT = 5
INVALID = 6
MARK = 0xA5
GUARD = 256
MiB = 1 << 20


def check(st):
    assert st == 0, (st, lib.mec_last_error())


def cptr(a):
    return a.ctypes.data_as(ctypes.c_char_p)


def i64arr(v):
    return (ctypes.c_int64 * max(len(v), 1))(*v)


@pytest.fixture(scope="module")
def ctx():
    with minio_amd.Erasure(8, 4, MiB, device=0) as e:
        yield e


def frames_of(part, S):
    return (part + S - 1) // S


@functools.lru_cache(maxsize=None)
def golden(part, S, seed):
    """One intact shard file of part bytes at shard size S, computed once
    per distinct (part, S, seed) and shared read-only."""
    data = oracle.fill_random(max(part, 1), seed)[:part]
    out = bytearray()
    for k in range(frames_of(part, S)):
        msg = data[k * S:(k + 1) * S]
        out += oracle.bitrot_sum(HH, msg) + msg
    assert len(out) == minio_amd.bitrot_shard_file_size(part, S, HH)
    a = np.frombuffer(bytes(out), dtype=np.uint8)
    a.setflags(write=False)
    return a


class Batch:
    """Files at chosen offsets.  specs: (part, S, seed, file_off % 8) per
    file; each file starts at the first address of that phase behind its
    predecessor, so neighbours are 0..7 marker bytes apart."""

    def __init__(self, specs):
        self.parts = [s[0] for s in specs]
        self.shards = [s[1] for s in specs]
        self.files = [golden(p, S, seed).copy() for p, S, seed, _ in specs]
        self.offs = []
        cur = 0
        for f, (_, _, _, phase) in zip(self.files, specs):
            cur += (phase - cur) % 8
            self.offs.append(cur)
            cur += len(f)
        self.n = len(specs)

    @property
    def sizes(self):
        return [len(f) for f in self.files]

    @property
    def nbytes(self):
        return max(o + len(f) for o, f in zip(self.offs, self.files))

    def nframes(self, f):
        return frames_of(self.parts[f], self.shards[f])

    def msg_addr(self, f, k):
        return self.offs[f] + k * (32 + self.shards[f]) + 32

    def msg_len(self, f, k):
        S = self.shards[f]
        return min(S, self.parts[f] - k * S)

    def flip_msg(self, f, k, byte, bit=0):
        assert 0 <= byte < self.msg_len(f, k)
        self.files[f][k * (32 + self.shards[f]) + 32 + byte] ^= 1 << bit

    def flip_digest(self, f, k, byte, bit=0):
        assert 0 <= byte < 32
        self.files[f][k * (32 + self.shards[f]) + byte] ^= 1 << bit

    def image(self, marker=MARK):
        buf = np.full(self.nbytes + GUARD, marker, dtype=np.uint8)
        for o, f in zip(self.offs, self.files):
            buf[o:o + len(f)] = f
        return buf

    def run_dev(self, e, marker=MARK, first_bad=True):
        """(status, first_bad) of the device call; the device buffer must
        come back as uploaded, guard included."""
        return run_dev(e, self.image(marker), self.nbytes, self.offs,
                       self.sizes, self.parts, self.shards, first_bad)

    def run_host(self, e):
        n = self.n
        ptrs = (ctypes.c_char_p * n)(*[cptr(f) for f in self.files])
        status = ctypes.create_string_buffer(b"\x77" * n, n)
        fb = i64arr([-9] * n)
        check(lib.mec_bitrot_verify_files(
            e._ctx, n, ptrs, i64arr(self.sizes), i64arr(self.parts),
            i64arr(self.shards), HH, status, fb))
        return list(status.raw), list(fb)

    def run_stream(self, e):
        """mec_bitrot_verify_stream, one call per file."""
        out = []
        for f, part, S in zip(self.files, self.parts, self.shards):
            st = lib.mec_bitrot_verify_stream(e._ctx, cptr(f), len(f), part,
                                              HH, None, S)
            assert st in (0, CORRUPT), (st, lib.mec_last_error())
            out.append(st)
        return out


def run_dev(e, buf, files_bytes, offs, sizes, parts, shards, first_bad=True):
    n = len(offs)
    dev = ctypes.c_void_p()
    check(lib.mec_dev_alloc(e._ctx, buf.nbytes, ctypes.byref(dev)))
    try:
        check(lib.mec_memcpy_h2d(e._ctx, dev, cptr(buf), buf.nbytes))
        status = ctypes.create_string_buffer(b"\x77" * n, n)
        fb = i64arr([-9] * n)
        check(lib.mec_bitrot_verify_files_dev(
            e._ctx, n, dev, files_bytes, i64arr(offs), i64arr(sizes),
            i64arr(parts), i64arr(shards), HH, status,
            fb if first_bad else None))
        back = np.empty_like(buf)
        check(lib.mec_memcpy_d2h(e._ctx, cptr(back), dev, back.nbytes))
    finally:
        lib.mec_dev_free(e._ctx, dev)
    assert np.array_equal(back, buf), "the call wrote to the files buffer"
    return list(status.raw), list(fb)[:n]


# ---- all eight address phases and all tails ------------------------------

def phase_specs():
    specs = []
    i = 0

    def add(part, S):
        nonlocal i
        specs.append((part, S, 100 + i, i % 8))
        i += 1

    # a short last frame of every residue 1..31 modulo 32 behind a full
    # frame of the two production shard sizes; the pitch of S = 87382 is
    # 6 modulo 8, so later frames change phase, that of 131072 keeps it
    for r in range(1, 32):
        S = 87382 if r % 2 else 131072
        add(S + 32 * (r % 4) + r, S)
    # one phase sweep of multi-frame files of both
    for ph in range(8):
        add(3 * 87382 + 1000 + ph, 87382)
    for ph in range(8):
        add(131072 + 5, 131072)
    # the small shard sizes: every last-frame length behind two full frames
    for S in (31, 33):
        for last in range(1, S + 1):
            add(2 * S + last, S)
    for part in (32, 64, 96, 97, 127, 320):
        add(part, 32)
    for part in (1, 2, 5, 8, 9, 40, 41):
        add(part, 1)
    # shift the phase pattern so that S = 32 and S = 1 files see others too
    for ph in range(8):
        add(70 + ph, 32)
        add(11, 1)
        add(1, 1)
    return specs


@pytest.fixture(scope="module")
def phase_batch():
    return Batch(phase_specs())


def test_phase_batch_covers_what_it_claims(phase_batch):
    b = phase_batch
    assert {o % 8 for o in b.offs} == set(range(8))
    assert set(b.shards) == {1, 31, 32, 33, 87382, 131072}
    first, later, residues = set(), set(), set()
    for f in range(b.n):
        for k in range(b.nframes(f)):
            (later if k else first).add(b.msg_addr(f, k) % 8)
        residues.add(b.msg_len(f, b.nframes(f) - 1) % 32)
    assert first == set(range(8)) and later == set(range(8))
    assert residues >= set(range(1, 32))


def test_all_phases_and_tails_intact(ctx, phase_batch):
    b = phase_batch
    status, fb = b.run_dev(ctx)
    bad = [(f, b.offs[f] % 8, b.parts[f], b.shards[f], fb[f])
           for f in range(b.n) if status[f] != 0 or fb[f] != -1]
    assert not bad, bad[:10]


@pytest.mark.parametrize("where", ["first", "last"])
def test_all_phases_and_tails_one_flip_each(ctx, where):
    """A bit flip in the first byte of every file's first message, or in
    the last byte of its last message: every file is corrupt at exactly
    that frame."""
    b = Batch(phase_specs())
    want_fb = []
    for f in range(b.n):
        k = 0 if where == "first" else b.nframes(f) - 1
        b.flip_msg(f, k, 0 if where == "first" else b.msg_len(f, k) - 1,
                   bit=f % 8)
        want_fb.append(k)
    status, fb = b.run_dev(ctx)
    assert status == [CORRUPT] * b.n
    assert fb == want_fb


# ---- prefetch thresholds --------------------------------------------------

THRESHOLD_LENS = (511, 512, 513, 1023, 1024, 1025, 1535, 1537)


def threshold_specs():
    # one frame per file, the message at the named phase; 1535 and 1537
    # also as the full frames of a three-frame file
    specs = []
    for ln in THRESHOLD_LENS:
        for ph in (0, 1, 4, 7):
            specs.append((ln, ln, 7000 + ln, ph))
    for ph in (0, 1, 4, 7):
        specs.append((2 * 1535 + 513, 1535, 7100, ph))
        specs.append((2 * 1537 + 511, 1537, 7101, ph))
    return specs


def test_prefetch_thresholds(ctx):
    b = Batch(threshold_specs())
    for ln in THRESHOLD_LENS:
        assert {b.msg_addr(f, 0) % 8 for f in range(b.n)
                if b.parts[f] == ln} == {0, 1, 4, 7}
    status, fb = b.run_dev(ctx)
    assert status == [0] * b.n and fb == [-1] * b.n
    # the last byte of the last whole 16-packet block, and the byte behind
    # it, where there is one: both edges of the ring
    want = []
    for f in range(b.n):
        ln = b.msg_len(f, 0)
        edge = ln // 512 * 512
        at = edge - 1 if f % 2 == 0 or edge == ln else edge
        b.flip_msg(f, 0, max(at, 0), bit=(f * 3) % 8)
        want.append(0)
    status, fb = b.run_dev(ctx)
    assert status == [CORRUPT] * b.n and fb == want


# ---- edge files -------------------------------------------------------------

def test_edge_files(ctx):
    specs = [
        (0, 64, 1, 3),          # 0: empty: OK, nothing hashed
        (10, 64, 2, 5),         # 1: one short frame
        (1, 131072, 3, 1),      # 2: one byte
        (4 * 100, 100, 4, 2),   # 3: exact multiple, no short frame
        (87382, 87382, 5, 7),   # 4: exactly one full frame
        (300, 100, 6, 0),       # 5: will be one byte too long
        (300, 100, 7, 6),       # 6: will be one byte short
        (0, 1, 8, 4),           # 7: empty again, between two files
        (33, 32, 9, 1),         # 8: a one-byte last frame
    ]
    b = Batch(specs)
    b.files[5] = np.concatenate([b.files[5], np.array([0x11], np.uint8)])
    b.files[6] = b.files[6][:-1].copy()
    # re-place: the sizes changed
    cur = 0
    b.offs = []
    for f, (_, _, _, phase) in zip(b.files, specs):
        cur += (phase - cur) % 8
        b.offs.append(cur)
        cur += len(f)
    assert b.sizes[0] == 0 and b.sizes[7] == 0
    want = [0, 0, 0, 0, 0, CORRUPT, CORRUPT, 0, 0]
    status, fb = b.run_dev(ctx)
    assert status == want and fb == [-1] * b.n
    assert b.run_host(ctx) == (want, [-1] * b.n)
    assert b.run_stream(ctx) == want
    # only early verdicts: nothing is launched, the verdicts still come
    only = Batch([(0, 64, 1, 3), (0, 5, 1, 0)])
    buf = np.full(GUARD, MARK, dtype=np.uint8)
    assert run_dev(ctx, buf, 16, only.offs, [0, 0], [0, 0], [64, 5]) == \
        ([0, 0], [-1, -1])
    assert only.run_host(ctx) == ([0, 0], [-1, -1])


# ---- corruption ---------------------------------------------------------------

def corruption_batch():
    specs = []
    for i in range(24):
        S = (87382, 1000, 33, 131072)[i % 4]
        specs.append((4 * S + 17 + i, S, 300 + i, (3 * i + 1) % 8))
    b = Batch(specs)
    want = {}
    b.flip_msg(1, 0, 0)                              # first message byte
    want[1] = 0
    b.flip_msg(3, 2, b.msg_len(3, 2) - 1, bit=7)     # last byte, full frame
    want[3] = 2
    b.flip_msg(5, 4, b.msg_len(5, 4) - 1, bit=3)     # last byte, short frame
    want[5] = 4
    b.flip_digest(7, 1, 0)                           # first digest byte
    want[7] = 1
    b.flip_digest(9, 4, 31, bit=7)                   # last digest byte
    want[9] = 4
    b.flip_msg(11, 2, 500, bit=4)                    # a middle frame
    want[11] = 2
    b.flip_msg(13, 3, 9)                             # two frames of one file:
    b.flip_msg(13, 1, 1)                             # the lower index
    want[13] = 1
    b.flip_digest(15, 4, 5)                          # digest and message of
    b.flip_msg(15, 2, 30)                            # different frames
    want[15] = 2
    b.flip_msg(16, 0, 0)                             # direct neighbours
    want[16] = 0
    b.flip_msg(17, 4, 0)
    want[17] = 4
    return b, want


def test_corruption(ctx):
    b, want = corruption_batch()
    want_st = [CORRUPT if f in want else 0 for f in range(b.n)]
    want_fb = [want.get(f, -1) for f in range(b.n)]
    status, fb = b.run_dev(ctx, MARK)
    assert status == want_st and fb == want_fb
    # the bytes between the files never influence a verdict
    assert b.run_dev(ctx, 0x5A) == (status, fb)
    # first_bad is optional
    assert b.run_dev(ctx, MARK, first_bad=False)[0] == want_st
    # the contender agrees file by file
    assert b.run_stream(ctx) == want_st
    assert b.run_host(ctx) == (want_st, want_fb)
    assert ctx.bitrot_verify_files(
        [bytes(f) for f in b.files], b.parts, b.shards) == (want_st, want_fb)


# ---- cross-checks ---------------------------------------------------------------

def test_verdicts_equal_verify_stream(ctx):
    """Every file's verdict equals mec_bitrot_verify_stream's on the same
    bytes, for the phase batch with a flip in every third file."""
    b = Batch(phase_specs())
    for f in range(0, b.n, 3):
        k = (f // 3) % b.nframes(f)
        b.flip_msg(f, k, (f * 7) % b.msg_len(f, k), bit=f % 8)
    status, fb = b.run_dev(ctx)
    assert status == b.run_stream(ctx)
    assert status == [CORRUPT if f % 3 == 0 else 0 for f in range(b.n)]
    assert b.run_host(ctx) == (status, fb)


@pytest.mark.parametrize("d,p", [(8, 4), (12, 4)])
def test_encode_stream_output_verifies(d, p):
    """What mec_encode_stream writes to the drives is what the scrub reads:
    a 3-block object with a short last block, every drive file intact
    through both entry points and the wrapper; then one drive rots."""
    length = 2 * MiB + 300001
    src = oracle.fill_random(length, 42 + d)
    with minio_amd.Erasure(d, p, MiB, device=0) as e:
        streams, _ = e.encode_stream(src, HH)
        t = d + p
        S = e.shard_size()
        part = e.shard_file_size(length)
        assert frames_of(part, S) == 3 and part % S != 0
        assert e.bitrot_verify_files(streams, [part] * t, [S] * t) == \
            ([0] * t, [-1] * t)
        b = Batch([(0, 1, 0, (5 * i + 1) % 8) for i in range(t)])
        b.parts, b.shards = [part] * t, [S] * t
        b.files = [np.frombuffer(s, dtype=np.uint8).copy() for s in streams]
        cur, b.offs = 0, []
        for i, f in enumerate(b.files):
            cur += ((5 * i + 1) % 8 - cur) % 8
            b.offs.append(cur)
            cur += len(f)
        assert b.run_dev(e) == ([0] * t, [-1] * t)
        assert b.run_host(e) == ([0] * t, [-1] * t)
        b.flip_msg(t - 1, 2, b.msg_len(t - 1, 2) - 1)
        b.flip_digest(2, 1, 16)
        want_st = [0] * t
        want_fb = [-1] * t
        want_st[t - 1], want_fb[t - 1] = CORRUPT, 2
        want_st[2], want_fb[2] = CORRUPT, 1
        assert b.run_dev(e) == (want_st, want_fb)
        assert b.run_host(e) == (want_st, want_fb)


# ---- large n ---------------------------------------------------------------------

def test_large_n(ctx):
    """70 000 one-frame files of 40 part bytes, three of them corrupt: n is
    not limited to 65535.  The files lie 73 bytes apart, so their phases
    cycle through all eight."""
    n, part, S, pitch = 70000, 40, 64, 73
    data = np.frombuffer(oracle.fill_random(n * part, 99), dtype=np.uint8)
    buf = np.full(n * pitch + GUARD, MARK, dtype=np.uint8)
    rows = buf[:n * pitch].reshape(n, pitch)
    rows[:, 32:72] = data.reshape(n, part)
    for f in range(n):
        rows[f, :32] = np.frombuffer(
            oracle.bitrot_sum(HH, data[f * part:(f + 1) * part].tobytes()),
            dtype=np.uint8)
    bad = (0, 65536, n - 1)
    rows[0, 32] ^= 1
    rows[65536, 71] ^= 0x80
    rows[n - 1, 31] ^= 4
    offs = [f * pitch for f in range(n)]
    status, fb = run_dev(ctx, buf, n * pitch, offs, [72] * n, [part] * n,
                         [S] * n)
    assert [f for f in range(n) if status[f] != 0] == list(bad)
    assert [status[f] for f in bad] == [CORRUPT] * 3
    assert [f for f in range(n) if fb[f] != -1] == list(bad)
    assert [fb[f] for f in bad] == [0, 0, 0]


# ---- argument errors --------------------------------------------------------------

def test_argument_errors_write_nothing(ctx):
    b = Batch([(300, 100, 1, 1), (10, 64, 2, 4), (87382 + 9, 87382, 3, 6)])
    n = b.n
    buf = b.image()
    dev = ctypes.c_void_p()
    check(lib.mec_dev_alloc(ctx._ctx, buf.nbytes, ctypes.byref(dev)))
    try:
        check(lib.mec_memcpy_h2d(ctx._ctx, dev, cptr(buf), buf.nbytes))
        good = dict(n=n, dev=dev, nbytes=b.nbytes, offs=i64arr(b.offs),
                    sizes=i64arr(b.sizes), parts=i64arr(b.parts),
                    shards=i64arr(b.shards), algo=HH)

        def call(**kw):
            a = dict(good, **kw)
            status = ctypes.create_string_buffer(b"\x77" * n, n)
            fb = i64arr([-9] * n)
            st = lib.mec_bitrot_verify_files_dev(
                ctx._ctx, a["n"], a["dev"], a["nbytes"], a["offs"],
                a["sizes"], a["parts"], a["shards"], a["algo"],
                None if kw.get("no_status") else status, fb)
            assert status.raw == b"\x77" * n and list(fb) == [-9] * n, kw
            return st

        def with_entry(values, i, v):
            out = list(values)
            out[i] = v
            return i64arr(out)

        for kw in (
            dict(n=0), dict(n=-1), dict(dev=None), dict(offs=None),
            dict(sizes=None), dict(parts=None), dict(shards=None),
            dict(no_status=True),
            dict(sizes=with_entry(b.sizes, 1, -1)),
            dict(parts=with_entry(b.parts, 2, -1)),
            dict(shards=with_entry(b.shards, 0, 0)),
            dict(shards=with_entry(b.shards, 1, -7)),
            dict(offs=with_entry(b.offs, 0, -1)),
            dict(nbytes=b.nbytes - 1),
            dict(nbytes=-1),
            dict(offs=with_entry(b.offs, 2, b.offs[2] + 1)),
            dict(algo=minio_amd.HIGHWAYHASH256),
            dict(algo=minio_amd.SHA256),
            dict(algo=minio_amd.BLAKE2B512),
            dict(algo=0),
        ):
            assert call(**kw) == INVALID, kw

        # the host-pointer variant
        ptrs = (ctypes.c_char_p * n)(*[cptr(f) for f in b.files])
        hgood = dict(n=n, ptrs=ptrs, sizes=i64arr(b.sizes),
                     parts=i64arr(b.parts), shards=i64arr(b.shards), algo=HH)

        def hcall(**kw):
            a = dict(hgood, **kw)
            status = ctypes.create_string_buffer(b"\x77" * n, n)
            fb = i64arr([-9] * n)
            st = lib.mec_bitrot_verify_files(
                ctx._ctx, a["n"], a["ptrs"], a["sizes"], a["parts"],
                a["shards"], a["algo"],
                None if kw.get("no_status") else status, fb)
            assert status.raw == b"\x77" * n and list(fb) == [-9] * n, kw
            return st

        null_file = (ctypes.c_char_p * n)(*[cptr(f) for f in b.files])
        null_file[1] = None
        for kw in (
            dict(n=0), dict(ptrs=None), dict(ptrs=null_file),
            dict(sizes=None), dict(parts=None), dict(shards=None),
            dict(no_status=True),
            dict(sizes=with_entry(b.sizes, 0, -1)),
            dict(parts=with_entry(b.parts, 0, -1)),
            dict(shards=with_entry(b.shards, 2, 0)),
            dict(algo=minio_amd.SHA256),
        ):
            assert hcall(**kw) == INVALID, kw
    finally:
        lib.mec_dev_free(ctx._ctx, dev)
    # and the same tables unharmed verify
    assert b.run_dev(ctx) == ([0] * n, [-1] * n)
