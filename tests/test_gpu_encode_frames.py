"""GPU tests of mec_encode_frames_batch_var*: batch encode, with a block
length per item, straight into the on-disk [hash||shard] frames of
streamingBitrotWriter.  Expected bytes come from the CPU oracle
(oracle.RS.encode_data, oracle.bitrot_sum, oracle.encode_stream) or from
shard files a reference server wrote, never from the library.  On the device
a marker guard lies before and after `frames` and after `data`, and every
data row's [S_i, stride_i) holds the marker too: the guards and the data
must come back unchanged and every byte of `frames` must be right."""
import ctypes
import functools
import random

import numpy as np
import pytest

import minio_amd
import oracle
import reference_shards as refs

pytestmark = pytest.mark.gpu

lib = minio_amd._lib
HH = minio_amd.HIGHWAYHASH256S
MARK = 0xA5
GUARD = 256
MiB = 1 << 20


def check(st):
    assert st == 0, (st, lib.mec_last_error())


def cptr(a):
    return a.ctypes.data_as(ctypes.c_char_p)


def i64arr(v):
    return (ctypes.c_int64 * len(v))(*v)


class Dev:
    """A host numpy array's twin on the device."""

    def __init__(self, e, host):
        self.e = e
        self.nbytes = host.nbytes
        self.ptr = ctypes.c_void_p()
        check(lib.mec_dev_alloc(e._ctx, host.nbytes, ctypes.byref(self.ptr)))
        check(lib.mec_memcpy_h2d(e._ctx, self.ptr, cptr(host), host.nbytes))

    def at(self, off):
        return ctypes.c_void_p(self.ptr.value + off)

    def get(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        check(lib.mec_memcpy_d2h(self.e._ctx, cptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        lib.mec_dev_free(self.e._ctx, self.ptr)


@functools.lru_cache(maxsize=None)
def _rs(d, p):
    return oracle.RS(d, p)


def golden_block(d, p, blk):
    """One block through the oracle: its d data rows in device layout
    (d, stride) with MARK in [S, stride), and its d+p frames, each the
    32-byte digest followed by the S shard bytes."""
    shards = _rs(d, p).encode_data(blk)
    S = len(shards[0])
    assert S == oracle.ceil_frac(len(blk), d)
    stride = (S + 63) // 64 * 64
    rows = np.full((d, stride), MARK, dtype=np.uint8)
    for k in range(d):
        rows[k, :S] = np.frombuffer(shards[k], dtype=np.uint8)
    rows.setflags(write=False)
    return blk, rows, tuple(oracle.bitrot_sum(HH, sh) + sh for sh in shards)


@functools.lru_cache(maxsize=None)
def golden(d, p, length, seed):
    """golden_block of one seeded block, computed once per distinct
    (geometry, length, seed) and shared read-only."""
    return golden_block(d, p, oracle.fill_random(length, seed))


class Batch:
    """gold: one golden_block result per item.  The host image of the packed
    data buffer followed by a guard, and the d+p expected row streams."""

    def __init__(self, d, p, bs, gold):
        self.d, self.p, self.t, self.bs = d, p, d + p, bs
        self.n = len(gold)
        self.lens = [len(g[0]) for g in gold]
        self.R = minio_amd.var_row_offsets(d, bs, self.lens)
        self.F = minio_amd.frame_offsets(d, bs, self.lens)
        self.Fn = self.F[-1]
        self.data = np.full(d * self.R[-1] + GUARD, MARK, dtype=np.uint8)
        for i, g in enumerate(gold):
            self.data[d * self.R[i]:d * self.R[i] + g[1].size] = g[1].ravel()
        self.want = [b"".join(g[2][s] for g in gold) for s in range(self.t)]
        assert all(len(w) == self.Fn for w in self.want)
        self.nbytes = self.t * self.Fn

    @classmethod
    def seeded(cls, d, p, bs, specs):
        return cls(d, p, bs, [golden(d, p, ln, seed) for ln, seed in specs])

    def upload(self, e, shift=0):
        """Returns (data pointer, frames pointer): frames lies `shift` bytes
        behind a 256-byte guard at the start of its allocation."""
        self.shift = shift
        self.ddev = Dev(e, self.data)
        self.fdev = Dev(e, np.full(GUARD + shift + self.nbytes + GUARD, MARK,
                                   dtype=np.uint8))
        return self.ddev.ptr, self.fdev.at(GUARD + shift)

    def download(self):
        out = self.ddev.get(), self.fdev.get()
        self.ddev.free()
        self.fdev.free()
        return out

    def untouched(self, got):
        return (got[0] == self.data).all() and (got[1] == MARK).all()

    def streams(self, got):
        gd, gf = got
        lo = GUARD + self.shift
        assert (gd == self.data).all(), "the data buffer (or its guard) changed"
        assert (gf[:lo] == MARK).all(), "guard before frames"
        assert (gf[lo + self.nbytes:] == MARK).all(), "guard after frames"
        body = gf[lo:lo + self.nbytes].tobytes()
        return [body[s * self.Fn:(s + 1) * self.Fn] for s in range(self.t)]

    def verify(self, got):
        for s, (g, w) in enumerate(zip(self.streams(got), self.want)):
            if g != w:
                ga = np.frombuffer(g, dtype=np.uint8)
                wa = np.frombuffer(w, dtype=np.uint8)
                bad = np.flatnonzero(ga != wa)
                item = np.searchsorted(self.F, bad[0], side="right") - 1
                raise AssertionError(
                    f"row {s}: {bad.size} wrong bytes, first at {bad[0]} = "
                    f"frame {item} + {bad[0] - self.F[item]} "
                    f"(len {self.lens[item]})")


def run_dev(e, b, fn=None, algo=HH, lens=None, shift=0):
    """One device call on b; returns (status, (data, frames) buffers)."""
    fn = fn or lib.mec_encode_frames_batch_var_dev
    pd, pf = b.upload(e, shift)
    lens = b.lens if lens is None else lens
    rc = fn(e._ctx, len(lens), pd, i64arr(lens), pf, algo)
    return rc, b.download()


# ---- 1. files a reference server wrote ------------------------------------

def test_reference_written_files():
    """One call per geometry over every complete reference object: slice
    [F_first, F_last+1) of row s is the file that lay on row s's drive.
    Nothing is computed on the expected side."""
    groups = {}
    for obj in refs.COMPLETE:
        groups.setdefault((obj.d, obj.p, obj.block_size), []).append(obj)
    assert {(d, p): sorted(o.size for o in objs)
            for (d, p, _), objs in groups.items()} == \
        {(2, 2): [228, 228, 19113], (3, 2): [644520]}
    for (d, p, bs), objs in groups.items():
        blocks, span = [], []
        for obj in objs:
            data = obj.data()
            first = len(blocks)
            blocks += [data[o:o + bs] for o in range(0, len(data), bs)]
            span.append((first, len(blocks)))
        b = Batch(d, p, bs, [golden_block(d, p, blk) for blk in blocks])
        with minio_amd.Erasure(d, p, bs) as e:
            rc, got = run_dev(e, b)
        assert rc == 0
        rows = b.streams(got)
        for obj, (first, last) in zip(objs, span):
            for s in range(d + p):
                assert rows[s][b.F[first]:b.F[last]] == obj.bins[s], \
                    (obj.name, s)


# ---- 2. thresholds --------------------------------------------------------

def threshold_lengths():
    lens = []
    for S in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 511, 512,
              513, 2047, 2048, 2049):
        lens += [8 * S - 3, 8 * S]
    lens += [8 * (512 + r) for r in range(32)]   # every len % 32 residue
    lens += [MiB - 1, MiB]
    random.Random(0x6672616d).shuffle(lens)
    return lens


def shard_phases(b, base):
    """(phase, S) of every shard start address of the batch."""
    return [((base + s * b.Fn + b.F[i] + 32) % 16,
             oracle.ceil_frac(b.lens[i], b.d))
            for s in range(b.t) for i in range(b.n)]


def test_thresholds():
    d, p = 8, 4
    lens = threshold_lengths()
    assert len(lens) == 74
    b = Batch.seeded(d, p, MiB, [(ln, 1000 + i) for i, ln in enumerate(lens)])
    for base in (0, 1):
        ph = shard_phases(b, base)
        assert {f for f, _ in ph} == set(range(16)), base
        assert any(f % 2 and S < 16 for f, S in ph), base
        assert any(f % 2 and S >= 48 for f, S in ph), base
    with minio_amd.Erasure(d, p, MiB) as e:
        for shift in (0, 1):
            rc, got = run_dev(e, b, shift=shift)
            assert rc == 0
            b.verify(got)


# ---- 3. geometries --------------------------------------------------------

@pytest.mark.parametrize("d,p", [(2, 2), (4, 2), (12, 4), (16, 4)])
def test_geometries(d, p):
    rng = random.Random(0x67656f + d)
    lens = [rng.randint(1, 64 << 10) for _ in range(20)] + [MiB]
    rng.shuffle(lens)
    b = Batch.seeded(d, p, MiB, [(ln, 2000 + 100 * d + i)
                                 for i, ln in enumerate(lens)])
    if d == 12:
        assert oracle.ceil_frac(MiB, d) == 87382
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
    assert rc == 0
    b.verify(got)


# ---- 4. many tiny items ---------------------------------------------------

def test_many_tiny_items():
    """n > 65535 with frames of 33..64 bytes, so every granule is a boundary
    granule, and one 1 MiB item in the middle: the long frame follows short
    ones inside one wave's lookup.  Contents cycle over 63 distinct
    blocks."""
    d, p, n = 8, 4, 66000
    rng = random.Random(0x74696e79)
    distinct = [(ln, 3000 + k) for k, ln in
                enumerate([1, 255, 256] + rng.sample(range(2, 255), 60))]
    assert len(distinct) == 63
    specs = [distinct[rng.randrange(63)] for _ in range(n)]
    specs[n // 2] = (MiB, 3999)
    sizes = {32 + oracle.ceil_frac(ln, d) for ln, _ in distinct}
    assert min(sizes) == 33 and max(sizes) == 64
    b = Batch.seeded(d, p, MiB, specs)
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
    assert rc == 0
    b.verify(got)


# ---- 5. a multi-block object ----------------------------------------------

def test_multi_block_object_is_its_shard_files():
    d, p, t = 12, 4, 16
    size = 2 * MiB + 300001
    data = oracle.fill_random(size, 0x6f626a)
    blocks = [data[o:o + MiB] for o in range(0, size, MiB)]
    assert [len(x) for x in blocks] == [MiB, MiB, 300001]
    b = Batch(d, p, MiB, [golden_block(d, p, blk) for blk in blocks])
    want, _ = oracle.encode_stream(d, p, MiB, data, HH)
    assert b.want == want
    S = oracle.ceil_frac(MiB, d)
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
        assert rc == 0
        rows = b.streams(got)
        assert rows == want
        assert e.encode_stream(data, HH)[0] == rows
        part = e.shard_file_size(size)
        assert len(rows[0]) == minio_amd.bitrot_shard_file_size(part, S, HH)
        status, first_bad = e.bitrot_verify_files(rows, [part] * t, [S] * t)
        assert status == [0] * t and first_bad == [-1] * t
        hit = bytearray(rows[5])
        hit[b.F[1] + 32 + 777] ^= 0x10
        files = rows[:5] + [bytes(hit)] + rows[6:]
        status, first_bad = e.bitrot_verify_files(files, [part] * t, [S] * t)
        assert status == [0] * 5 + [5] + [0] * 10
        assert first_bad == [-1] * 5 + [1] + [-1] * 10


# ---- 6. async -------------------------------------------------------------

def test_two_async_calls_back_to_back():
    """Different length tables, two output buffers, the second batch larger
    so the context's scratch grows between the calls; one sync at the end."""
    d, p = 8, 4
    rng = random.Random(0x6173796e)
    a = Batch.seeded(d, p, MiB, [(rng.randint(1, 3000), 5000 + i)
                                 for i in range(24)])
    b = Batch.seeded(d, p, MiB, [(rng.randint(1, 200000), 5100 + i)
                                 for i in range(37)])
    assert b.R[-1] > 2 * a.R[-1] and b.n > a.n
    with minio_amd.Erasure(d, p, MiB) as e:
        pa, pb = a.upload(e), b.upload(e, shift=5)
        fn = lib.mec_encode_frames_batch_var_dev_async
        rc_a = fn(e._ctx, a.n, pa[0], i64arr(a.lens), pa[1], HH)
        rc_b = fn(e._ctx, b.n, pb[0], i64arr(b.lens), pb[1], HH)
        check(lib.mec_stream_sync(e._ctx))
        ga, gb = a.download(), b.download()
    assert rc_a == 0 and rc_b == 0
    a.verify(ga)
    b.verify(gb)


# ---- 7. argument errors ---------------------------------------------------

def test_argument_errors_touch_nothing():
    d, p = 8, 4
    bs = 64 << 10
    lens = [100, 4096, bs]
    b = Batch.seeded(d, p, bs, [(ln, 7000 + i) for i, ln in enumerate(lens)])
    with minio_amd.Erasure(d, p, bs) as e:
        for fn in (lib.mec_encode_frames_batch_var_dev,
                   lib.mec_encode_frames_batch_var_dev_async):
            for algo in (minio_amd.SHA256, minio_amd.BLAKE2B512, 0, 5):
                rc, got = run_dev(e, b, fn=fn, algo=algo)
                assert rc == 6 and b.untouched(got), algo
            for bad in ([100, 0, bs], [100, 4096, bs + 1], [-5, 4096, bs]):
                rc, got = run_dev(e, b, fn=fn, lens=bad)
                assert rc == 6 and b.untouched(got), bad
            pd, pf = b.upload(e)
            la = i64arr(lens)
            assert fn(e._ctx, 0, pd, la, pf, HH) == 6
            assert fn(e._ctx, -1, pd, la, pf, HH) == 6
            assert fn(e._ctx, 3, None, la, pf, HH) == 6
            assert fn(e._ctx, 3, pd, None, pf, HH) == 6
            assert fn(e._ctx, 3, pd, la, None, HH) == 6
            # n*(d+p) past 32 bits: refused before the lengths are read
            assert fn(e._ctx, 2**31 - 1, pd, la, pf, HH) == 6
            check(lib.mec_stream_sync(e._ctx))
            assert b.untouched(b.download())
        # the host-pointer variant refuses the same
        out = np.full(b.nbytes + GUARD, MARK, dtype=np.uint8)
        blob = b"x" * sum(lens)
        hfn = lib.mec_encode_frames_batch_var
        assert hfn(e._ctx, 3, blob, i64arr(lens), cptr(out),
                   minio_amd.SHA256) == 6
        assert hfn(e._ctx, 3, blob, i64arr([100, 0, bs]), cptr(out), HH) == 6
        assert hfn(e._ctx, 0, blob, i64arr(lens), cptr(out), HH) == 6
        assert hfn(e._ctx, 3, None, i64arr(lens), cptr(out), HH) == 6
        assert hfn(e._ctx, 3, blob, i64arr(lens), None, HH) == 6
        assert (out == MARK).all()
        # after all the refusals the context still encodes
        rc, got = run_dev(e, b, algo=minio_amd.HIGHWAYHASH256)
        assert rc == 0
        b.verify(got)
    # a geometry without a compiled specialisation
    with minio_amd.Erasure(5, 2, bs) as e:
        u = Batch.seeded(5, 2, bs, [(ln, 7100 + i)
                                    for i, ln in enumerate(lens)])
        for fn in (lib.mec_encode_frames_batch_var_dev,
                   lib.mec_encode_frames_batch_var_dev_async):
            rc, got = run_dev(e, u, fn=fn)
            assert rc == 6 and u.untouched(got)
            msg = lib.mec_last_error()
            assert b"specialization" in msg and b"EC5+2" in msg
        out = np.full(u.nbytes + GUARD, MARK, dtype=np.uint8)
        assert lib.mec_encode_frames_batch_var(
            e._ctx, 3, b"x" * sum(lens), i64arr(lens), cptr(out), HH) == 6
        assert b"EC5+2" in lib.mec_last_error()
        assert (out == MARK).all()


# ---- 8. host-pointer variant and Python -----------------------------------

def mix40():
    rng = random.Random(0x6d6978)
    lens = [1, 7, 8, 9, 255, 256, 257, 4096, 8 * 513 - 3, 65536, 700001, MiB]
    lens += [rng.randint(1, 20000) for _ in range(28)]
    rng.shuffle(lens)
    assert len(lens) == 40
    return [(ln, 8000 + i) for i, ln in enumerate(lens)]


def test_host_pointer_variant_and_python():
    d, p = 8, 4
    specs = mix40()
    b = Batch.seeded(d, p, MiB, specs)
    blocks = [golden(d, p, ln, seed)[0] for ln, seed in specs]
    out = np.full(b.nbytes + GUARD, MARK, dtype=np.uint8)
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
        assert rc == 0
        dev_rows = b.streams(got)
        check(lib.mec_encode_frames_batch_var(
            e._ctx, b.n, b"".join(blocks), i64arr(b.lens), cptr(out), HH))
        rows, off = e.encode_frames_batch_var(blocks)
        rows2, off2 = e.encode_frames_batch_var(blocks[:5],
                                                minio_amd.HIGHWAYHASH256)
        assert e.encode_frames_batch_var([]) == ([b""] * (d + p), [0])
        with pytest.raises(minio_amd.MecError):
            e.encode_frames_batch_var(blocks[:2], minio_amd.SHA256)
        with pytest.raises(minio_amd.MecError):
            e.encode_frames_batch_var([b"", b"x"])
    assert (out[b.nbytes:] == MARK).all(), "guard after frames"
    assert out[:b.nbytes].tobytes() == b"".join(dev_rows)
    assert dev_rows == b.want
    assert rows == dev_rows and off == b.F
    assert off2 == b.F[:6]
    assert rows2 == [r[:off2[-1]] for r in rows]
