"""GPU tests of mec_encode_batch_var*: batch encode + bitrot digests with a
different block length per item (a PUT batch across objects).  Expected
parity and digests come from the CPU oracle (oracle.RS.encode_data,
oracle.bitrot_sum), bit-exact.  Every data row's [S_i, stride_i) and the
whole parity and sums buffers are prefilled with a marker, and a marker
guard follows each buffer's end: the data buffer and all guards must come
back unchanged, parity[:S_i] and every digest must match."""
import ctypes
import functools
import random

import numpy as np
import pytest

import minio_amd
import oracle

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

    def get(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        check(lib.mec_memcpy_d2h(self.e._ctx, cptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        lib.mec_dev_free(self.e._ctx, self.ptr)


@functools.lru_cache(maxsize=None)
def _rs(d, p):
    return oracle.RS(d, p)


@functools.lru_cache(maxsize=None)
def golden(d, p, length, seed):
    """One seeded block through the oracle, computed once per distinct
    (geometry, length, seed) and shared read-only: the block, its d data
    rows in device layout (d, stride) with MARK in [S, stride), the p
    parity rows (p, S) and the d+p digests (d+p, 32)."""
    blk = oracle.fill_random(length, seed)
    shards = _rs(d, p).encode_data(blk)
    S = len(shards[0])
    assert S == oracle.ceil_frac(length, d)
    stride = (S + 63) // 64 * 64
    rows = np.full((d, stride), MARK, dtype=np.uint8)
    for k in range(d):
        rows[k, :S] = np.frombuffer(shards[k], dtype=np.uint8)
    par = np.stack([np.frombuffer(sh, dtype=np.uint8) for sh in shards[d:]])
    dig = np.stack([np.frombuffer(oracle.bitrot_sum(HH, sh), dtype=np.uint8)
                    for sh in shards])
    for a in (rows, par, dig):
        a.setflags(write=False)
    return blk, rows, par, dig


class Batch:
    """specs: one (length, seed) per item.  Host images of the three device
    buffers in the packed layout, each followed by a guard."""

    def __init__(self, d, p, bs, specs):
        self.d, self.p, self.t, self.specs = d, p, d + p, specs
        self.n = len(specs)
        self.lens = [ln for ln, _ in specs]
        self.R = minio_amd.var_row_offsets(d, bs, self.lens)
        Rn = self.R[-1]
        self.data = np.full(d * Rn + GUARD, MARK, dtype=np.uint8)
        for i, (ln, seed) in enumerate(specs):
            rows = golden(d, p, ln, seed)[1]
            self.data[d * self.R[i]:d * self.R[i] + rows.size] = rows.ravel()
        self.parity = np.full(p * Rn + GUARD, MARK, dtype=np.uint8)
        self.sums = np.full(self.n * self.t * 32 + GUARD, MARK,
                            dtype=np.uint8)

    def upload(self, e):
        self.dev = [Dev(e, a) for a in (self.data, self.parity, self.sums)]
        return [dv.ptr for dv in self.dev]

    def download(self):
        out = [dv.get() for dv in self.dev]
        for dv in self.dev:
            dv.free()
        return out

    def untouched(self, got):
        return all((g == h).all() for g, h in
                   zip(got, (self.data, self.parity, self.sums)))

    def verify(self, got, sums=True):
        gd, gp, gs = got
        d, p, t, n, R = self.d, self.p, self.t, self.n, self.R
        assert (gd == self.data).all(), "the data buffer (or its guard) changed"
        assert (gp[p * R[-1]:] == MARK).all(), "parity guard"
        assert (gs[n * t * 32:] == MARK).all(), "sums guard"
        for i, (ln, seed) in enumerate(self.specs):
            _, rows, par, _ = golden(d, p, ln, seed)
            S, stride = par.shape[1], rows.shape[1]
            g = gp[p * R[i]:p * R[i] + p * stride].reshape(p, stride)[:, :S]
            assert (g == par).all(), \
                f"parity of item {i} (len {ln}): rows " \
                f"{np.argwhere((g != par).any(axis=1)).ravel().tolist()}"
        if not sums:
            assert (gs == MARK).all(), "sums written under sums_dev = NULL"
            return
        want = np.stack([golden(d, p, ln, seed)[3] for ln, seed in self.specs])
        gdig = gs[:n * t * 32].reshape(n, t, 32)
        wrong = np.argwhere((gdig != want).any(axis=2))
        assert wrong.size == 0, \
            f"first wrong digests (item,row): {wrong[:6].tolist()}, " \
            f"lens {[self.lens[i] for i, _ in wrong[:6]]}"


def run_dev(e, b, fn=None, sums=True, algo=HH, lens=None):
    """One device call on b; returns (status, the three buffers)."""
    fn = fn or lib.mec_encode_batch_var_dev
    pd, pp, ps = b.upload(e)
    lens = b.lens if lens is None else lens
    rc = fn(e._ctx, len(lens), pd, i64arr(lens), pp, algo,
            ps if sums else None)
    return rc, b.download()


# ---- 1. thresholds --------------------------------------------------------

def threshold_lengths():
    lens = [1, 7, 8, 9]                    # S = 1, all-padding tails, S = 2
    lens += [8 * (512 + r) for r in range(32)]   # every len % 32 residue
    for S in (31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537,
              2047, 2048, 2049):           # double-buffer branches, stride
        lens += [8 * S - 3, 8 * S]
    lens += [MiB - 1, MiB]
    random.Random(0x7468).shuffle(lens)
    return lens


def test_thresholds():
    d, p = 8, 4
    lens = threshold_lengths()
    assert len(lens) == 68
    b = Batch(d, p, MiB, [(ln, 1000 + i) for i, ln in enumerate(lens)])
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
    assert rc == 0
    b.verify(got)


# ---- 2. geometries --------------------------------------------------------

@pytest.mark.parametrize("d,p", [(2, 2), (4, 2), (12, 4), (16, 4)])
def test_geometries(d, p):
    rng = random.Random(0x67656f + d)
    lens = [rng.randint(1, 64 << 10) for _ in range(20)] + [MiB]
    rng.shuffle(lens)
    b = Batch(d, p, MiB, [(ln, 2000 + 100 * d + i)
                          for i, ln in enumerate(lens)])
    if d == 12:
        assert oracle.ceil_frac(MiB, d) == 87382
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
    assert rc == 0
    b.verify(got)


# ---- 3. many tiny items ---------------------------------------------------

def test_many_tiny_items():
    """n > 65535, one or two columns per item, one 1 MiB item in the
    middle: the lane-to-item lookup across workgroup boundaries and the
    descending-length order.  Contents cycle over 63 distinct blocks."""
    d, p, n = 8, 4, 66000
    rng = random.Random(0x74696e79)
    distinct = [(ln, 3000 + k) for k, ln in
                enumerate([1, 255, 256] + rng.sample(range(2, 255), 60))]
    assert len(distinct) == 63
    specs = [distinct[rng.randrange(63)] for _ in range(n)]
    specs[n // 2] = (MiB, 3999)
    cols = {-(-oracle.ceil_frac(ln, d) // 32) for ln, _ in distinct}
    assert cols == {1}, "one column each at EC8+4"
    b = Batch(d, p, MiB, specs)
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
    assert rc == 0
    b.verify(got)


def test_two_column_items():
    """EC2+2 with lengths in [1, 256]: S up to 128, so up to four columns
    per item and waves that mix items of one to four columns."""
    d, p, n = 2, 2, 3000
    rng = random.Random(0x32636f6c)
    distinct = [(ln, 3500 + k) for k, ln in
                enumerate(rng.sample(range(1, 257), 64))]
    specs = [distinct[rng.randrange(64)] for _ in range(n)]
    b = Batch(d, p, MiB, specs)
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
    assert rc == 0
    b.verify(got)


# ---- 4. equal lengths agree with the uniform call -------------------------

@pytest.mark.parametrize("L", [MiB, 700001])
def test_equal_lengths_match_uniform_call(L):
    d, p, n = 8, 4, 5
    t = d + p
    b = Batch(d, p, MiB, [(L, 4000 + i) for i in range(n)])
    S = oracle.ceil_frac(L, d)
    vstride = (S + 63) // 64 * 64
    with minio_amd.Erasure(d, p, MiB) as e:
        rc, got = run_dev(e, b)
        # the same rows at the uniform call's fixed stride
        ustride = lib.mec_shard_stride(MiB, d)
        udata = np.full((n, d, ustride), MARK, dtype=np.uint8)
        for i, (ln, seed) in enumerate(b.specs):
            udata[i, :, :S] = golden(d, p, ln, seed)[1][:, :S]
        dd = Dev(e, udata)
        dp = Dev(e, np.full(n * p * ustride, MARK, dtype=np.uint8))
        ds = Dev(e, np.full(n * t * 32, MARK, dtype=np.uint8))
        check(lib.mec_encode_batch_dev(e._ctx, n, dd.ptr, L, dp.ptr, HH,
                                       ds.ptr))
        upar = dp.get().reshape(n, p, ustride)
        usum = ds.get()
        for dv in (dd, dp, ds):
            dv.free()
    assert rc == 0
    b.verify(got)
    _, gp, gs = got
    for i in range(n):
        rows = gp[p * b.R[i]:p * b.R[i] + p * vstride].reshape(p, vstride)
        for r in range(p):
            assert (rows[r, :S] == upar[i, r, :S]).all(), (i, r)
    assert (gs[:n * t * 32] == usum).all()


# ---- 5. async -------------------------------------------------------------

def test_two_async_calls_back_to_back():
    d, p = 8, 4
    rng = random.Random(0x6173796e)
    a = Batch(d, p, MiB, [(rng.randint(1, 200000), 5000 + i)
                          for i in range(24)])
    b = Batch(d, p, MiB, [(rng.randint(1, 3000), 5100 + i)
                          for i in range(37)])
    with minio_amd.Erasure(d, p, MiB) as e:
        pa, pb = a.upload(e), b.upload(e)
        fn = lib.mec_encode_batch_var_dev_async
        rc_a = fn(e._ctx, a.n, pa[0], i64arr(a.lens), pa[1], HH, pa[2])
        rc_b = fn(e._ctx, b.n, pb[0], i64arr(b.lens), pb[1], HH, pb[2])
        check(lib.mec_stream_sync(e._ctx))
        ga, gb = a.download(), b.download()
    assert rc_a == 0 and rc_b == 0
    a.verify(ga)
    b.verify(gb)


# ---- 6. null sums ---------------------------------------------------------

def test_null_sums_is_encode_only():
    d, p = 8, 4
    lens = [1, 100, 4096, 8 * 513 - 3, 70000, MiB]
    b = Batch(d, p, MiB, [(ln, 6000 + i) for i, ln in enumerate(lens)])
    with minio_amd.Erasure(d, p, MiB) as e:
        # no digests asked for: the algorithm id is not looked at
        rc, got = run_dev(e, b, sums=False, algo=minio_amd.SHA256)
    assert rc == 0
    b.verify(got, sums=False)


# ---- 7. argument errors ---------------------------------------------------

def test_argument_errors_touch_nothing():
    d, p = 8, 4
    bs = 64 << 10
    lens = [100, 4096, bs]
    b = Batch(d, p, bs, [(ln, 7000 + i) for i, ln in enumerate(lens)])
    with minio_amd.Erasure(d, p, bs) as e:
        for fn in (lib.mec_encode_batch_var_dev,
                   lib.mec_encode_batch_var_dev_async):
            for algo in (minio_amd.SHA256, minio_amd.BLAKE2B512, 0, 5):
                rc, got = run_dev(e, b, fn=fn, algo=algo)
                assert rc == 6 and b.untouched(got), algo
            for bad in ([100, 0, bs], [100, 4096, bs + 1], [-5, 4096, bs]):
                rc, got = run_dev(e, b, fn=fn, lens=bad)
                assert rc == 6 and b.untouched(got), bad
        pd, pp, ps = b.upload(e)
        la = i64arr(lens)
        fn = lib.mec_encode_batch_var_dev
        assert fn(e._ctx, 0, pd, la, pp, HH, ps) == 6
        assert fn(e._ctx, -1, pd, la, pp, HH, ps) == 6
        assert fn(e._ctx, 3, None, la, pp, HH, ps) == 6
        assert fn(e._ctx, 3, pd, None, pp, HH, ps) == 6
        assert fn(e._ctx, 3, pd, la, None, HH, ps) == 6
        assert b.untouched(b.download())
        # after all the refusals the context still encodes
        rc, got = run_dev(e, b, algo=minio_amd.HIGHWAYHASH256)
        assert rc == 0
        b.verify(got)
    # a geometry without a compiled specialisation
    with minio_amd.Erasure(5, 2, bs) as e:
        u = Batch(5, 2, bs, [(ln, 7100 + i) for i, ln in enumerate(lens)])
        for sums in (True, False):
            rc, got = run_dev(e, u, sums=sums)
            assert rc == 6 and u.untouched(got)
            assert b"specialization" in lib.mec_last_error()
        par = ctypes.create_string_buffer(1 << 16)
        assert lib.mec_encode_batch_var(e._ctx, 1, b"x" * 100, i64arr([100]),
                                        par, HH, None) == 6


# ---- 8. host-pointer variant and Python -----------------------------------

def mix40():
    rng = random.Random(0x6d6978)
    lens = [1, 7, 8, 9, 255, 256, 257, 4096, 8 * 513 - 3, 65536, 700001, MiB]
    lens += [rng.randint(1, 20000) for _ in range(28)]
    rng.shuffle(lens)
    assert len(lens) == 40
    return [(ln, 8000 + i) for i, ln in enumerate(lens)]


def test_host_pointer_variant():
    d, p = 8, 4
    t = d + p
    specs = mix40()
    n = len(specs)
    gold = [golden(d, p, ln, seed) for ln, seed in specs]
    data = b"".join(g[0] for g in gold)
    par_len = sum(g[2].size for g in gold)
    for with_sums in (True, False):
        parity = np.full(par_len + GUARD, MARK, dtype=np.uint8)
        sums = np.full(n * t * 32 + GUARD, MARK, dtype=np.uint8)
        with minio_amd.Erasure(d, p, MiB) as e:
            check(lib.mec_encode_batch_var(
                e._ctx, n, data, i64arr([ln for ln, _ in specs]),
                cptr(parity), HH, cptr(sums) if with_sums else None))
        assert (parity[par_len:] == MARK).all()
        assert (sums[n * t * 32:] == MARK).all()
        want = np.concatenate([g[2].ravel() for g in gold])
        assert (parity[:par_len] == want).all()
        if with_sums:
            assert (sums[:n * t * 32].reshape(n, t, 32) ==
                    np.stack([g[3] for g in gold])).all()
        else:
            assert (sums == MARK).all()


def test_python_encode_batch_var():
    d, p = 8, 4
    specs = mix40()
    blocks = [golden(d, p, ln, seed)[0] for ln, seed in specs]
    rs = _rs(d, p)
    with minio_amd.Erasure(d, p, MiB) as e:
        shards, sums = e.encode_batch_var(blocks, HH)
        shards2, none = e.encode_batch_var(blocks[:5])
        assert e.encode_batch_var([]) == ([], None)
        with pytest.raises(minio_amd.MecError):
            e.encode_batch_var(blocks[:2], minio_amd.SHA256)
        with pytest.raises(minio_amd.MecError):
            e.encode_batch_var([b"", b"x"], HH)
    assert none is None and shards2 == shards[:5]
    for i, blk in enumerate(blocks):
        want = rs.encode_data(blk)
        assert shards[i] == want, i
        for s, sh in enumerate(want):
            assert sums[i][s] == oracle.bitrot_sum(HH, sh), (i, s)
