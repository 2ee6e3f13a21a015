"""GPU tests of mec_verify_reconstruct_batch_var*: the verified batch read
with a different shard length per item (a GET or heal batch across objects,
parallelReader.Read's shortened last block, cmd/erasure-decode.go:138-139).
Rows and digests come from the CPU oracle (oracle.RS, oracle.bitrot_sum),
bit-exact, built per item at its own length.  Rows that were not read, their
digest slots, every row's bytes in [S_i, stride_i) and a guard behind each
buffer are prefilled with a marker that must never influence a result and,
outside the scratch tails of rebuilt rows, must come back unchanged."""
import ctypes
import functools

import numpy as np
import pytest

import minio_amd
import oracle

pytestmark = pytest.mark.gpu

lib = minio_amd._lib
HH = minio_amd.HIGHWAYHASH256S
TOO_FEW = 3
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
    (geometry, length, seed) and shared read-only: rows (d+p, S) and digests
    (d+p, 32)."""
    shards = _rs(d, p).encode_data(oracle.fill_random(length, seed))
    assert len(shards[0]) == oracle.ceil_frac(length, d)
    rows = np.stack([np.frombuffer(sh, dtype=np.uint8) for sh in shards])
    dig = np.stack([np.frombuffer(oracle.bitrot_sum(HH, sh), dtype=np.uint8)
                    for sh in shards])
    rows.setflags(write=False)
    dig.setflags(write=False)
    return rows, dig


class Batch:
    """specs: one (length, seed) per item; read: (n, d+p) flags.  buf and dig
    are the host images of the two device buffers in the packed layout, each
    followed by a guard: rows and digests where read, MARK everywhere else."""

    def __init__(self, d, p, bs, specs, read):
        self.d, self.p, self.t, self.bs = d, p, d + p, bs
        self.n = len(specs)
        self.specs = specs
        self.lens = [ln for ln, _ in specs]
        self.S = [oracle.ceil_frac(ln, d) for ln in self.lens]
        self.stride = [(S + 63) // 64 * 64 for S in self.S]
        self.R = minio_amd.var_row_offsets(d, bs, self.lens)
        self.read = np.asarray(read, dtype=np.uint8).reshape(self.n, self.t)
        self.bad = np.zeros((self.n, self.t), dtype=bool)
        self.buf = np.full(self.t * self.R[-1] + GUARD, MARK, dtype=np.uint8)
        self.dig = np.full(self.n * self.t * 32 + GUARD, MARK, dtype=np.uint8)
        for i, (ln, seed) in enumerate(specs):
            rows, dig = golden(d, p, ln, seed)
            for s in range(self.t):
                if self.read[i, s]:
                    o = self.off(i, s)
                    self.buf[o:o + self.S[i]] = rows[s]
                    c = i * self.t + s
                    self.dig[c * 32:(c + 1) * 32] = dig[s]

    def off(self, i, s):
        return self.t * self.R[i] + s * self.stride[i]

    def flip(self, i, s, byte, bit=0):
        """Bitrot in a row that was read."""
        assert self.read[i, s] and 0 <= byte < self.S[i]
        self.buf[self.off(i, s) + byte] ^= np.uint8(1 << bit)
        self.bad[i, s] = True

    def flip_digest(self, i, s, byte, bit=0):
        assert self.read[i, s]
        self.dig[(i * self.t + s) * 32 + byte] ^= np.uint8(1 << bit)
        self.bad[i, s] = True

    @property
    def verified(self):
        return (self.read != 0) & ~self.bad

    def expect(self, data_only, rehash):
        """What the call must leave, from oracle.RS.reconstruct on the
        verified mask: (rows, compare mask, digests, statuses)."""
        want, wdig = self.buf.copy(), self.dig.copy()
        cmp = np.ones(self.buf.shape, dtype=bool)
        scope = self.d if data_only else self.t
        st = []
        for i in range(self.n):
            v, S = self.verified[i], self.S[i]
            if v.sum() < self.d:
                st.append(TOO_FEW)
                continue
            st.append(0)
            if v[:scope].all():
                continue
            ref = _rs(self.d, self.p).reconstruct(
                [bytes(self.buf[self.off(i, s):self.off(i, s) + S])
                 if v[s] else None for s in range(self.t)],
                data_only=bool(data_only))
            true_rows, true_dig = golden(self.d, self.p, *self.specs[i])
            for s in range(scope):
                if v[s]:
                    continue
                o = self.off(i, s)
                want[o:o + S] = np.frombuffer(ref[s], dtype=np.uint8)
                assert (want[o:o + S] == true_rows[s]).all()
                cmp[o + S:o + self.stride[i]] = False   # scratch
                if rehash:
                    c = i * self.t + s
                    wdig[c * 32:(c + 1) * 32] = true_dig[s]
        return want, cmp, wdig, st


def call(e, b, data_only=0, rehash=0, algo=HH, status=True, fn=None, n=None,
         lens=None, null=()):
    """One device call on b's images.  Returns (rc, present, statuses, rows,
    digests); present and statuses are prefilled with 0xEE."""
    ds, dd = Dev(e, b.buf), Dev(e, b.dig)
    n = b.n if n is None else n
    present = ctypes.create_string_buffer(b"\xee" * b.read.size, b.read.size)
    st = ctypes.create_string_buffer(b"\xee" * b.n, b.n) if status else None
    fn = fn or lib.mec_verify_reconstruct_batch_var_dev
    rc = fn(e._ctx, n,
            None if "shards" in null else ds.ptr,
            None if "sums" in null else dd.ptr,
            None if "lens" in null else i64arr(b.lens if lens is None
                                               else lens),
            None if "mask" in null else b.read.tobytes(), algo, data_only,
            rehash, present, st)
    got, gdig = ds.get(), dd.get()
    ds.free()
    dd.free()
    pres = np.frombuffer(present.raw, dtype=np.uint8).reshape(b.read.shape)
    return rc, pres, (list(st.raw) if status else None), got, gdig


def run_and_check(e, b, data_only=0, rehash=0, algo=HH):
    """One call; checks present_out, statuses, every byte outside the
    scratch tails (guards included) and every digest slot."""
    rc, pres, st, got, gdig = call(e, b, data_only, rehash, algo)
    assert rc == 0, (rc, lib.mec_last_error())
    assert (pres == b.verified).all(), np.argwhere(pres != b.verified)[:4]
    want, cmp, wdig, wst = b.expect(data_only, rehash)
    assert st == wst
    wrong = np.flatnonzero((got != want) & cmp)
    assert wrong.size == 0, \
        f"first wrong row bytes at {wrong[:6].tolist()}, R = {b.R[:8]}"
    wrong = np.flatnonzero(gdig != wdig)
    assert wrong.size == 0, \
        f"first wrong digest chains: {sorted(set(wrong // 32))[:6]}"
    return got, gdig, st


def one_down(n, total, shift=0):
    """One drive down, round-robin: item i has not read row (i+shift)%total."""
    read = np.ones((n, total), dtype=np.uint8)
    read[np.arange(n), (np.arange(n) + shift) % total] = 0
    return read


# ---- 1. round trip from the write side ------------------------------------

@pytest.mark.parametrize("rehash", [0, 1])
def test_round_trip_from_encode_batch_var(rehash):
    """mec_encode_batch_var_dev's data, parity and sums, re-laid on the host
    into the single rows buffer, one row per item dropped and one corrupted:
    the rows come back bit-exact and, with rehash, so do the digests."""
    d, p = 8, 4
    t = d + p
    lens = [1, 8, 4096, 4097, 70001, 8 * 2049, 300, MiB, 8 * 512, 33, 65537]
    n = len(lens)
    R = minio_amd.var_row_offsets(d, MiB, lens)
    S = [oracle.ceil_frac(ln, d) for ln in lens]
    stride = [(s + 63) // 64 * 64 for s in S]
    data = np.full(d * R[-1], MARK, dtype=np.uint8)
    for i, ln in enumerate(lens):
        rows = golden(d, p, ln, 7000 + i)[0]
        for k in range(d):
            o = d * R[i] + k * stride[i]
            data[o:o + S[i]] = rows[k]
    with minio_amd.Erasure(d, p, MiB) as e:
        dd = Dev(e, data)
        dp = Dev(e, np.full(p * R[-1], MARK, dtype=np.uint8))
        dsum = Dev(e, np.full(n * t * 32, MARK, dtype=np.uint8))
        check(lib.mec_encode_batch_var_dev(e._ctx, n, dd.ptr, i64arr(lens),
                                           dp.ptr, HH, dsum.ptr))
        par, sums = dp.get(), dsum.get()
        for dv in (dd, dp, dsum):
            dv.free()
        # the read side's layout: all d+p rows of an item together
        full = np.full(t * R[-1] + GUARD, MARK, dtype=np.uint8)
        for i in range(n):
            w = d * stride[i]
            full[t * R[i]:t * R[i] + w] = data[d * R[i]:d * R[i] + w]
            w2 = p * stride[i]
            full[t * R[i] + w:t * R[i] + w + w2] = par[p * R[i]:p * R[i] + w2]
        b = Batch(d, p, MiB, [(ln, 7000 + i) for i, ln in enumerate(lens)],
                  one_down(n, t, shift=3))
        b.buf[:] = full
        b.dig[:n * t * 32] = sums
        for i in range(n):
            s = (i + 3) % t
            o = b.off(i, s)
            b.buf[o:o + stride[i]] = MARK            # the dropped row
            b.dig[(i * t + s) * 32:(i * t + s + 1) * 32] = MARK
            b.flip(i, (i * 5 + 7) % t if (i * 5 + 7) % t != s else (s + 1) % t,
                   (i * 977) % S[i], bit=i % 8)
        got, gdig, st = run_and_check(e, b, data_only=0, rehash=rehash)
    assert st == [0] * n
    for i in range(n):
        w = t * stride[i]
        g = got[t * R[i]:t * R[i] + w].reshape(t, stride[i])[:, :S[i]]
        f = full[t * R[i]:t * R[i] + w].reshape(t, stride[i])[:, :S[i]]
        assert (g == f).all(), i
    if rehash:
        assert (gdig[:n * t * 32] == sums).all()


# ---- 2. shard-length edges ------------------------------------------------

EDGES = (1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097,
         131072)


@pytest.mark.parametrize("data_only", [0, 1])
def test_shard_length_edges(data_only):
    """Hash tail and packet edges, the 64-byte stride edge, one tile, the
    tile boundary -1/0/+1, several tiles ending mid-tile, the full shard; a
    length of S*d - (d-1) puts Split's zero padding into the last rows."""
    d, p = 8, 4
    t = d + p
    specs = [(S * d if k % 2 == 0 or S == 1 else S * d - (d - 1), 7100 + k)
             for k, S in enumerate(EDGES)]
    n = len(specs)
    read = np.ones((n, t), dtype=np.uint8)
    for i in range(n):
        m = i % 4            # 0..3 rows unread, and one more corrupt below
        for k in range(m):
            read[i, (3 * i + 5 * k) % t] = 0
    b = Batch(d, p, MiB, specs, read)
    assert b.S == list(EDGES)
    for i in range(0, n, 2):  # bitrot at the last valid byte
        s = next(s for s in range(t) if read[i, (s + i) % t])
        b.flip(i, (s + i) % t, b.S[i] - 1, bit=i % 8)
    with minio_amd.Erasure(d, p, MiB) as e:
        _, _, st = run_and_check(e, b, data_only=data_only, rehash=1)
    assert st == [0] * n


# ---- 3. adjacent waves, different plans -----------------------------------

def test_adjacent_waves_serve_different_plans():
    """67 items of S = 512 (a quarter tile each), every one with a different
    single- or double-erasure mask, interleaved with items of S = 2049 whose
    last tile holds one live lane: the four waves of a workgroup serve four
    pairs with different entries, and no work list is a multiple of 4."""
    d, p = 8, 4
    t = d + p
    masks = [(a,) for a in range(t)] + \
        [(a, c) for a in range(t) for c in range(a + 1, t)]
    specs, read = [], []
    k = 0
    for i in range(67):
        specs.append((512 * d, 7200 + i % 6))
        row = np.ones(t, dtype=np.uint8)
        row[list(masks[(i * 7) % len(masks)])] = 0
        read.append(row)
        if i % 5 == 2:
            specs.append((2049 * d - 3, 7210 + k % 3))
            row = np.ones(t, dtype=np.uint8)
            row[(k * 5) % t] = 0
            if k % 2:
                row[(k * 5 + 4) % t] = 0
            read.append(row)
            k += 1
    read = np.stack(read)
    small = [tuple(r) for r, (ln, _) in zip(read, specs) if ln == 512 * d]
    assert len(small) == 67 and len(set(small)) == 67
    missing = (read == 0).sum(axis=1)
    assert set(missing) == {1, 2}
    assert (missing == 1).sum() % 4 != 0 and (missing == 2).sum() % 4 != 0
    b = Batch(d, p, MiB, specs, read)
    assert sorted(set(b.S)) == [512, 2049]
    with minio_amd.Erasure(d, p, MiB) as e:
        _, _, st = run_and_check(e, b, data_only=0, rehash=1)
    assert st == [0] * b.n


# ---- 4. hash lists --------------------------------------------------------

def test_hash_list_lengths_and_every_lane_of_the_compare():
    """EC2+4.  In hash order the first 16 chains (one wave) are 3 of
    S = 4097, 6 of 2048, 3 of 2047, 2 of 33 and 2 of 1: a 32-multiple between
    two ragged lengths.  The list has 19 chains.  Single corrupt bytes at
    position 0, at S-1 and in each 8-byte lane of the last packet are each
    caught, and only those rows are flagged."""
    d, p = 2, 4
    t = d + p
    S_of = [33, 1, 2048, 4097, 1, 2047]          # batch order != hash order
    n_read = [2, 3, 6, 3, 2, 3]
    read = np.zeros((len(S_of), t), dtype=np.uint8)
    for i, k in enumerate(n_read):
        read[i, [(i + 2 * j) % t if k <= 3 else j for j in range(k)]] = 1
    assert read.sum() == 19 and (read.sum(axis=1) == n_read).all()
    b = Batch(d, p, 8194, [(S * d - (S > 1), 7300 + i)
                           for i, S in enumerate(S_of)], read)
    assert b.S == S_of
    for lane in range(4):                         # the last packet of S=2048
        b.flip(2, lane + 1, 2048 - 32 + 8 * lane + lane, bit=lane)
    rows = [int(np.flatnonzero(read[i])[0]) for i in range(len(S_of))]
    b.flip(3, rows[3], 0, bit=7)                  # position 0
    b.flip(5, rows[5], 2046, bit=1)               # S-1, in the ragged tail
    b.flip(1, rows[1], 0, bit=3)                  # S = 1: both at once
    assert b.bad.sum() == 7 and (b.verified.sum(axis=1) >= d).all()
    with minio_amd.Erasure(d, p, 8194) as e:
        _, _, st = run_and_check(e, b, data_only=0, rehash=1)
    assert st == [0] * b.n


# ---- 5. nothing outside an item is written --------------------------------

def test_neighbours_and_verified_rows_keep_their_bytes():
    d, p = 8, 4
    t = d + p
    specs = [(d * 100, 7400), (d * 2049, 7401), (d * 33 - 1, 7402),
             (d * 513, 7403), (d * 64, 7404)]
    read = np.ones((5, t), dtype=np.uint8)
    read[1, [0, 11]] = 0      # rebuilt, between two complete neighbours
    read[3, [4, 5, 9]] = 0
    read[4, 10] = 0           # parity only: out of scope under data_only
    b = Batch(d, p, MiB, specs, read)
    with minio_amd.Erasure(d, p, MiB) as e:
        for data_only in (0, 1):
            got, gdig, st = run_and_check(e, b, data_only=data_only,
                                          rehash=1)
            assert st == [0] * 5
            for i in (0, 2) + ((4,) if data_only else ()):
                lo, hi = t * b.R[i], t * b.R[i + 1]
                assert (got[lo:hi] == b.buf[lo:hi]).all(), i
            for i, s in np.argwhere(read):
                o = b.off(i, s)
                assert (got[o:o + b.stride[i]] ==
                        b.buf[o:o + b.stride[i]]).all(), (i, s)
            assert (got[t * b.R[-1]:] == MARK).all()
            if data_only:     # unread parity rows keep the marker
                for i, s in ((1, 11), (3, 9), (4, 10)):
                    o = b.off(i, s)
                    assert (got[o:o + b.stride[i]] == MARK).all(), (i, s)


# ---- 6. TOO_FEW -----------------------------------------------------------

def test_too_few_between_recoverable_items():
    d, p = 8, 4
    t = d + p
    specs = [(d * 2049, 7500), (d * 700 - 5, 7501), (d * 31, 7502)]
    read = np.ones((3, t), dtype=np.uint8)
    read[0, [1, 8]] = 0
    read[1, [0, 2, 4, 6]] = 0                      # 8 read, one corrupt
    read[2, 7] = 0
    b = Batch(d, p, MiB, specs, read)
    b.flip(1, 3, 699, bit=4)
    with minio_amd.Erasure(d, p, MiB) as e:
        got, gdig, st = run_and_check(e, b, rehash=1)
        assert st == [0, TOO_FEW, 0]
        lo, hi = t * b.R[1], t * b.R[2]
        assert (got[lo:hi] == b.buf[lo:hi]).all()
        assert (gdig[t * 32:2 * t * 32] == b.dig[t * 32:2 * t * 32]).all()
        # no status array: the call fails, nothing is modified, present_out
        # is still filled
        rc, pres, _, got, gdig = call(e, b, rehash=1, status=False)
        assert rc == TOO_FEW
        assert (pres == b.verified).all()
        assert (got == b.buf).all() and (gdig == b.dig).all()


# ---- 7. more than 8 rebuilt rows ------------------------------------------

def test_more_than_eight_rebuilt_rows():
    """EC4+10 with all ten parity rows unread and data_only = 0: every item
    takes two plan entries (8 + 2 rows).  No compiled (d,p) specialization
    exists for this geometry, and none is needed."""
    d, p = 4, 10
    t = d + p
    specs = [(d * 2049 - 1, 7600), (d * 40, 7601), (d * 4096, 7602)]
    read = np.zeros((3, t), dtype=np.uint8)
    read[:, :d] = 1
    b = Batch(d, p, d * 4096, specs, read)
    with minio_amd.Erasure(d, p, d * 4096) as e:
        _, _, st = run_and_check(e, b, data_only=0, rehash=1)
    assert st == [0, 0, 0]


# ---- 8. agreement with the uniform call -----------------------------------

@pytest.mark.parametrize("data_only", [0, 1])
def test_agrees_with_the_uniform_call(data_only):
    """All items at block_size: the packed layout is the uniform one byte
    for byte, so the same images go through both calls."""
    d, p, L, n = 8, 4, 1000, 24
    t = d + p
    read = one_down(n, t)
    read[5, :5] = 0                                 # unrecoverable
    read[6, :] = 1                                  # complete
    b = Batch(d, p, d * L, [(d * L, 7700 + i % 4) for i in range(n)], read)
    for i in range(0, n, 4):
        b.flip(i, (i + 3) % t, (i * 41) % L, bit=i % 8)
    b.flip_digest(9, 2, 17, bit=5)
    with minio_amd.Erasure(d, p, d * L) as e:
        stride = lib.mec_shard_stride(d * L, d)
        assert b.R == [i * stride for i in range(n + 1)]
        rc, pres, st, got, gdig = call(e, b, data_only, 1)

        def uniform(ctx, n_, shards, sums, lens, mask, algo, do, rh, pr, sa):
            return lib.mec_verify_reconstruct_batch_dev(
                ctx, n_, shards, sums, mask, L, algo, do, rh, pr, sa)

        rc_u, pres_u, st_u, got_u, gdig_u = call(e, b, data_only, 1,
                                                 fn=uniform)
    assert rc == 0 and rc_u == 0
    assert (pres == pres_u).all() and (pres == b.verified).all()
    assert st == st_u and st[5] == TOO_FEW and st.count(TOO_FEW) == 1
    _, cmp, _, _ = b.expect(data_only, 1)
    assert not (got == b.buf).all()                 # something was rebuilt
    assert ((got == got_u) | ~cmp).all()
    assert (gdig == gdig_u).all()


# ---- 9. large n -----------------------------------------------------------

def test_large_n():
    """n = 70000 > 65535 items at EC2+1 with S cycling through 1, 33, 64,
    100, one drive down round-robin: many tiles and chains per launch.  The
    layout repeats every four items (3 rows of 64, 64, 64 and 128 bytes), so
    images and expectations are built as (n/4, 960) arrays from a small pool
    of oracle-encoded blocks."""
    d, p, n = 2, 1, 70000
    t = d + p
    cyc, strides, pool = (1, 33, 64, 100), (64, 64, 64, 128), 5
    g = n // 4
    lens = [cyc[i % 4] * d - (i % 2 if cyc[i % 4] > 1 else 0)
            for i in range(n)]
    R = minio_amd.var_row_offsets(d, 200, lens)
    assert R[4] == 320 and R[-1] == 320 * g
    idx = np.arange(n)
    down = idx % t                                   # the unread row
    buf = np.full((g, 960), MARK, dtype=np.uint8)
    want = buf.copy()
    cmp = np.ones(buf.shape, dtype=bool)
    dig = np.full((n, t, 32), MARK, dtype=np.uint8)
    wdig = dig.copy()
    col = 0
    for k, (S, stride) in enumerate(zip(cyc, strides)):
        items = idx[k::4]                            # g items of this class
        # lens alternate with the item's parity, which is k's: one length
        ln = S * d - (k % 2 if S > 1 else 0)
        assert all(lens[i] == ln for i in items[:8])
        gold = [golden(d, p, ln, 7900 + 10 * k + j) for j in range(pool)]
        rows = np.stack([r for r, _ in gold])[(items // 4) % pool]
        dg = np.stack([x for _, x in gold])[(items // 4) % pool]
        img = np.full((g, t, stride), MARK, dtype=np.uint8)
        img[:, :, :S] = rows
        full = img.copy()
        keep = np.ones((g, t, stride), dtype=bool)
        gone = down[items]
        img[np.arange(g), gone] = MARK
        keep[np.arange(g), gone, S:] = False         # scratch of rebuilt rows
        buf[:, col:col + t * stride] = img.reshape(g, -1)
        want[:, col:col + t * stride] = full.reshape(g, -1)
        cmp[:, col:col + t * stride] = keep.reshape(g, -1)
        wdig[items] = dg
        dig[items] = dg
        dig[items, gone] = MARK
        col += t * stride
    assert col == 960
    read = one_down(n, t)
    with minio_amd.Erasure(d, p, 200) as e:
        ds, dd = Dev(e, buf), Dev(e, dig)
        present = ctypes.create_string_buffer(n * t)
        st = ctypes.create_string_buffer(n)
        rc = lib.mec_verify_reconstruct_batch_var_dev(
            e._ctx, n, ds.ptr, dd.ptr, i64arr(lens), read.tobytes(), HH, 0, 1,
            present, st)
        got = ds.get().reshape(g, 960)
        gdig = dd.get().reshape(n, t, 32)
        ds.free()
        dd.free()
    assert rc == 0, (rc, lib.mec_last_error())
    assert present.raw == read.tobytes()
    assert st.raw == bytes(n)
    wrong = np.argwhere(((got != want) & cmp).any(axis=1))
    assert wrong.size == 0, f"first wrong groups of 4: {wrong[:4].ravel()}"
    wrong = np.argwhere((gdig != wdig).any(axis=2))
    assert wrong.size == 0, f"first wrong digests: {wrong[:4].tolist()}"
    # the oracle itself on the first and last group of four
    for i in list(range(4)) + list(range(n - 4, n)):
        S, stride = cyc[i % 4], strides[i % 4]
        o = t * R[i] + np.arange(t) * stride
        flat = got.ravel()
        have = [bytes(flat[x:x + S]) for x in o]
        ref = _rs(d, p).reconstruct([None if s == down[i] else have[s]
                                     for s in range(t)])
        assert have == ref, i


# ---- 10. argument checks --------------------------------------------------

def test_argument_checks():
    d, p = 4, 2
    t = d + p
    bs = d * 96
    specs = [(bs, 8000), (d * 33, 8001), (5, 8002), (bs - 1, 8003)]
    read = one_down(4, t)
    b = Batch(d, p, bs, specs, read)
    b.flip(3, 5, 50)
    with minio_amd.Erasure(d, p, bs) as e:
        def refused(**kw):
            rc, pres, st, got, gdig = call(e, b, **kw)
            assert rc == 6, kw
            assert (got == b.buf).all() and (gdig == b.dig).all(), kw
            assert (pres == 0xEE).all() and st == [0xEE] * 4, kw

        for algo in (minio_amd.SHA256, minio_amd.BLAKE2B512, 0, 5):
            refused(algo=algo)
        refused(n=0)
        refused(n=-1)
        for name in ("shards", "sums", "lens", "mask"):
            refused(null=(name,))
        for at in range(4):
            for bad in (0, -1, bs + 1):
                lens = list(b.lens)
                lens[at] = bad
                refused(lens=lens)
        # n*(d+p) past 32 bits: refused before the lengths are read
        refused(n=2**32 // t + 1)
        # both HighwayHash ids name the same function
        a1 = run_and_check(e, b, 0, 1, algo=minio_amd.HIGHWAYHASH256S)
        a2 = run_and_check(e, b, 0, 1, algo=minio_amd.HIGHWAYHASH256)
    assert (a1[0] == a2[0]).all() and (a1[1] == a2[1]).all()
    assert a1[2] == a2[2] == [0] * 4


# ---- 11. host-pointer variant and Python ----------------------------------

@pytest.mark.parametrize("data_only,rehash", [(False, False), (False, True),
                                              (True, False), (True, True)])
def test_python_verify_reconstruct_batch_var(data_only, rehash):
    d, p = 8, 4
    t = d + p
    S_of = [1000, 1, 2049, 64, 131072, 77, 512]
    gold = [golden(d, p, S * d - (i % 3 if S > 1 else 0), 8100 + i)
            for i, S in enumerate(S_of)]
    n = len(S_of)
    items = [[bytes(r) for r in rows] for rows, _ in gold]
    digs = [[bytes(x) for x in dg] for _, dg in gold]

    def rot(bs_, at, mask):
        return bs_[:at] + bytes([bs_[at] ^ mask]) + bs_[at + 1:]

    items[0][2] = None                          # not read
    digs[0][2] = None
    items[1][5] = rot(items[1][5], 0, 0x10)     # bitrot in a data row, S = 1
    items[2][10] = rot(items[2][10], 2048, 1)   # parity, the last byte
    items[3] = [None] * t                       # nothing read at all
    digs[3] = [None] * t
    for s in (0, 3, 6, 9):                      # item 4: 7 rows verify
        items[4][s] = None
    items[4][11] = rot(items[4][11], 131071, 0x80)
    digs[5][1] = rot(digs[5][1], 0, 2)          # bad digest
    for s in (4, 8):
        items[6][s] = None                      # two rows not read
    with minio_amd.Erasure(d, p, MiB) as e:
        out, sums_out, st, corrupt = e.verify_reconstruct_batch_var(
            items, digs, data_only=data_only, rehash=rehash)
    assert st == [0, 0, 0, TOO_FEW, TOO_FEW, 0, 0]
    assert corrupt == [[], [5], [10], [], [11], [1], []]
    assert out[3] == items[3] and out[4] == items[4]
    assert (sums_out is None) == (not rehash)
    for i in (0, 1, 2, 5, 6):
        rows, dg = gold[i]
        gone = [s for s in range(t) if items[i][s] is None or s in corrupt[i]]
        ref = _rs(d, p).reconstruct([None if s in gone else items[i][s]
                                     for s in range(t)], data_only=data_only)
        for s in range(t):
            if s in gone and (s < d or not data_only):
                assert out[i][s] == ref[s] == bytes(rows[s]), (i, s)
                if rehash:
                    assert sums_out[i][s] == bytes(dg[s]), (i, s)
            else:
                assert out[i][s] == items[i][s], (i, s)
                if rehash:
                    assert sums_out[i][s] == digs[i][s], (i, s)
    if rehash:
        assert sums_out[3] == digs[3] and sums_out[4] == digs[4]
