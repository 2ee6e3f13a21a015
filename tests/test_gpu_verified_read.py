"""GPU tests of mec_verify_reconstruct_batch*: bitrot check on the device
feeding the mixed-pattern reconstruct (streamingBitrotReader.ReadAt +
parallelReader.Read + Decode/Heal for a batch across objects).  Rows and
digests come from the CPU oracle (oracle.RS, oracle.bitrot_sum), bit-exact.
Rows that were not read, their digest slots, and every row's bytes in
[shard_len, stride) are prefilled with a marker that must never influence a
result."""
import ctypes
import functools
import random
import time

import numpy as np
import pytest

import minio_amd
import oracle

pytestmark = pytest.mark.gpu

lib = minio_amd._lib
HH = minio_amd.HIGHWAYHASH256S
TOO_FEW = 3
MARK = 0xA5


def check(st):
    assert st == 0, (st, lib.mec_last_error())


def cptr(a):
    return a.ctypes.data_as(ctypes.c_char_p)


class Dev:
    """A host numpy array's twin on the device."""

    def __init__(self, e, host):
        self.e = e
        self.shape = host.shape
        self.nbytes = host.nbytes
        self.ptr = ctypes.c_void_p()
        check(lib.mec_dev_alloc(e._ctx, host.nbytes, ctypes.byref(self.ptr)))
        self.put(host)

    def put(self, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes == self.nbytes
        check(lib.mec_memcpy_h2d(self.e._ctx, self.ptr, cptr(host),
                                 host.nbytes))

    def get(self):
        out = np.empty(self.shape, dtype=np.uint8)
        check(lib.mec_memcpy_d2h(self.e._ctx, cptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        lib.mec_dev_free(self.e._ctx, self.ptr)


@functools.lru_cache(maxsize=None)
def golden(d, p, bs, n, seed):
    """n seeded blocks encoded and hashed by the oracle: rows (n, d+p, S)
    and digests (n, d+p, 32), read-only, shared by the tests that ask for
    the same arguments."""
    rs = oracle.RS(d, p)
    S = oracle.ceil_frac(bs, d)
    rows = np.empty((n, d + p, S), dtype=np.uint8)
    sums = np.empty((n, d + p, 32), dtype=np.uint8)
    for i in range(n):
        for s, sh in enumerate(rs.encode_data(oracle.fill_random(bs, seed + i))):
            rows[i, s] = np.frombuffer(sh, dtype=np.uint8)
            sums[i, s] = np.frombuffer(oracle.bitrot_sum(HH, sh),
                                       dtype=np.uint8)
    rows.setflags(write=False)
    sums.setflags(write=False)
    return rows, sums


def make_input(rows, sums, stride, read):
    """Device-layout input: rows and digests where read, MARK elsewhere and
    in every row's [S, stride)."""
    n, total, S = rows.shape
    buf = np.full((n, total, stride), MARK, dtype=np.uint8)
    buf[:, :, :S] = rows
    dig = sums.copy()
    buf[read == 0] = MARK
    dig[read == 0] = MARK
    return buf, dig


def run(e, dshards, dsums, read, L, data_only=0, rehash=0, algo=HH,
        status=True, fn=None):
    n = read.shape[0]
    present = ctypes.create_string_buffer(read.size)
    st = ctypes.create_string_buffer(n) if status else None
    fn = fn or lib.mec_verify_reconstruct_batch_dev
    rc = fn(e._ctx, n, dshards.ptr, dsums.ptr, read.tobytes(), L, algo,
            data_only, rehash, present, st)
    pres = np.frombuffer(present.raw, dtype=np.uint8).reshape(read.shape)
    return rc, pres, (list(st.raw) if status else None)


def expect(rs, inp, dig, verified, d, L, data_only, rehash):
    """What the call must leave, from oracle.RS.reconstruct on the verified
    mask.  Returns (rows, compare_mask, digests, statuses)."""
    n, total, stride = inp.shape
    want, wdig = inp.copy(), dig.copy()
    cmp = np.ones(inp.shape, dtype=bool)
    scope = d if data_only else total
    st = []
    for i in range(n):
        v = verified[i]
        if v.sum() < d:
            st.append(TOO_FEW)
            continue
        st.append(0)
        if v[:scope].all():
            continue
        ref = rs.reconstruct([bytes(inp[i, s, :L]) if v[s] else None
                              for s in range(total)],
                             data_only=bool(data_only))
        for s in range(scope):
            if not v[s]:
                want[i, s, :L] = np.frombuffer(ref[s], dtype=np.uint8)
                cmp[i, s, L:] = False  # scratch up to the stride
                if rehash:
                    wdig[i, s] = np.frombuffer(oracle.bitrot_sum(HH, ref[s]),
                                               dtype=np.uint8)
    return want, cmp, wdig, st


def run_and_check(e, rs, inp, dig, read, bad, L, data_only=0, rehash=0,
                  algo=HH):
    """One call on (inp, dig); bad marks the rows the test corrupted.
    Checks present_out, statuses, every byte and every digest slot."""
    d = e.d
    verified = (read != 0) & ~bad
    ds, dd = Dev(e, inp), Dev(e, dig)
    rc, pres, st = run(e, ds, dd, read, L, data_only, rehash, algo)
    got, gdig = ds.get(), dd.get()
    ds.free()
    dd.free()
    assert rc == 0
    assert (pres == verified).all(), np.argwhere(pres != verified)[:4]
    want, cmp, wdig, wst = expect(rs, inp, dig, verified, d, L, data_only,
                                  rehash)
    assert st == wst
    wrong = np.argwhere(((got != want) & cmp).any(axis=2))
    assert wrong.size == 0, f"first wrong (item,row): {wrong[:4].tolist()}"
    wrong = np.argwhere((gdig != wdig).any(axis=2))
    assert wrong.size == 0, f"first wrong digests: {wrong[:4].tolist()}"
    return got, gdig, st


def flip(buf, i, s, byte, bit=0):
    buf[i, s, byte] ^= np.uint8(1 << bit)


# ---- 1. clean batch -------------------------------------------------------

@pytest.mark.parametrize("data_only", [0, 1])
def test_clean_batch(data_only):
    d, p, L, n = 4, 2, 96, 8
    rows, sums = golden(d, p, d * L, n, 100)
    read = np.ones((n, d + p), dtype=np.uint8)
    with minio_amd.Erasure(d, p, d * L) as e:
        stride = lib.mec_shard_stride(d * L, d)
        assert e.shard_size() == L and stride == 128
        inp, dig = make_input(rows, sums, stride, read)
        got, gdig, st = run_and_check(e, oracle.RS(d, p), inp, dig, read,
                                      np.zeros(read.shape, bool), L,
                                      data_only)
    assert st == [0] * n
    assert (got == inp).all() and (gdig == dig).all()


# ---- 2. every lane takes part in the compare ------------------------------

def test_every_lane_takes_part_in_the_compare():
    d, p, L, n = 4, 2, 96, 10
    total = d + p
    rows, sums = golden(d, p, d * L, n, 200)
    read = np.ones((n, total), dtype=np.uint8)
    bad = np.zeros((n, total), dtype=bool)
    with minio_amd.Erasure(d, p, d * L) as e:
        stride = lib.mec_shard_stride(d * L, d)
        inp, dig = make_input(rows, sums, stride, read)
        # items 0-4: one bit of a row, at the first byte of each lane's
        # word of packet 0 and at the last byte of the row
        for i, off in enumerate((0, 8, 16, 24, L - 1)):
            s = (2 * i + 1) % total
            flip(inp, i, s, off, bit=i)
            bad[i, s] = True
        # items 5-8: one bit in each 8-byte word of a digest
        for w in range(4):
            i, s = 5 + w, (w + 3) % total
            flip(dig, i, s, 8 * w + (w * 3) % 8, bit=7 - w)
            bad[i, s] = True
        # item 9 stays untouched
        got, _, st = run_and_check(e, oracle.RS(d, p), inp, dig, read, bad,
                                   L)
    assert st == [0] * n
    assert bad.sum(axis=1).tolist() == [1] * 9 + [0]
    # corrupt rows were rebuilt to the oracle's bytes; a corrupt digest
    # leaves the (good) bytes of its row equal to what reconstruct gives
    assert (got[:, :, :L] == rows).all()


# ---- 3. list index differs from chain id ----------------------------------

@pytest.mark.parametrize("extra", [0, 1])
def test_read_mask_with_holes(extra):
    d, p, L, n = 8, 4, 100, 30
    total = d + p
    rows, sums = golden(d, p, d * L, n, 300)
    rng = random.Random(303)
    read = np.zeros((n, total), dtype=np.uint8)
    bad = np.zeros((n, total), dtype=bool)
    for i in range(n):
        chosen = rng.sample(range(total), d + extra)
        read[i, chosen] = 1 + (i % 200)       # any nonzero byte means read
        if i % 3 == 0:
            bad[i, chosen[i % d]] = True
    assert len({tuple(r != 0) for r in read}) > n // 2
    with minio_amd.Erasure(d, p, d * L) as e:
        stride = lib.mec_shard_stride(d * L, d)
        assert stride == 128
        inp, dig = make_input(rows, sums, stride, read)
        for i, s in np.argwhere(bad):
            flip(inp, i, s, (7 * i + s) % L, bit=i % 8)
        got, _, st = run_and_check(e, oracle.RS(d, p), inp, dig, read, bad,
                                   L)
    if extra == 0:
        assert st == [TOO_FEW if i % 3 == 0 else 0 for i in range(n)]
        for i in range(0, n, 3):
            assert (got[i] == inp[i]).all()
    else:
        assert st == [0] * n
        assert (got[:, :, :L] == rows).all()


# ---- 4. lengths that cross every loop edge --------------------------------

LENGTHS = (1, 3, 4, 17, 31, 32, 33, 511, 512, 513, 543, 1024, 1055, 1536,
           2065, 87382,
           # each side of the prefetch loop's edges (blocks of 512 bytes)
           1023, 1025, 1535, 1537, 2047, 2048, 2049)
GEOMETRIES = ((2, 1), (4, 2), (8, 4), (12, 4), (16, 4), (8, 8))


@pytest.mark.parametrize(
    "L,d,p", [(L, *GEOMETRIES[k % len(GEOMETRIES)])
              for k, L in enumerate(LENGTHS)])
def test_lengths_cross_every_loop_edge(L, d, p):
    n, total = 2, d + p
    bs = 1 << 20 if L == 87382 else d * L
    rows, sums = golden(d, p, bs, n, 400 + L)
    read = np.ones((n, total), dtype=np.uint8)
    bad = np.zeros((n, total), dtype=bool)
    with minio_amd.Erasure(d, p, bs) as e:
        assert e.shard_size() == L, "EC12+4's real shard size at 1 MiB"
        stride = lib.mec_shard_stride(bs, d)
        inp, dig = make_input(rows, sums, stride, read)
        s = L % total
        flip(inp, 0, s, L - 1, bit=L % 8)   # the last valid byte of one row
        bad[0, s] = True
        got, _, st = run_and_check(e, oracle.RS(d, p), inp, dig, read, bad,
                                   L)
    assert st == [0, 0]
    assert (got[:, :, :L] == rows).all()
    assert (got[1] == inp[1]).all()


@pytest.mark.parametrize("L", range(512, 544))
def test_every_tail_residue_after_a_prefetch_block(L):
    """512 bytes are one full prefetch block, so L covers every mod-32 tail
    after it.  One row has its last valid byte flipped: verify mode accepts
    the good rows and rejects that one, and with rehash sum mode writes the
    rebuilt row's digest."""
    d, p, n = 4, 2, 2
    total = d + p
    rows, sums = golden(d, p, d * L, n, 450 + L)
    read = np.ones((n, total), dtype=np.uint8)
    bad = np.zeros((n, total), dtype=bool)
    with minio_amd.Erasure(d, p, d * L) as e:
        assert e.shard_size() == L
        stride = lib.mec_shard_stride(d * L, d)
        inp, dig = make_input(rows, sums, stride, read)
        s = L % total
        flip(inp, 0, s, L - 1, bit=L % 8)   # the last valid byte of one row
        bad[0, s] = True
        got, gdig, st = run_and_check(e, oracle.RS(d, p), inp, dig, read, bad,
                                      L, rehash=1)
    assert st == [0, 0]
    assert (got[:, :, :L] == rows).all()
    assert (gdig == sums).all()


# ---- 5. partial waves -----------------------------------------------------

def test_partial_waves():
    """16 chains fill a wave: list lengths around one and four waves, the
    last listed row corrupt."""
    d, p, L, n = 2, 1, 64, 40
    total = d + p
    rows, sums = golden(d, p, d * L, n, 500)
    rs = oracle.RS(d, p)
    rng = random.Random(505)
    with minio_amd.Erasure(d, p, d * L) as e:
        stride = lib.mec_shard_stride(d * L, d)
        for count in (1, 15, 16, 17, 63, 64, 65):
            chains = sorted(rng.sample(range(n * total), count))
            read = np.zeros(n * total, dtype=np.uint8)
            read[chains] = 1
            read = read.reshape(n, total)
            bad = np.zeros(n * total, dtype=bool)
            bad[chains[-1]] = True
            bad = bad.reshape(n, total)
            inp, dig = make_input(rows, sums, stride, read)
            i, s = divmod(chains[-1], total)
            flip(inp, i, s, count % L, bit=count % 8)
            run_and_check(e, rs, inp, dig, read, bad, L)


# ---- 6. more chains than a grid dimension ---------------------------------

def test_more_chains_than_a_grid_dimension():
    d, p, L, n = 2, 1, 64, 70000
    total = d + p
    rows16, sums16 = golden(d, p, d * L, 16, 600)
    rs = oracle.RS(d, p)
    idx = np.arange(n)
    rows, sums = rows16[idx % 16], sums16[idx % 16]
    read = np.ones((n, total), dtype=np.uint8)
    holes = idx[idx % 7 == 6]
    read[holes, holes % total] = 0              # one row not read
    bad = np.zeros((n, total), dtype=bool)
    hit = idx[idx % 1000 == 0]
    bad[hit, (hit // 1000 + 2) % total] = True  # one corrupt row per 1000
    assert not (bad & (read == 0)).any()
    verified = (read != 0) & ~bad
    too_few = verified.sum(axis=1) < d
    assert too_few[1000] and too_few.sum() >= 1 and not too_few[0]
    with minio_amd.Erasure(d, p, d * L) as e:
        assert lib.mec_shard_stride(d * L, d) == L
        inp, dig = make_input(rows, sums, L, read)
        for i, s in np.argwhere(bad):
            flip(inp, i, s, (i // 1000) % L, bit=i % 8)
        ds, dd = Dev(e, inp), Dev(e, dig)
        rc, pres, st = run(e, ds, dd, read, L)
        got, gdig = ds.get(), dd.get()
        ds.free()
        dd.free()
    assert rc == 0
    assert (pres == verified).all()
    assert (np.array(st) == np.where(too_few, TOO_FEW, 0)).all()
    assert (gdig == dig).all()
    # every item at once: a recoverable item ends up complete, the others
    # keep their bytes
    want = np.where(too_few[:, None, None], inp, rows)
    wrong = np.argwhere((got != want).any(axis=(1, 2)))
    assert wrong.size == 0, f"first wrong items: {wrong[:4].ravel().tolist()}"
    # the oracle itself at the first, the last and 50 seeded items
    rebuilt_items = idx[~too_few & ~verified.all(axis=1)]
    assert rebuilt_items[0] == 0 and rebuilt_items[-1] == n - 1
    picks = [0, n - 1] + random.Random(606).sample(list(rebuilt_items), 50)
    for i in picks:
        ref = rs.reconstruct([bytes(inp[i, s]) if verified[i, s] else None
                              for s in range(total)])
        for s in range(total):
            assert bytes(got[i, s]) == ref[s], (i, s)


# ---- 7. agrees with the existing pieces -----------------------------------

def composition(e, n, total, S, stride, dshards_ptr, dscratch_ptr, want_dig,
                read, data_only, status):
    """What a caller does without the new call: hash every row on the
    device, fetch the digests, compare on the host, build the mask, call
    the mixed reconstruct."""
    ctx = e._ctx
    got = np.empty((n, total, 32), dtype=np.uint8)
    check(lib.mec_bitrot_sum_batch_dev(ctx, HH, n * total, dshards_ptr, S,
                                       stride, dscratch_ptr))
    check(lib.mec_memcpy_d2h(ctx, cptr(got), dscratch_ptr, got.nbytes))
    present = ((read != 0) & (got == want_dig).all(axis=2)).astype(np.uint8)
    rc = lib.mec_reconstruct_batch_mixed_dev(ctx, n, dshards_ptr,
                                             present.tobytes(), S, data_only,
                                             status)
    return rc, present


@pytest.mark.parametrize("data_only", [0, 1])
def test_agrees_with_existing_pieces(data_only):
    d, p, bs, n = 8, 4, 1 << 20, 64
    total = d + p
    rows4, sums4 = golden(d, p, bs, 4, 700)
    idx = np.arange(n)
    rows, sums = rows4[idx % 4], sums4[idx % 4]
    read = np.ones((n, total), dtype=np.uint8)
    read[idx, idx % total] = 0                  # one drive down, rotated
    read[9, :5] = 0                             # item 9: unrecoverable
    with minio_amd.Erasure(d, p, bs) as e:
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        inp, dig = make_input(rows, sums, stride, read)
        for i in range(0, n, 5):                # bitrot in every fifth item
            s = (i + 3) % total
            flip(inp, i, s, (i * 4099) % S, bit=i % 8)
        flip(inp, 9, 7, S - 1)
        a, b, dd = Dev(e, inp), Dev(e, inp), Dev(e, dig)
        scratch = Dev(e, np.zeros((n, total, 32), dtype=np.uint8))
        st_a = ctypes.create_string_buffer(n)
        rc_a, pres_a = composition(e, n, total, S, stride, a.ptr, scratch.ptr,
                                   dig, read, data_only, st_a)
        check(lib.mec_stream_sync(e._ctx))
        rc_b, pres_b, st_b = run(e, b, dd, read, S, data_only)
        ga, gb, gd = a.get(), b.get(), dd.get()
        for dv in (a, b, dd, scratch):
            dv.free()
    assert rc_a == 0 and rc_b == 0
    assert (pres_a == pres_b).all()
    assert pres_b[0, 3] == 0 and read[0, 3] != 0   # a bitrot hit
    assert list(st_a.raw) == st_b and st_b[9] == TOO_FEW
    assert st_b.count(TOO_FEW) == 1
    assert not (gb == inp).all()                   # something was rebuilt
    assert (ga == gb).all()
    assert (gd == dig).all()


# ---- 8. rehash ------------------------------------------------------------

@pytest.mark.parametrize("rehash", [0, 1])
def test_rehash(rehash):
    d, p, L, n = 4, 2, 100, 8
    total = d + p
    rows, sums = golden(d, p, d * L, n, 800)
    read = np.ones((n, total), dtype=np.uint8)
    bad = np.zeros((n, total), dtype=bool)
    for i in range(n):
        read[i, i % total] = 0                  # one row not read
        bad[i, (i + 2) % total] = True          # one row corrupt
    bad[5, (5 + 3) % total] = True              # item 5: a third row lost
    with minio_amd.Erasure(d, p, d * L) as e:
        stride = lib.mec_shard_stride(d * L, d)
        inp, dig = make_input(rows, sums, stride, read)
        for i, s in np.argwhere(bad):
            flip(inp, i, s, (13 * i + s) % L, bit=s)
        got, gdig, st = run_and_check(e, oracle.RS(d, p), inp, dig, read,
                                      bad, L, data_only=0, rehash=rehash)
    assert st == [TOO_FEW if i == 5 else 0 for i in range(n)]
    assert (got[5] == inp[5]).all() and (gdig[5] == dig[5]).all()
    verified = (read != 0) & ~bad
    assert (gdig[verified] == dig[verified]).all()
    if rehash:
        # every row of a recoverable item now carries its own digest
        for i in range(n):
            if i == 5:
                continue
            for s in range(total):
                assert bytes(gdig[i, s]) == oracle.bitrot_sum(
                    HH, bytes(got[i, s, :L])), (i, s)
        assert (np.delete(gdig, 5, axis=0) == np.delete(sums, 5, axis=0)).all()
    else:
        assert (gdig == dig).all()


# ---- 9. argument checks ---------------------------------------------------

def test_argument_checks():
    d, p, L, n = 4, 2, 96, 4
    total = d + p
    rows, sums = golden(d, p, d * L, n, 900)
    read = np.ones((n, total), dtype=np.uint8)
    read[1, 0] = 0
    read[2, :3] = 0                             # item 2: unrecoverable
    bad = np.zeros((n, total), dtype=bool)
    bad[3, 4] = True
    rs = oracle.RS(d, p)
    with minio_amd.Erasure(d, p, d * L) as e:
        stride = lib.mec_shard_stride(d * L, d)
        inp, dig = make_input(rows, sums, stride, read)
        flip(inp, 3, 4, 50)
        ds, dd = Dev(e, inp), Dev(e, dig)
        for algo in (minio_amd.SHA256, minio_amd.BLAKE2B512, 0, 5):
            rc, _, _ = run(e, ds, dd, read, L, algo=algo)
            assert rc == 6, algo
        assert (ds.get() == inp).all()
        # shard_len past the stride, n = 0
        assert run(e, ds, dd, read, stride + 1)[0] == 6
        assert lib.mec_verify_reconstruct_batch_dev(
            e._ctx, 0, ds.ptr, dd.ptr, read.tobytes(), L, HH, 0, 0, None,
            None) == 6
        # no status array and an unrecoverable item: the call fails,
        # nothing is modified, present_out is still filled
        rc, pres, _ = run(e, ds, dd, read, L, status=False)
        assert rc == TOO_FEW
        assert (pres == ((read != 0) & ~bad)).all()
        assert (ds.get() == inp).all() and (dd.get() == dig).all()
        ds.free()
        dd.free()
        # both HighwayHash ids name the same function
        a = run_and_check(e, rs, inp, dig, read, bad, L, 0, 1,
                          algo=minio_amd.HIGHWAYHASH256S)
        b = run_and_check(e, rs, inp, dig, read, bad, L, 0, 1,
                          algo=minio_amd.HIGHWAYHASH256)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]
    assert a[2] == [0, 0, TOO_FEW, 0]


# ---- 10. host-pointer variant and Python ----------------------------------

@pytest.mark.parametrize("data_only,rehash", [(False, False), (False, True),
                                              (True, True)])
def test_python_verify_reconstruct_batch(data_only, rehash):
    d, p, L, n = 8, 4, 1000, 6
    total = d + p
    rows, sums = golden(d, p, d * L, n, 1000)
    rs = oracle.RS(d, p)
    items = [[bytes(rows[i, s]) for s in range(total)] for i in range(n)]
    digs = [[bytes(sums[i, s]) for s in range(total)] for i in range(n)]
    items[0][2] = None                          # not read
    digs[0][2] = None
    items[1][5] = items[1][5][:77] + bytes([items[1][5][77] ^ 0x10]) + \
        items[1][5][78:]                        # bitrot in a data row
    items[2][10] = bytes([items[2][10][0] ^ 1]) + items[2][10][1:]  # parity
    for s in (0, 3, 6, 9):                      # item 3: 7 rows verify
        items[3][s] = None
    items[3][11] = items[3][11][:-1] + bytes([items[3][11][-1] ^ 0x80])
    digs[4][1] = bytes([digs[4][1][0] ^ 2]) + digs[4][1][1:]  # bad digest
    for s in (4, 8):
        items[5][s] = None                      # two rows not read
    with minio_amd.Erasure(d, p, d * L) as e:
        out, sums_out, st, corrupt = e.verify_reconstruct_batch(
            items, digs, data_only=data_only, rehash=rehash)
    assert st == [0, 0, 0, TOO_FEW, 0, 0]
    assert corrupt == [[], [5], [10], [11], [1], []]
    assert out[3] == items[3]
    assert (sums_out is None) == (not rehash)
    for i in (0, 1, 2, 4, 5):
        gone = [s for s in range(total) if items[i][s] is None or
                s in corrupt[i]]
        ref = rs.reconstruct([None if s in gone else items[i][s]
                              for s in range(total)], data_only=data_only)
        for s in range(total):
            if s in gone and (s < d or not data_only):
                assert out[i][s] == ref[s] == bytes(rows[i, s]), (i, s)
                if rehash:
                    assert sums_out[i][s] == bytes(sums[i, s]), (i, s)
            else:
                assert out[i][s] == items[i][s], (i, s)
                if rehash:
                    assert sums_out[i][s] == digs[i][s], (i, s)
    if rehash:
        assert sums_out[3] == digs[3]


# ---- 11. canary -----------------------------------------------------------

def test_new_call_keeps_up_with_the_composition():
    """Healthy batch, all rows read, through the new call and through the
    composition of test 7, alternating: the new call may take at most 2x
    the composition, the project's existing 'about 2x, only trips when the
    path stops doing the work' margin."""
    d, p, bs, n = 8, 4, 1 << 20, 256
    total = d + p
    with minio_amd.Erasure(d, p, bs) as e:
        ctx = e._ctx
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        dev, dsum, dscr = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(lib.mec_dev_alloc(ctx, n * total * stride, ctypes.byref(dev)))
        check(lib.mec_dev_alloc(ctx, n * total * 32, ctypes.byref(dsum)))
        check(lib.mec_dev_alloc(ctx, n * total * 32, ctypes.byref(dscr)))
        check(lib.mec_memset_dev(ctx, dev, 7, n * total * stride))
        one = np.frombuffer(oracle.bitrot_sum(HH, bytes([7]) * S),
                            dtype=np.uint8)
        dig = np.ascontiguousarray(np.broadcast_to(one, (n, total, 32)))
        check(lib.mec_memcpy_h2d(ctx, dsum, cptr(dig), dig.nbytes))
        read = np.ones((n, total), dtype=np.uint8)
        read_b = read.tobytes()
        present = ctypes.create_string_buffer(n * total)

        def old():
            rc, pres = composition(e, n, total, S, stride, dev, dscr, dig,
                                   read, 1, None)
            assert rc == 0 and pres.all()

        def new():
            check(lib.mec_verify_reconstruct_batch_dev(
                ctx, n, dev, dsum, read_b, S, HH, 1, 0, present, None))

        for _ in range(2):
            old()
            new()
        assert present.raw == b"\x01" * (n * total)
        t_o = t_n = 0.0
        for _ in range(5):
            t0 = time.perf_counter()
            old()
            t1 = time.perf_counter()
            new()
            t2 = time.perf_counter()
            t_o += t1 - t0
            t_n += t2 - t1
        for ptr in (dev, dsum, dscr):
            lib.mec_dev_free(ctx, ptr)
    print(f"composition {t_o / 5 * 1e3:.3f} ms, verified read "
          f"{t_n / 5 * 1e3:.3f} ms, ratio {t_n / t_o:.2f}")
    assert t_n <= 2 * t_o, f"verified read {t_n / 5 * 1e3:.3f} ms vs " \
                           f"composition {t_o / 5 * 1e3:.3f} ms"
