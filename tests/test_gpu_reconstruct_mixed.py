"""GPU tests of mec_reconstruct_batch_mixed*: batch reconstruct with one
erasure pattern PER ITEM (what a degraded read or heal batched across
objects produces: every object rotates its shards by hashOrder,
cmd/erasure-metadata-utils.go:178).  Every result is compared bit-exactly
with the CPU oracle (or with the uniform call where the test says so)."""
import ctypes
import functools
import itertools
import random
import time

import numpy as np
import pytest

import minio_amd
import oracle

pytestmark = pytest.mark.gpu

lib = minio_amd._lib
TOO_FEW = 3
HOLE = 0xA5  # prefill of missing rows: a rebuilt row can never pass by luck


def check(st):
    assert st == 0, (st, lib.mec_last_error())


def cptr(a):
    return a.ctypes.data_as(ctypes.c_char_p)


class Dev:
    """n x (d+p) x stride shard buffer on the device, numpy on the host."""

    def __init__(self, e, host):
        self.e = e
        self.shape = host.shape
        self.ptr = ctypes.c_void_p()
        check(lib.mec_dev_alloc(e._ctx, host.nbytes, ctypes.byref(self.ptr)))
        self.put(host)

    def put(self, host):
        host = np.ascontiguousarray(host)
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
    """n seeded blocks encoded by the oracle: (n, d+p, S) uint8, read-only,
    shared by every test that asks for the same arguments."""
    rs = oracle.RS(d, p)
    S = oracle.ceil_frac(bs, d)
    out = np.empty((n, d + p, S), dtype=np.uint8)
    for i in range(n):
        shards = rs.encode_data(oracle.fill_random(bs, seed + i))
        for s, sh in enumerate(shards):
            out[i, s] = np.frombuffer(sh, dtype=np.uint8)
    out.setflags(write=False)
    return out


def masks_with_erasures(total, ks):
    out = []
    for k in ks:
        for gone in itertools.combinations(range(total), k):
            m = [1] * total
            for g in gone:
                m[g] = 0
            out.append(tuple(m))
    return out


def damaged(gold, masks, stride):
    """Device-layout input: gold rows at `stride`, missing rows = HOLE."""
    n, total, S = gold.shape
    buf = np.zeros((n, total, stride), dtype=np.uint8)
    buf[:, :, :S] = gold
    pres = np.array(masks, dtype=np.uint8)
    buf[pres == 0] = HOLE
    return buf, pres


def expected(inp, gold, pres, d, data_only, shard_len=None):
    """What the call must leave: inp with the rebuilt rows' first shard_len
    bytes taken from gold.  Returns (want, compare_mask)."""
    n, total, stride = inp.shape
    L = gold.shape[2] if shard_len is None else shard_len
    want = inp.copy()
    cmp = np.ones(inp.shape, dtype=bool)
    rebuilt = pres == 0
    if data_only:
        rebuilt = rebuilt.copy()
        rebuilt[:, d:] = False
    want[rebuilt, :L] = gold[rebuilt][:, :L]
    # a rebuilt row's bytes past shard_len are scratch up to the stride
    tail = np.zeros(inp.shape, dtype=bool)
    tail[rebuilt, L:] = True
    cmp &= ~tail
    return want, cmp


def run_mixed(e, dev, pres, shard_len, data_only, fn=None, status=True):
    n = pres.shape[0]
    st = ctypes.create_string_buffer(n) if status else None
    fn = fn or lib.mec_reconstruct_batch_mixed_dev
    rc = fn(e._ctx, n, dev.ptr, pres.tobytes(), shard_len,
            1 if data_only else 0, st)
    return rc, (list(st.raw) if status else None)


# ---- 1. all patterns in one call ------------------------------------------

@pytest.mark.parametrize("data_only", [0, 1])
def test_all_patterns_one_call(data_only):
    d, p, bs = 8, 4, 8 << 10
    total = d + p
    masks = masks_with_erasures(total, (1, 2, 3, 4))
    assert len(masks) == 793
    masks.append((1,) * total)
    random.Random(794).shuffle(masks)
    n = len(masks)
    gold = golden(d, p, bs, n, 1000)
    with minio_amd.Erasure(d, p, bs) as e:
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        assert S == 1024
        inp, pres = damaged(gold, masks, stride)
        dev = Dev(e, inp)
        rc, st = run_mixed(e, dev, pres, S, data_only)
        got = dev.get()
        dev.free()
    assert rc == 0 and st == [0] * n
    want, cmp = expected(inp, gold, pres, d, data_only)
    assert cmp.all()  # S == stride here: every byte is compared
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, f"first wrong (item,row): {bad[:4].tolist()}"
    if not data_only:
        assert (got == gold).all()


# ---- 2. geometries and ragged lengths -------------------------------------

def random_masks(d, p, n, seed):
    rng = random.Random(seed)
    total = d + p
    out = []
    for i in range(n):
        if i == 0:
            gone = rng.sample(range(total), p)      # the most a call can lose
        elif i == 1:
            gone = list(range(min(d, p)))           # leading data rows
        elif i == 2:
            gone = []                               # complete item
        else:
            gone = rng.sample(range(total), rng.randint(1, p))
        out.append(tuple(0 if s in gone else 1 for s in range(total)))
    return out


def oracle_rows(rs, rows, mask, L, data_only):
    """oracle.RS.reconstruct on one item's first L bytes."""
    shards = [bytes(rows[s, :L]) if mask[s] else None
              for s in range(len(mask))]
    return rs.reconstruct(shards, data_only=bool(data_only))


@pytest.mark.parametrize("d,p", [(2, 1), (4, 2), (6, 6), (8, 8), (12, 4),
                                 (17, 5)])
def test_geometries_and_ragged_lengths(d, p):
    bs, n = 64 << 10, 64
    total = d + p
    gold = golden(d, p, bs, n, 2000 + d)
    masks = random_masks(d, p, n, 31 * d + p)
    rs = oracle.RS(d, p)
    with minio_amd.Erasure(d, p, bs) as e:
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        if (d, p) == (12, 4):
            assert S == 5462 and S % 32 != 0
        inp, pres = damaged(gold, masks, stride)
        dev = Dev(e, inp)
        for L in (1, 31, 32, 33, S):
            for data_only in (0, 1):
                dev.put(inp)
                rc, st = run_mixed(e, dev, pres, L, data_only)
                assert rc == 0 and st == [0] * n
                got = dev.get()
                want, cmp = expected(inp, gold, pres, d, data_only, L)
                assert (got[cmp] == want[cmp]).all(), (L, data_only)
                # the oracle itself, item by item, on the bytes the call saw
                for i in (0, 1, 2, 3, n - 1) if L != S else range(n):
                    ref = oracle_rows(rs, inp[i], masks[i], L, data_only)
                    for s in range(total):
                        if ref[s] is not None:
                            assert bytes(got[i, s, :L]) == ref[s], \
                                (L, data_only, i, s)
        dev.free()


def test_more_than_eight_rows_is_chunked():
    """(9,9) with all 9 data rows erased rebuilds 9 rows: two plan entries
    (8 rows + 1 row) over the same sources, in two launches.
    mec_ctx_create accepts the geometry (d <= 32, d+p <= 40)."""
    d, p, bs, n = 9, 9, 64 << 10, 6
    total = d + p
    gold = golden(d, p, bs, n, 2900)
    nine = tuple([0] * 9 + [1] * 9)
    masks = [nine, (1,) * total, nine,
             tuple([1] * 9 + [0] * 9), nine,
             tuple(0 if s % 2 else 1 for s in range(total))]
    with minio_amd.Erasure(d, p, bs) as e:
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        inp, pres = damaged(gold, masks, stride)
        dev = Dev(e, inp)
        for data_only in (0, 1):
            dev.put(inp)
            rc, st = run_mixed(e, dev, pres, S, data_only)
            assert rc == 0 and st == [0] * n
            got = dev.get()
            want, cmp = expected(inp, gold, pres, d, data_only)
            assert (got[cmp] == want[cmp]).all(), data_only
        dev.free()


# ---- 3. unrecoverable items -----------------------------------------------

def test_unrecoverable_items():
    d, p, bs, n = 4, 2, 64 << 10, 8
    total = d + p
    gold = golden(d, p, bs, n, 3000)
    masks = [(0, 1, 1, 1, 1, 1), (1, 1, 0, 1, 0, 1), (0, 0, 1, 1, 0, 1),
             (1, 1, 1, 1, 1, 1), (1, 0, 1, 0, 1, 1), (1, 0, 1, 0, 0, 1),
             (1, 1, 1, 1, 0, 0), (0, 1, 1, 0, 1, 1)]
    with minio_amd.Erasure(d, p, bs) as e:
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        inp, pres = damaged(gold, masks, stride)
        dev = Dev(e, inp)
        for fn in (lib.mec_reconstruct_batch_mixed_dev,
                   lib.mec_reconstruct_batch_mixed_dev_async):
            dev.put(inp)
            rc, st = run_mixed(e, dev, pres, S, 0, fn=fn)
            check(lib.mec_stream_sync(e._ctx))
            assert rc == 0
            assert st == [0, 0, TOO_FEW, 0, 0, TOO_FEW, 0, 0]
            got = dev.get()
            for i in range(n):
                if i in (2, 5):
                    assert (got[i] == inp[i]).all(), i  # untouched
                else:
                    assert (got[i, :, :S] == gold[i]).all(), i
            # no status array: the whole call fails, nothing is modified
            dev.put(inp)
            rc, _ = run_mixed(e, dev, pres, S, 0, fn=fn, status=False)
            check(lib.mec_stream_sync(e._ctx))
            assert rc == TOO_FEW
            assert (dev.get() == inp).all()
        dev.free()


# ---- 4. agreement with the uniform call -----------------------------------

@pytest.mark.parametrize("data_only", [0, 1])
def test_agrees_with_uniform_call(data_only):
    d, p, bs, n = 8, 4, 1 << 20, 32
    total = d + p
    mask = (1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1)
    with minio_amd.Erasure(d, p, bs) as e:
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        inp = np.frombuffer(oracle.fill_random(n * total * stride, 4000),
                            dtype=np.uint8).reshape(n, total, stride)
        pres = np.array([mask] * n, dtype=np.uint8)
        a, b = Dev(e, inp), Dev(e, inp)
        check(lib.mec_reconstruct_batch_dev(e._ctx, n, a.ptr, bytes(mask), S,
                                            data_only))
        rc, st = run_mixed(e, b, pres, S, data_only)
        assert rc == 0 and st == [0] * n
        ga, gb = a.get(), b.get()
        a.free()
        b.free()
    assert not (ga == inp).all()  # the uniform call did rebuild something
    assert (ga == gb).all()


# ---- 5. async ordering ----------------------------------------------------

def test_async_calls_back_to_back():
    """Two _async mixed calls with disjoint pattern sets, then a uniform
    async call with a third mask, one sync at the end: the second call's
    plan table must not overwrite what the first call's kernels read."""
    d, p, bs, n = 8, 4, 64 << 10, 64
    total = d + p
    one = masks_with_erasures(total, (1,))
    three = masks_with_erasures(total, (3,))
    random.Random(5).shuffle(three)
    m1 = [one[i % len(one)] for i in range(n)]
    m2 = three[:n]
    assert not set(m1) & set(m2)
    m3 = (1, 1, 0, 1, 1, 1, 1, 0, 1, 0, 0, 1)
    assert m3 not in m1 and m3 not in m2
    g1, g2, g3 = (golden(d, p, bs, n, s) for s in (5100, 5200, 5300))
    with minio_amd.Erasure(d, p, bs) as e:
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        i1, p1 = damaged(g1, m1, stride)
        i2, p2 = damaged(g2, m2, stride)
        i3, _ = damaged(g3, [m3] * n, stride)
        d1, d2, d3 = Dev(e, i1), Dev(e, i2), Dev(e, i3)
        fn = lib.mec_reconstruct_batch_mixed_dev_async
        rc1, st1 = run_mixed(e, d1, p1, S, 0, fn=fn)
        rc2, st2 = run_mixed(e, d2, p2, S, 0, fn=fn)
        check(lib.mec_reconstruct_batch_dev_async(e._ctx, n, d3.ptr,
                                                  bytes(m3), S, 0))
        check(lib.mec_stream_sync(e._ctx))
        assert rc1 == 0 and rc2 == 0 and st1 == [0] * n and st2 == [0] * n
        o1, o2, o3 = d1.get(), d2.get(), d3.get()
        for dv in (d1, d2, d3):
            dv.free()
    assert (o1[:, :, :S] == g1).all()
    assert (o2[:, :, :S] == g2).all()
    assert (o3[:, :, :S] == g3).all()


# ---- 6. n above 65535 -----------------------------------------------------

def test_more_items_than_a_grid_dimension():
    d, p, bs, n = 8, 4, 512, 70000
    total = d + p
    rs = oracle.RS(d, p)
    gold = golden(d, p, bs, 16, 6000)                       # 16 contents
    S = gold.shape[2]
    assert S == 64
    masks = [(0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1),
             (1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1),
             (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0),
             (0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1),
             (1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1),
             (1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1),
             (0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1, 1),
             (1, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0),
             (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1),
             (0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1),
             (1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1),
             (1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1),
             (1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0)]           # 13 patterns
    pm = np.array(masks, dtype=np.uint8)
    # the 16 x 13 oracle results and their damaged inputs
    inp_cm = np.empty((16, 13, total, S), dtype=np.uint8)
    want_cm = np.empty_like(inp_cm)
    for c in range(16):
        for m in range(13):
            inp_cm[c, m] = gold[c]
            inp_cm[c, m][pm[m] == 0] = HOLE
            ref = oracle_rows(rs, inp_cm[c, m], masks[m], S, 0)
            for s in range(total):
                want_cm[c, m, s] = np.frombuffer(ref[s], dtype=np.uint8)
    ic, im = np.arange(n) % 16, np.arange(n) % 13
    inp = inp_cm[ic, im]
    pres = pm[im]
    with minio_amd.Erasure(d, p, bs) as e:
        assert lib.mec_shard_stride(bs, d) == S
        dev = Dev(e, inp)
        rc, st = run_mixed(e, dev, pres, S, 0)
        got = dev.get()
        dev.free()
    assert rc == 0 and not any(st)
    bad = np.argwhere((got != want_cm[ic, im]).any(axis=(1, 2)))
    assert bad.size == 0, f"first wrong items: {bad[:4].ravel().tolist()}"


# ---- 7. host-pointer and Python paths -------------------------------------

@pytest.mark.parametrize("data_only", [False, True])
def test_python_reconstruct_batch(data_only):
    d, p, bs, n = 8, 4, 64 << 10, 24
    total = d + p
    gold = golden(d, p, bs, n, 7000)
    rng = random.Random(7)
    rs = oracle.RS(d, p)
    items = []
    for i in range(n):
        if i == 4:
            gone = []                                    # all present
        elif i == 9:
            gone = rng.sample(range(total), p + 1)       # unrecoverable
        else:
            gone = rng.sample(range(total), rng.randint(1, p))
        items.append([None if s in gone else bytes(gold[i, s])
                      for s in range(total)])
    with minio_amd.Erasure(d, p, bs) as e:
        out, st = e.reconstruct_batch(items, data_only=data_only)
    assert st == [TOO_FEW if i == 9 else 0 for i in range(n)]
    assert out[9] == items[9]
    assert out[4] == items[4]
    for i in range(n):
        if i in (4, 9):
            continue
        assert out[i] == rs.reconstruct(items[i], data_only=data_only), i


# ---- 8. canary ------------------------------------------------------------

def test_mixed_call_keeps_up_with_uniform_call():
    """Same job through both calls: the mixed call may take at most 2x the
    uniform call measured here, the project's existing 'about 2x, only
    trips when the path stops doing the work' margin."""
    d, p, bs, n = 8, 4, 1 << 20, 256
    total = d + p
    with minio_amd.Erasure(d, p, bs) as e:
        ctx = e._ctx
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        dev = ctypes.c_void_p()
        check(lib.mec_dev_alloc(ctx, n * total * stride, ctypes.byref(dev)))
        check(lib.mec_memset_dev(ctx, dev, 7, n * total * stride))
        present = bytes([0] * 3 + [1] * (total - 3))
        present_n = present * n

        def uniform():
            check(lib.mec_reconstruct_batch_dev(ctx, n, dev, present, S, 1))

        def mixed():
            check(lib.mec_reconstruct_batch_mixed_dev(ctx, n, dev, present_n,
                                                      S, 1, None))

        for _ in range(2):
            uniform()
            mixed()
        t_u = t_m = 0.0
        for _ in range(5):
            t0 = time.perf_counter()
            uniform()
            t1 = time.perf_counter()
            mixed()
            t2 = time.perf_counter()
            t_u += t1 - t0
            t_m += t2 - t1
        lib.mec_dev_free(ctx, dev)
    print(f"uniform {t_u / 5 * 1e3:.3f} ms, mixed {t_m / 5 * 1e3:.3f} ms, "
          f"ratio {t_m / t_u:.2f}")
    assert t_m <= 2 * t_u, f"mixed {t_m / 5 * 1e3:.3f} ms vs uniform " \
                           f"{t_u / 5 * 1e3:.3f} ms"
