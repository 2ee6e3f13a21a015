"""GPU tests for the launch shapes of the bit-sliced GF kernels
(gf_encode_bs_kernel, gf_matmul_bs_kernel) that small batches never reach.

 - Grid-stride loops.  gf_grid launches min(ceil(cols/256), ceil(2048 *
   scale / n)) workgroups in x, so a thread takes a second column only when
   n * ceil(cols/256) exceeds 16384 (specialized encode) or 8192 (runtime
   matrix).  n = 16385 and n = 8193 at S = 9376 (293 columns of 32 bytes)
   are the smallest such shapes: one workgroup in x, threads 0..36 take
   two columns, the rest one.
 - More items than a grid's y dimension holds (65535): the launchers slice
   the batch.
 - More than MEC_KMAX_E = 8 output rows on the uniform encode and
   reconstruct: several launches sharing one mask buffer.

All cases go through the device entry points.  Every item has data of its
own, and its reference comes from the CPU oracle, item by item.  The
references are device-layout images: rows at the context's stride with the
marker between a row's end and the next row, so one comparison covers the
rows, the bytes behind them and, with the 256 marker bytes every output
buffer carries at its end, the canary.
"""
import ctypes

import pytest

import minio_amd
import oracle

pytestmark = pytest.mark.gpu

SEED = 0x67666c73
CANARY = 256
FILL = 0xA5
HH = minio_amd.HIGHWAYHASH256S

lib = minio_amd._lib
vp = ctypes.c_void_p


def check(st):
    assert st == 0, lib.mec_last_error()


def as_c(buf):
    """A bytearray as the char array ctypes passes without copying."""
    return (ctypes.c_char * len(buf)).from_buffer(buf)


class Ref:
    """n blocks of block_len bytes encoded by the oracle, as the images the
    device entry points read and write: data (n*d rows), par (n*p rows)
    and, on request, sums (the fused n x (d+p) x 32 HighwayHash256S
    layout); full_image(m) puts the first m items' rows together in the
    reconstruct layout.  Bytes [S, stride) of every row hold FILL.  Images
    of the first m items are prefixes.  Computed once, shared, never
    modified."""

    def __init__(self, d, p, block_len, n, with_sums=False):
        self.d, self.p, self.n, self.block_len = d, p, n, block_len
        self.S = S = oracle.ceil_frac(block_len, d)
        self.stride = st = lib.mec_shard_stride(block_len, d)
        self.cols32 = (S + 31) // 32 * 32
        assert self.cols32 <= st
        t = d + p
        ors = oracle.RS(d, p)
        self.data = bytearray([FILL]) * (n * d * st)
        self.par = bytearray([FILL]) * (n * p * st)
        self.sums = bytearray(n * t * 32) if with_sums else None
        seed = SEED + (d << 40) + (p << 32) + (block_len << 8)
        for b in range(n):
            sh = ors.encode_data(oracle.fill_random(block_len, seed + b))
            for s in range(t):
                if s < d:
                    o = (b * d + s) * st
                    self.data[o:o + S] = sh[s]
                else:
                    o = (b * p + s - d) * st
                    self.par[o:o + S] = sh[s]
                if with_sums:
                    o = (b * t + s) * 32
                    self.sums[o:o + 32] = oracle.bitrot_sum(HH, sh[s])

    def full_image(self, m):
        d, p, st = self.d, self.p, self.stride
        out = bytearray()
        for b in range(m):
            out += memoryview(self.data)[b * d * st:(b + 1) * d * st]
            out += memoryview(self.par)[b * p * st:(b + 1) * p * st]
        return out


@pytest.fixture(scope="module")
def ref_2_2_strided():
    return Ref(2, 2, 2 * 9376, 16385)


@pytest.fixture(scope="module")
def ref_3_1_strided():
    return Ref(3, 1, 3 * 9376, 8193)


@pytest.fixture(scope="module")
def ref_2_2_small():
    return Ref(2, 2, 128, 65537, with_sums=True)


@pytest.fixture(scope="module")
def ref_9_9():
    return Ref(9, 9, 9 * 96, 3)


class Dev:
    """Device buffers of one case, freed on exit."""

    def __init__(self, e):
        self.ctx = e._ctx
        self.owned = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for ptr in self.owned:
            lib.mec_dev_free(self.ctx, ptr)

    def upload(self, image, nbytes):
        """image[:nbytes] followed by CANARY bytes of FILL."""
        ptr = vp()
        check(lib.mec_dev_alloc(self.ctx, nbytes + CANARY, ctypes.byref(ptr)))
        self.owned.append(ptr)
        check(lib.mec_memset_dev(self.ctx, ptr, FILL, nbytes + CANARY))
        if image is not None:
            check(lib.mec_memcpy_h2d(self.ctx, ptr, as_c(image), nbytes))
        return ptr

    def output(self, nbytes):
        return self.upload(None, nbytes)

    def read(self, ptr, nbytes):
        out = bytearray(nbytes + CANARY)
        check(lib.mec_memcpy_d2h(self.ctx, as_c(out), ptr, nbytes + CANARY))
        return out


def assert_image(got, want, nbytes, row_bytes, what, scratch=None):
    """got (nbytes + CANARY) against want[:nbytes] and the canary.  scratch
    = (S, cols32): bytes [S, cols32) of each row are the kernel's to write
    (it stores whole 32-byte columns) and are not compared."""
    assert got[nbytes:] == bytes([FILL]) * CANARY, what + ": canary"
    mv_got, mv_want = memoryview(got), memoryview(want)
    if scratch is None:
        if mv_got[:nbytes] == mv_want[:nbytes]:
            return
        scratch = (row_bytes, row_bytes)
    S, c32 = scratch
    for r in range(nbytes // row_bytes):
        o = r * row_bytes
        if mv_got[o:o + S] != mv_want[o:o + S]:
            first = next(i for i in range(S) if got[o + i] != want[o + i])
            raise AssertionError(
                "%s: row %d differs from byte %d on" % (what, r, first))
        assert mv_got[o + c32:o + row_bytes] == mv_want[o + c32:o + row_bytes], \
            "%s: row %d written past its last column" % (what, r)


def encode_case(ref, n, with_sums=False):
    """mec_encode_batch_dev over the first n items of ref."""
    d, p, st = ref.d, ref.p, ref.stride
    par_bytes, sum_bytes = n * p * st, n * (d + p) * 32
    with minio_amd.Erasure(d, p, ref.block_len) as e, Dev(e) as dev:
        data = dev.upload(ref.data, n * d * st)
        par = dev.output(par_bytes)
        sums = dev.output(sum_bytes) if with_sums else None
        check(lib.mec_encode_batch_dev(dev.ctx, n, data, ref.block_len, par,
                                       HH, sums))
        scratch = (ref.S, ref.cols32) if ref.S != ref.cols32 else None
        assert_image(dev.read(par, par_bytes), ref.par, par_bytes, st,
                     "parity", scratch)
        if with_sums:
            assert_image(dev.read(sums, sum_bytes), ref.sums, sum_bytes, 32,
                         "sums")


def reconstruct_case(ref, n, erased, data_only=False, oracle_items=()):
    """mec_reconstruct_batch_dev over the first n items of ref with the
    rows in erased holding FILL on entry.  The whole in-place buffer is
    compared: rebuilt rows equal the oracle's, every other byte is as it
    was.  For the items in oracle_items the expectation is taken from
    oracle.RS.reconstruct on the damaged item instead of from the encode."""
    d, p, st, S = ref.d, ref.p, ref.stride, ref.S
    assert S == ref.cols32, "rebuilt rows are written in whole columns"
    t = d + p
    nbytes = n * t * st
    want = ref.full_image(n)
    damaged = bytearray(want)
    hole = bytes([FILL]) * st
    ors = oracle.RS(d, p)
    for b in range(n):
        for s in erased:
            o = (b * t + s) * st
            damaged[o:o + st] = hole
            if data_only and s >= d:
                want[o:o + st] = hole
    for b in oracle_items:
        sh = [bytes(want[(b * t + s) * st:(b * t + s) * st + S])
              for s in range(t)]
        rec = ors.reconstruct([None if s in erased else sh[s]
                               for s in range(t)], data_only)
        for s in range(t):
            o = (b * t + s) * st
            assert want[o:o + S] == (rec[s] if rec[s] is not None
                                     else hole[:S]), ("oracle", b, s)
    present = bytes(0 if s in erased else 1 for s in range(t))
    with minio_amd.Erasure(d, p, ref.block_len) as e, Dev(e) as dev:
        buf = dev.upload(damaged, nbytes)
        check(lib.mec_reconstruct_batch_dev(dev.ctx, n, buf, present, S,
                                            1 if data_only else 0))
        assert_image(dev.read(buf, nbytes), want, nbytes, st, "shards")


# ---- grid-stride loops ---------------------------------------------------

def test_specialized_encode_takes_a_second_column(ref_2_2_strided):
    """(2,2), n = 16385, S = 9376, sums = NULL: gf_encode_bs_kernel with
    one workgroup in x over 293 columns."""
    encode_case(ref_2_2_strided, 16385)


def test_specialized_encode_strided_ragged_last_column():
    """block_len = 2*9376 - 3: S = 9375, so the last of the 293 columns is
    one byte short and the second data row ends in Split's zero padding."""
    ref = Ref(2, 2, 2 * 9376 - 3, 16385)
    assert ref.S == 9375 and ref.cols32 == 9376 and ref.stride == 9408
    encode_case(ref, 16385)


def test_runtime_matrix_encode_takes_a_second_column(ref_3_1_strided):
    """(3,1) has no compiled specialization: gf_matmul_bs_kernel, n = 8193."""
    encode_case(ref_3_1_strided, 8193)


def test_reconstruct_takes_a_second_column_3_1(ref_3_1_strided):
    reconstruct_case(ref_3_1_strided, 8193, {0},
                     oracle_items=(0, 1, 4096, 8192))


def test_reconstruct_takes_a_second_column_2_2(ref_2_2_strided):
    """A data row and a parity row rebuilt, two output rows per column."""
    reconstruct_case(ref_2_2_strided, 8193, {0, 3},
                     oracle_items=(0, 1, 4096, 8192))


# ---- more items than gridDim.y holds ---------------------------------------

@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_encode_beyond_the_grid_y_limit(ref_2_2_small, n):
    """One slice exactly full, one item over, two items over; the hash
    launch behind it is linear in x."""
    encode_case(ref_2_2_small, n, with_sums=True)


@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_reconstruct_beyond_the_grid_y_limit(ref_2_2_small, n):
    reconstruct_case(ref_2_2_small, n, {1, 2},
                     oracle_items=(0, 65534, n - 2, n - 1))


# ---- more than MEC_KMAX_E output rows --------------------------------------

def test_encode_nine_parity_rows(ref_9_9):
    """Two launches, 8 + 1 rows, the masks re-uploaded in between."""
    encode_case(ref_9_9, 3)


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("erased", [
    set(range(9)),                       # every data row: 8 + 1
    {0, 2, 4, 6, 8, 9, 11, 13, 15},      # 5 data + 4 parity rows: 8 + 1
], ids=["9data", "5data4parity"])
def test_reconstruct_nine_rows(ref_9_9, erased, data_only):
    reconstruct_case(ref_9_9, 3, erased, data_only, oracle_items=(0, 1, 2))
