"""GPU tests for the GF lane mapping of the one-pass encode kernel
(fused4.hip): lane (g, o) holds bytes [16o, 16o+16) and [T/2 + 16o,
T/2 + 16o + 16) of each row of block g's tile, and reads, LDS parity writes
and global parity stores all go through those two offsets.

 - every 16-byte chunk of a tile row carries a single non-zero byte in some
   item, so a wrong half or column offset shows up in a named chunk of a
   named row;
 - the parity store addresses respect a row stride longer than the shard;
 - the two store-skipping MEC_F4_PROBE bits keep the barrier contract: the
   launch completes and writes nothing outside its buffers.

The 4-operation transpose is held equal to bs_transpose by a static_assert
in gf_bs.h that every build evaluates, so it has no test of its own here;
the parity comparisons below and test_gpu_fused4.py run it on the device.
"""
import ctypes
import os
import subprocess
import sys

import pytest

import minio_amd
import oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x6C61796F
D, P = 8, 4
TOT = D + P
T = 512      # fused4::T
CANARY = 256
FILL = 0xA5
ALGO = minio_amd.HIGHWAYHASH256S

lib = minio_amd._lib
vp = ctypes.c_void_p
lib.mec_fused4_launches.restype = ctypes.c_uint64
lib.mec_fused4_launches.argtypes = []


@pytest.fixture(autouse=True)
def _every_batch_size_reaches_fused4(monkeypatch):
    monkeypatch.setenv("MEC_F4_MIN", "1")


def check(st):
    assert st == 0, lib.mec_last_error()


class Case:
    """One encode call: `blocks` (each D*S bytes) laid out at the context's
    row stride; parity and sums buffers filled with FILL, with CANARY bytes
    in front of and behind their extents."""

    def __init__(self, e, blocks, S, ctx_bs):
        self.ctx = e._ctx
        self.n, self.S = len(blocks), S
        self.stride = lib.mec_shard_stride(ctx_bs, D)
        n, st = self.n, self.stride
        rows = bytearray(n * D * st)
        for b, blk in enumerate(blocks):
            for k in range(D):
                o = (b * D + k) * st
                rows[o:o + S] = blk[k * S:(k + 1) * S]
        self.par_bytes = n * P * st
        self.sum_bytes = n * TOT * 32
        self.owned = []
        self.data = self.alloc(len(rows))
        check(lib.mec_memcpy_h2d(self.ctx, self.data, bytes(rows), len(rows)))
        self.par_buf = self.alloc(self.par_bytes + 2 * CANARY, FILL)
        self.sum_buf = self.alloc(self.sum_bytes + 2 * CANARY, FILL)
        self.par = vp(self.par_buf.value + CANARY)
        self.sums = vp(self.sum_buf.value + CANARY)

    def alloc(self, nbytes, fill=None):
        ptr = vp()
        check(lib.mec_dev_alloc(self.ctx, nbytes, ctypes.byref(ptr)))
        self.owned.append(ptr)
        if fill is not None:
            check(lib.mec_memset_dev(self.ctx, ptr, fill, nbytes))
        return ptr

    def read(self, ptr, nbytes):
        buf = ctypes.create_string_buffer(nbytes)
        check(lib.mec_memcpy_d2h(self.ctx, buf, ptr, nbytes))
        return buf.raw

    def free(self):
        for ptr in self.owned:
            lib.mec_dev_free(self.ctx, ptr)

    def encode(self):
        """One asynchronous call, then a synchronise; the call must have
        gone through fused4 exactly once."""
        before = lib.mec_fused4_launches()
        check(lib.mec_encode_batch_dev_async(
            self.ctx, self.n, self.data, D * self.S, self.par, ALGO,
            self.sums))
        check(lib.mec_stream_sync(self.ctx))
        assert lib.mec_fused4_launches() - before == 1

    def outputs(self):
        """(parity, sums) extents after checking the four canaries."""
        par = self.read(self.par_buf, self.par_bytes + 2 * CANARY)
        sums = self.read(self.sum_buf, self.sum_bytes + 2 * CANARY)
        can = bytes([FILL]) * CANARY
        assert par[:CANARY] == can, "canary before parity"
        assert par[-CANARY:] == can, "canary after parity"
        assert sums[:CANARY] == can, "canary before sums"
        assert sums[-CANARY:] == can, "canary after sums"
        return par[CANARY:-CANARY], sums[CANARY:-CANARY]


def oracle_outputs(blocks):
    ors = oracle.RS(D, P)
    shards = [ors.encode_data(blk) for blk in blocks]
    sums = [[oracle.bitrot_sum(oracle.HIGHWAYHASH256S, x) for x in sh]
            for sh in shards]
    return shards, sums


def first_bad_chunk(got, want):
    for c in range(0, len(want), 16):
        if got[c:c + 16] != want[c:c + 16]:
            return c // T, (c % T) // 16
    return None


def test_every_half_column_position():
    """S = 2T, n = 65: sixteen full groups of G = 4 and a group with three
    blocks missing.  Item i < 64 is zero but for one byte i + 1 in data row
    i % 8, tile (i / 8) % 2, chunk c = i % 32, byte i % 16 of the chunk;
    item 64 is random."""
    S, n = 2 * T, 65
    blocks = []
    for i in range(n - 1):
        blk = bytearray(D * S)
        c = i % 32
        blk[(i % 8) * S + ((i // 8) % 2) * T + 16 * c + (i % 16)] = i + 1
        blocks.append(bytes(blk))
    blocks.append(oracle.fill_random(D * S, SEED))
    shards, osums = oracle_outputs(blocks)
    with minio_amd.Erasure(D, P, D * S) as e:
        case = Case(e, blocks, S, D * S)
        try:
            case.encode()
            par, sums = case.outputs()
            st = case.stride
            for b in range(n):
                for i in range(P):
                    o = (b * P + i) * st
                    bad = first_bad_chunk(par[o:o + S], shards[b][D + i])
                    assert bad is None, (
                        "parity: item %d parity row %d tile %d chunk %d "
                        "(its byte sits in data row %d, tile %d, chunk %d)"
                        % (b, i, bad[0], bad[1], b % 8, (b // 8) % 2, b % 32))
                for s in range(TOT):
                    o = (b * TOT + s) * 32
                    assert sums[o:o + 32] == osums[b][s], ("digest", b, s)
        finally:
            case.free()


def test_row_stride_longer_than_the_shard():
    """A 1 MiB context (rows 131072 bytes apart) called with 8 x 1536-byte
    blocks: parity rows exact, and every byte of a parity row past S still
    holds the fill pattern."""
    S, n, ctx_bs = 3 * T, 5, 1 << 20
    blocks = [oracle.fill_random(D * S, SEED + 1 + b) for b in range(n)]
    shards, osums = oracle_outputs(blocks)
    with minio_amd.Erasure(D, P, ctx_bs) as e:
        case = Case(e, blocks, S, ctx_bs)
        try:
            assert case.stride == 131072
            case.encode()
            par, sums = case.outputs()
            st = case.stride
            tail = bytes([FILL]) * (st - S)
            for b in range(n):
                for i in range(P):
                    o = (b * P + i) * st
                    bad = first_bad_chunk(par[o:o + S], shards[b][D + i])
                    assert bad is None, ("parity", b, i) + bad
                    assert par[o + S:o + st] == tail, ("row tail written", b, i)
                for s in range(TOT):
                    o = (b * TOT + s) * 32
                    assert sums[o:o + 32] == osums[b][s], ("digest", b, s)
        finally:
            case.free()


_PROBE_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["MEC_TEST_REPO"])
sys.path.insert(0, os.path.join(os.environ["MEC_TEST_REPO"], "tests"))
import minio_amd, oracle
import test_gpu_fused4_layout as t
probe = int(os.environ["MEC_F4_PROBE"])
S, n = 3 * t.T, 5
blocks = [oracle.fill_random(t.D * S, t.SEED + 9 + b) for b in range(n)]
with minio_amd.Erasure(t.D, t.P, t.D * S) as e:
    case = t.Case(e, blocks, S, t.D * S)
    try:
        case.encode()            # MEC_OK, synchronised, one fused4 launch
        par, sums = case.outputs()   # canaries
        if probe & 8:
            assert par == bytes([t.FILL]) * len(par), "parity was stored"
    finally:
        case.free()
print("PROBE_OK", probe)
"""


@pytest.mark.parametrize("probe", [8, 16, 24, 31])
def test_probe_bits_keep_the_barrier_contract(probe):
    """MEC_F4_PROBE is latched per process, hence a fresh child per value.
    Results are declared invalid under a probe and are not compared; the
    launch must complete, and with bit 3 no parity byte may be stored."""
    env = dict(os.environ)
    env["MEC_F4_PROBE"] = str(probe)
    env["MEC_F4_MIN"] = "1"
    env["MEC_TEST_REPO"] = os.path.dirname(HERE)
    r = subprocess.run([os.environ.get("PYTHON", sys.executable), "-c",
                        _PROBE_CHILD], env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0 and "PROBE_OK %d" % probe in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-2000:])
