"""GPU tests for the one-pass encode + HighwayHash kernel (fused4.hip).

Every case is bit-exact three ways: against the CPU oracle, and, in the
same process, against the kernel pair the one-pass kernel replaces (parity
from an encode call with sums = NULL, digests from
mec_bitrot_sum_batch_dev).  mec_fused4_launches() tells which path ran,
since the results are the same by design.

Shapes are the smallest at which the kernel takes another path.  With
T = 512 bytes per row per step and DP = 6 data ring slots:
 - shard lengths T, 2T (shorter than the pipeline is deep), (DP-1)T, DP*T,
   (DP+1)T (the ring wraps once) and 2*DP*T + T (it wraps twice);
 - batch sizes 1 and 3 (a partial group of G = 4), 4 (one group), 5 and 9
   (full groups plus a partial one).
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
SEED = 0x66757334
D, P = 8, 4
TOT = D + P
T = 512      # fused4::T
DP = 6       # fused4::DP
NMAX = 9
CANARY = 256
FILL = 0xA5
ALGO = minio_amd.HIGHWAYHASH256S
LENGTHS = [T, 2 * T, (DP - 1) * T, DP * T, (DP + 1) * T, 2 * DP * T + T]
BATCHES = [1, 3, 4, 5, 9]

lib = minio_amd._lib
vp = ctypes.c_void_p
lib.mec_fused4_launches.restype = ctypes.c_uint64
lib.mec_fused4_launches.argtypes = []

_REF = {}


@pytest.fixture(autouse=True)
def _every_batch_size_reaches_fused4(monkeypatch):
    """The default threshold sends small batches to the pair, where it is
    faster; these tests are about the one-pass kernel at small shapes."""
    monkeypatch.setenv("MEC_F4_MIN", "1")


def reference(S, n=NMAX):
    """(blocks, shards, sums) of max(n, NMAX) blocks of 8*S bytes from the
    oracle; computed once per length and shared, never modified."""
    count = max(n, NMAX)
    if (S, count) not in _REF:
        ors = oracle.RS(D, P)
        blocks, shards, sums = [], [], []
        for b in range(count):
            blk = oracle.fill_random(D * S, SEED + S * 31 + b)
            sh = ors.encode_data(blk)
            blocks.append(blk)
            shards.append(sh)
            sums.append([oracle.bitrot_sum(oracle.HIGHWAYHASH256S, x)
                         for x in sh])
        _REF[S, count] = (blocks, shards, sums)
    return _REF[S, count]


def check(st):
    assert st == 0, lib.mec_last_error()


class Bufs:
    """Device buffers of one case: data rows at the context's stride, and
    parity / sums outputs pre-filled with FILL, CANARY bytes longer than
    their extents."""

    def __init__(self, e, n, S, ctx_bs, outputs=1):
        self.ctx = e._ctx
        self.n, self.S = n, S
        self.stride = lib.mec_shard_stride(ctx_bs, D)
        blocks, _, _ = reference(S, n)
        rows = bytearray(n * D * self.stride)
        for b in range(n):
            for k in range(D):
                o = (b * D + k) * self.stride
                rows[o:o + S] = blocks[b][k * S:(k + 1) * S]
        self.par_bytes = n * P * self.stride
        self.sum_bytes = n * TOT * 32
        self.data = self.alloc(len(rows))
        check(lib.mec_memcpy_h2d(self.ctx, self.data, bytes(rows), len(rows)))
        self.par = [self.alloc(self.par_bytes + CANARY, FILL)
                    for _ in range(outputs + 1)]
        self.sums = [self.alloc(self.sum_bytes + CANARY, FILL)
                     for _ in range(outputs + 1)]
        self.owned = [self.data] + self.par + self.sums

    def alloc(self, nbytes, fill=None):
        ptr = vp()
        check(lib.mec_dev_alloc(self.ctx, nbytes, ctypes.byref(ptr)))
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

    def run_pair(self):
        """The kernel pair into the LAST output set: parity by an encode
        call without sums, digests by the batch hash over data rows and
        over those parity rows."""
        par, sums = self.par[-1], self.sums[-1]
        check(lib.mec_encode_batch_dev(self.ctx, self.n, self.data,
                                       D * self.S, par, ALGO, None))
        n, S, st = self.n, self.S, self.stride
        tmp_d = self.alloc(n * D * 32)
        tmp_p = self.alloc(n * P * 32)
        self.owned += [tmp_d, tmp_p]
        check(lib.mec_bitrot_sum_batch_dev(self.ctx, ALGO, n * D, self.data,
                                           S, st, tmp_d))
        check(lib.mec_bitrot_sum_batch_dev(self.ctx, ALGO, n * P, par,
                                           S, st, tmp_p))
        sd = self.read(tmp_d, n * D * 32)
        sp = self.read(tmp_p, n * P * 32)
        out = b""
        for b in range(n):
            out += sd[b * D * 32:(b + 1) * D * 32]
            out += sp[b * P * 32:(b + 1) * P * 32]
        return self.read(par, self.par_bytes + CANARY), out

    def verify(self, idx, pair):
        """Output set idx against the oracle and the pair; bytes the call
        must not write (row tails past S, the canaries) still hold FILL."""
        n, S, st = self.n, self.S, self.stride
        _, shards, osums = reference(S, n)
        par = self.read(self.par[idx], self.par_bytes + CANARY)
        sums = self.read(self.sums[idx], self.sum_bytes + CANARY)
        pair_par, pair_sums = pair
        for b in range(n):
            for i in range(P):
                o = (b * P + i) * st
                assert par[o:o + S] == shards[b][D + i], ("parity", b, i)
                assert par[o + S:o + st] == bytes([FILL]) * (st - S), \
                    ("row tail written", b, i)
            for s in range(TOT):
                o = (b * TOT + s) * 32
                assert sums[o:o + 32] == osums[b][s], ("digest", b, s)
        assert par[self.par_bytes:] == bytes([FILL]) * CANARY, "parity canary"
        assert sums[self.sum_bytes:] == bytes([FILL]) * CANARY, "sums canary"
        assert par == pair_par, "parity differs from the pair's"
        assert sums[:self.sum_bytes] == pair_sums, "digests differ from the pair's"


def encode_case(n, S, ctx_bs, expect_fused4):
    with minio_amd.Erasure(D, P, ctx_bs) as e:
        bufs = Bufs(e, n, S, ctx_bs)
        try:
            before = lib.mec_fused4_launches()
            check(lib.mec_encode_batch_dev(bufs.ctx, n, bufs.data, D * S,
                                           bufs.par[0], ALGO, bufs.sums[0]))
            ran = lib.mec_fused4_launches() - before
            assert ran == (1 if expect_fused4 else 0), ran
            pair = bufs.run_pair()
            assert lib.mec_fused4_launches() - before == ran, \
                "the pair's legs must not go through fused4"
            bufs.verify(0, pair)
        finally:
            bufs.free()


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("tiles", [L // T for L in LENGTHS])
def test_fused4_lengths_and_batches(tiles, n):
    S = tiles * T
    encode_case(n, S, D * S, True)


def test_fused4_second_round_of_workgroups():
    """258 workgroups on 256 compute units, the last one holding a single
    block: the kernel's second round, with a partial group in it."""
    encode_case(4 * 256 + 5, T, D * T, True)


@pytest.mark.parametrize("n", [3, 9])
def test_fused4_row_stride_differs_from_shard_len(n):
    """A 1 MiB context called with a short block_len: rows lie 128 KiB
    apart while the shards are 7 tiles long."""
    encode_case(n, (DP + 1) * T, 1 << 20, True)


@pytest.mark.parametrize("n", [3, 5])
def test_fused4_ineligible_length_falls_back(n):
    """S = T + 32 is no multiple of the tile: the pair runs, same results."""
    encode_case(n, T + 32, D * (T + 32), False)


def test_fused4_batch_threshold_is_per_context(monkeypatch):
    """MEC_F4_MIN is read when a context is created, not latched: a context
    created under MEC_F4_MIN=5 sends n = 4 to the pair and n = 5 to
    fused4; a later context created under MEC_F4_MIN=1 sends n = 4 to
    fused4 again."""
    S = DP * T
    monkeypatch.setenv("MEC_F4_MIN", "5")
    encode_case(4, S, D * S, False)
    encode_case(5, S, D * S, True)
    monkeypatch.setenv("MEC_F4_MIN", "1")
    encode_case(4, S, D * S, True)


def test_fused4_default_rule_follows_the_fill_of_the_last_round(monkeypatch):
    """Without MEC_F4_MIN the context decides by how full the last round of
    one workgroup (4 blocks) per compute unit is: 9 blocks go to the pair,
    and so does one workgroup more than a round; a full round goes to
    fused4."""
    monkeypatch.delenv("MEC_F4_MIN")
    cus = 256  # MI355X
    encode_case(9, T, D * T, False)
    encode_case(4 * cus, T, D * T, True)
    encode_case(4 * cus + 4, T, D * T, False)


def test_fused4_async_back_to_back():
    """Two _async calls into different outputs, then one sync."""
    n, S = 9, 2 * DP * T + T
    with minio_amd.Erasure(D, P, D * S) as e:
        bufs = Bufs(e, n, S, D * S, outputs=2)
        try:
            before = lib.mec_fused4_launches()
            for idx in (0, 1):
                check(lib.mec_encode_batch_dev_async(
                    bufs.ctx, n, bufs.data, D * S, bufs.par[idx], ALGO,
                    bufs.sums[idx]))
            check(lib.mec_stream_sync(bufs.ctx))
            assert lib.mec_fused4_launches() - before == 2
            pair = bufs.run_pair()
            bufs.verify(0, pair)
            bufs.verify(1, pair)
        finally:
            bufs.free()


def test_fused4_pipe_entry():
    """mec_encode_batch_dev_pipe takes the one-pass kernel too."""
    n, S = 5, (DP + 1) * T
    with minio_amd.Erasure(D, P, D * S) as e:
        bufs = Bufs(e, n, S, D * S, outputs=2)
        try:
            before = lib.mec_fused4_launches()
            for idx in (0, 1):
                check(lib.mec_encode_batch_dev_pipe(
                    bufs.ctx, n, bufs.data, D * S, bufs.par[idx], ALGO,
                    bufs.sums[idx]))
            check(lib.mec_pipe_sync(bufs.ctx))
            assert lib.mec_fused4_launches() - before == 2
            pair = bufs.run_pair()
            bufs.verify(0, pair)
            bufs.verify(1, pair)
        finally:
            bufs.free()


_KNOB_OFF = r"""
import os, sys
sys.path.insert(0, os.environ["MEC_TEST_REPO"])
sys.path.insert(0, os.path.join(os.environ["MEC_TEST_REPO"], "tests"))
import test_gpu_fused4 as t
t.encode_case(5, t.DP * t.T, t.D * t.DP * t.T, False)
print("KNOB_OFF_OK")
"""


def test_fused4_knob_off():
    """MEC_FUSED4=0 on an eligible shape: the pair runs (the knob is read
    once per process, hence the subprocess), same results."""
    env = dict(os.environ)
    env["MEC_FUSED4"] = "0"
    env["MEC_TEST_REPO"] = os.path.dirname(HERE)
    r = subprocess.run([os.environ.get("PYTHON", sys.executable), "-c",
                        _KNOB_OFF], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "KNOB_OFF_OK" in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-2000:])
