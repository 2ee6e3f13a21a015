"""GPU tests for the SHA-256 and BLAKE2b-512 batch kernels (kernels.hip).

Every digest has two independent references, the CPU oracle and Python's
hashlib; each case first asserts that the two agree on the CPU and then that
the device matches them.  Messages go through the device entry
mec_bitrot_sum_batch_dev at a row stride of the test's choosing, with the
bytes between a message's end and the next row holding a marker the digest
must not depend on, and the digests come back in a buffer pre-filled with
the marker and 256 bytes longer than its extent.

Shapes are the ones at which the kernels take another path:
 - SHA-256 keeps two chains per lane and 512 chains per workgroup, loads
   whole 64-byte blocks one ahead (edges at 64 and 128 bytes left) and pads
   into one tail block below 56 bytes left and two from 56 on: every length
   0..255 at an odd chain count, and chain counts around one lane, one
   workgroup and three workgroups at a length with a two-block tail;
 - BLAKE2b-512 keeps one chain per lane and 256 per workgroup and loads a
   128-byte block ahead while more than 128 bytes are left: every length
   0..385, and chain counts around one and two workgroups;
 - both at a row stride that is a multiple of 16 but not of 64;
 - both through the fused n x (d+p) sums layout of an encode call, on a
   compiled specialization and on the runtime-matrix path.
"""
import ctypes
import functools
import hashlib

import pytest

import minio_amd
import oracle

pytestmark = pytest.mark.gpu

SEED = 0x68617368
CANARY = 256
FILL = 0xA5
SHA, B2B = minio_amd.SHA256, minio_amd.BLAKE2B512
HSZ = {SHA: 32, B2B: 64}

lib = minio_amd._lib
vp = ctypes.c_void_p


def check(st):
    assert st == 0, lib.mec_last_error()


def hashlib_sum(algo, msg):
    if algo == SHA:
        return hashlib.sha256(msg).digest()
    return hashlib.blake2b(msg, digest_size=64).digest()


@functools.lru_cache(maxsize=None)
def chain(algo, L, c):
    """(message, digest) of chain c at length L: the message from the
    oracle's generator under a seed of its own, the digest from the oracle
    once hashlib has confirmed it."""
    msg = oracle.fill_random(L, SEED + (algo << 24) + L * 4099 + c)
    want = oracle.bitrot_sum(algo, msg)
    assert want == hashlib_sum(algo, msg), ("oracle vs hashlib", algo, L, c)
    return msg, want


@pytest.fixture(scope="module")
def ctx():
    """The hash entry only uses the context's device and stream."""
    with minio_amd.Erasure(2, 2, 1024) as e:
        yield e._ctx


def roundup64(x):
    return (x + 63) & ~63


def device_case(ctx, algo, L, n, stride):
    """n chains of L bytes, stride apart, through mec_bitrot_sum_batch_dev;
    slot i must hold chain i's digest and the canary must survive."""
    assert stride >= L and n < 4099
    hs = HSZ[algo]
    rows = bytearray([FILL]) * (n * stride)
    want = []
    for c in range(n):
        msg, dig = chain(algo, L, c)
        rows[c * stride:c * stride + L] = msg
        want.append(dig)
    owned = []

    def alloc(nbytes):
        ptr = vp()
        check(lib.mec_dev_alloc(ctx, nbytes, ctypes.byref(ptr)))
        owned.append(ptr)
        return ptr

    try:
        msgs = alloc(len(rows))
        check(lib.mec_memcpy_h2d(ctx, msgs, bytes(rows), len(rows)))
        sums = alloc(n * hs + CANARY)
        check(lib.mec_memset_dev(ctx, sums, FILL, n * hs + CANARY))
        check(lib.mec_bitrot_sum_batch_dev(ctx, algo, n, msgs, L, stride,
                                           sums))
        buf = ctypes.create_string_buffer(n * hs + CANARY)
        check(lib.mec_memcpy_d2h(ctx, buf, sums, n * hs + CANARY))
        got = buf.raw
    finally:
        for ptr in owned:
            lib.mec_dev_free(ctx, ptr)
    for c in range(n):
        assert got[c * hs:(c + 1) * hs] == want[c], ("digest", algo, L, c)
    assert got[n * hs:] == bytes([FILL]) * CANARY, "sums canary"


@pytest.mark.parametrize("L", range(256))
def test_sha256_every_length(ctx, L):
    """Five chains: two full lanes and one whose second slot is inactive.
    Every mod-64 residue with no full block, with one (no prefetch) and
    with two or three (prefetch taken, then not)."""
    device_case(ctx, SHA, L, 5, max(64, roundup64(L)))


@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 1025])
def test_sha256_chain_counts(ctx, n):
    """L = 119 is one full block and a two-block tail.  One chain beside
    an inactive slot, one workgroup short of a chain, full, and one chain
    over, and three workgroups with an odd tail."""
    device_case(ctx, SHA, 119, n, 128)


@pytest.mark.parametrize("L", range(386))
def test_blake2b512_every_length(ctx, L):
    """Three chains; crosses the > 128 loop edge at 128, 256 and 384 from
    both sides and includes the empty message."""
    device_case(ctx, B2B, L, 3, max(64, roundup64(L)))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_blake2b512_chain_counts(ctx, n):
    device_case(ctx, B2B, 129, n, 192)


@pytest.mark.parametrize("L", [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128,
                               129, 255, 256])
@pytest.mark.parametrize("algo", [SHA, B2B])
def test_row_stride_multiple_of_16_only(ctx, algo, L):
    """Rows 272 bytes apart: 16-byte aligned, never 64-byte aligned twice
    in a row.  The gap bytes [L, 272) hold the marker."""
    device_case(ctx, algo, L, 5, 272)


@pytest.mark.parametrize("d,p", [(3, 2), (7, 2)])
@pytest.mark.parametrize("algo", [SHA, B2B])
def test_fused_sums_layout_through_encode(algo, d, p):
    """encode_batch with a whole-file algorithm: the hash kernels' chain to
    (block, shard) mapping with a parity pointer.  (3,2) is a compiled
    specialization (15 chains, an odd count), (7,2) takes the
    runtime-matrix kernel (27 chains); S = 100 either way."""
    n, block_len = 3, d * 100
    data = oracle.fill_random(n * block_len, SEED + algo * 131 + d)
    ors = oracle.RS(d, p)
    with minio_amd.Erasure(d, p, block_len) as e:
        shards, sums = e.encode_batch(data, block_len, n, algo)
    for b in range(n):
        want = ors.encode_data(data[b * block_len:(b + 1) * block_len])
        assert shards[b] == want, ("shards", b)
        for s, sh in enumerate(want):
            ref = oracle.bitrot_sum(algo, sh)
            assert ref == hashlib_sum(algo, sh), ("oracle vs hashlib", b, s)
            assert sums[b][s] == ref, ("digest", b, s)
