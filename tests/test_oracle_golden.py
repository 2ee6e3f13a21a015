"""Oracle vs the reference's own boot-time golden vectors.

These pin the CPU oracle bit-exactly to the reference:
 - erasureSelfTest fingerprints (cmd/erasure-coding.go:149-206): xxh64 over
   index||shard of the full encode of bytes 0..255, 60 (d,p) configs, plus
   the delete-shard-0-and-reconstruct check.
 - bitrotSelfTest chained digests (cmd/bitrot.go:224-255) for
   SHA256 / BLAKE2b512 / HighwayHash256(S) with the magic key.
 - whole objects as a reference server wrote them to disk
   (tests/golden/reference_shards/): stored digests, data and parity rows,
   MD5 etags, at shard lengths with ragged HighwayHash tails.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

import oracle


def test_erasure_selftest_fingerprints():
    golden = json.load(open(os.path.join(HERE, "golden/erasure_selftest.json")))
    data = bytes(range(256))
    for key, want in golden["fingerprints"].items():
        d, p = map(int, key.split(","))
        rs = oracle.RS(d, p)
        shards = rs.encode_data(data)
        stream = b"".join(bytes([i]) + s for i, s in enumerate(shards))
        got = f"{oracle.xxh64(stream):016x}"
        assert got == want, f"d={d} p={p}"
        # reconstruct check (cmd/erasure-coding.go:192-200)
        first = shards[0]
        shards2 = [None] + shards[1:]
        rec = rs.reconstruct(shards2, data_only=True)
        assert rec[0] == first, f"reconstruct d={d} p={p}"


def test_bitrot_selftest_digests():
    golden = json.load(open(os.path.join(HERE, "golden/bitrot_selftest.json")))
    block_sizes = {"SHA256": (oracle.SHA256, 64),
                   "HighwayHash256": (oracle.HIGHWAYHASH256, 32),
                   "HighwayHash256S": (oracle.HIGHWAYHASH256S, 32),
                   "BLAKE2b512": (oracle.BLAKE2B512, 128)}
    for name, (algo, block) in block_sizes.items():
        size = oracle.bitrot_size(algo)
        msg = b""
        sum_ = b""
        for _ in range(block):
            sum_ = oracle.bitrot_sum(algo, msg)
            msg += sum_
        assert sum_.hex() == golden["digests"][name], name


# ---- shard files a reference server wrote to disk --------------------------
#
# tests/golden/reference_shards/ holds complete objects as they lay on the
# drives: per row the 32-byte HighwayHash256S digest followed by the shard,
# with the erasure geometry and the object's MD5 etag in manifest.json (see
# tools/extract_reference_shards.py).  Expected values below are fixture
# bytes and hashlib.md5, never an oracle call.  Shard lengths 114, 9557 and
# 214840 end in 18, 21 and 24 bytes modulo 32: the `size_mod32 & 16` branch
# of UpdateRemainder with size_mod4 = 2, 1, 0.  66048 has no tail.

import hashlib
import re

import pytest

import reference_shards as refs

HH_KEY = bytes.fromhex(
    "4be734fa8e238acd263e83e6bb968552040f935da39f441497e09d1322de36a0")


def test_reference_shards_floor():
    """The fixture set cannot silently shrink: the mandatory objects are
    there and complete, and between them a ragged shard of each of the two
    EC2+2 sizes."""
    by_name = {o.name: o for o in refs.OBJECTS}
    for name in refs.MANDATORY:
        assert name in by_name, name
        assert by_name[name].complete, name
    ragged = {o.size for o in refs.COMPLETE
              if (o.d, o.p) == (2, 2) and o.S % 32 != 0}
    assert ragged >= {228, 19113}, ragged
    assert {by_name[n].S % 32 for n in refs.MANDATORY} == {18, 21}
    for o in refs.OBJECTS:
        assert len(o.stored) >= o.d, o  # at least decodable
        assert o.size <= o.block_size, o  # one short block each
        for b in o.bins:
            assert b is None or len(b) == 32 + o.S, o


@pytest.mark.parametrize("obj", refs.OBJECTS, ids=repr)
def test_reference_shards_fixture_intact(obj):
    for r in obj.rows:
        got = hashlib.sha256(obj.bins[r["row"]]).hexdigest()
        assert got == r["sha256"], r["file"]
        # placement: drive k of the set holds row EcDist[k-1] (the number
        # in the drive's name counts within its set of d+p)
        k = (int(re.search(r"\d+$", r["disk"]).group()) - 1) % obj.total
        assert obj.dist[k] == r["ec_index"], r["file"]


@pytest.mark.parametrize("obj", refs.OBJECTS, ids=repr)
def test_reference_shards_digests(obj):
    """The scalar oracle, under both HighwayHash ids, and the AVX2 leg
    reproduce the digest the reference stored in front of every row."""
    for i in obj.stored:
        for algo in (oracle.HIGHWAYHASH256S, oracle.HIGHWAYHASH256):
            assert oracle.bitrot_sum(algo, obj.shards[i]) == obj.digests[i], \
                (obj, i, algo)
        assert oracle.hh256_fast(HH_KEY, obj.shards[i]) == obj.digests[i], \
            (obj, i, oracle.cpu_isa())


@pytest.mark.parametrize("obj", refs.COMPLETE, ids=repr)
def test_reference_shards_encode(obj):
    data = obj.data()
    assert refs.md5hex(data) == obj.etag
    # Split's zero pad, as stored
    pad = obj.S * obj.d - obj.size
    assert obj.shards[obj.d - 1][obj.S - pad:] == b"\0" * pad
    assert oracle.RS(obj.d, obj.p).encode_data(data) == obj.shards
    streams, _ = oracle.encode_stream(obj.d, obj.p, obj.block_size, data,
                                      oracle.HIGHWAYHASH256S)
    assert streams == obj.bins


@pytest.mark.parametrize("obj", refs.COMPLETE, ids=repr)
def test_reference_shards_reconstruct(obj):
    rs = oracle.RS(obj.d, obj.p)
    for lost in obj.patterns():
        assert rs.reconstruct(obj.without(lost)) == obj.shards, lost
        rec = rs.reconstruct(obj.without(lost), data_only=True)
        assert rec[:obj.d] == obj.shards[:obj.d], lost


@pytest.mark.parametrize("obj", refs.PARTIAL, ids=repr)
def test_reference_shards_partial_decodes(obj):
    """Only some rows exist: rebuild the data rows from them and compare
    the object's MD5 with its etag."""
    rec = oracle.RS(obj.d, obj.p).reconstruct(list(obj.shards),
                                              data_only=True)
    for i in obj.stored:
        assert rec[i] == obj.shards[i]
    assert refs.md5hex(b"".join(rec[:obj.d])[:obj.size]) == obj.etag
