"""Loader for tests/golden/reference_shards/: shard files that a reference
server wrote to disk, extracted once by tools/extract_reference_shards.py.

Each .bin holds exactly what lay on one drive: the 32-byte HighwayHash256S
digest followed by the shard.  Nothing here computes a digest or a parity
byte: expected values are the fixture's bytes and the object's MD5 etag.
"""
import hashlib
import itertools
import json
import os

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                   "golden", "reference_shards")

# The objects no pull request may drop (the floor test holds them).
MANDATORY = ("merge-hosts-19113-null", "merge-hosts-228-1f163718",
             "merge-hosts-228-73c9f651")


class RefObject:
    """One manifest entry with its rows loaded.  bins/digests/shards are
    d+p long, indexed by logical row (EcIndex - 1), None where the
    reference tree holds no such row."""

    def __init__(self, entry):
        self.name = entry["name"]
        self.d, self.p = entry["d"], entry["p"]
        self.total = self.d + self.p
        self.block_size = entry["block_size"]
        self.size = entry["size"]
        self.etag = entry["etag"]
        self.dist = entry["dist"]
        self.S = -(-self.size // self.d)
        self.rows = entry["rows"]
        self.bins = [None] * self.total
        for r in self.rows:
            assert r["row"] == r["ec_index"] - 1
            with open(os.path.join(DIR, r["file"]), "rb") as f:
                self.bins[r["row"]] = f.read()
        self.digests = [b and b[:32] for b in self.bins]
        self.shards = [b and b[32:] for b in self.bins]
        self.stored = [i for i, b in enumerate(self.bins) if b is not None]
        self.complete = len(self.stored) == self.total

    def __repr__(self):
        return self.name

    def data(self):
        """The object's bytes (complete objects only)."""
        assert self.complete
        return b"".join(self.shards[:self.d])[:self.size]

    def patterns(self):
        """Every set of 1..p rows to lose."""
        for k in range(1, self.p + 1):
            yield from itertools.combinations(range(self.total), k)

    def without(self, lost, rows=None):
        rows = self.shards if rows is None else rows
        return [None if i in lost else r for i, r in enumerate(rows)]


def md5hex(b):
    return hashlib.md5(b).hexdigest()


def load():
    with open(os.path.join(DIR, "manifest.json")) as f:
        return [RefObject(e) for e in json.load(f)["objects"]]


OBJECTS = load()
COMPLETE = [o for o in OBJECTS if o.complete]
PARTIAL = [o for o in OBJECTS if not o.complete]
