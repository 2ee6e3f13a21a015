#!/usr/bin/env python3
"""Extract reference-written shard files into tests/golden/reference_shards/.

    python tools/extract_reference_shards.py REFERENCE_DIR OUT_DIR

The reference tree ships complete objects that a real server wrote to disk,
for its own metadata tests.  This tool reads the xl.meta files (and part.1
files) of those objects and writes, per object, one raw .bin per stored
shard row -- exactly the on-disk bytes, the 32-byte HighwayHash256S digest
followed by the shard -- plus one manifest.json entry with the erasure
geometry, the shard distribution and the object's MD5 etag.

Run by hand on a development machine that has the reference tree; no test,
smoke() or bench.py calls it, and nothing reads the reference at test time.
Only shard bytes and settings are written: no xl.meta, no zip.

xl.meta layout read here (format version 1.x):
    "XL2 " | major u16le | minor u16le | msgpack bin (metadata)
           | msgpack uint (CRC) | inline section
    inline section: 1 version byte | msgpack map {key: bytes}
    metadata, minor >= 3: header version, meta version, count, then per
                          version a bin (header) and a bin (msgpack map)
    metadata, minor <  3: msgpack map {"Versions": [map, ...]}
An inline key is the version's UUID, or "null" for the null version.
"""
import hashlib
import json
import os
import sys
import uuid
import zipfile

import msgpack

HASH = 32  # HighwayHash256S digest in front of every shard


def _ceil(n, d):
    return -(-n // d)


def parse_xl_meta(buf):
    """Returns (object versions, inline map).  A version is the V2Obj map
    of one xl.meta entry with str keys."""
    if buf[:4] != b"XL2 ":
        raise ValueError("not an xl.meta: bad magic")
    major = int.from_bytes(buf[4:6], "little")
    minor = int.from_bytes(buf[6:8], "little")
    if major != 1:
        raise ValueError(f"xl.meta major version {major} not handled")
    outer = msgpack.Unpacker(raw=True, strict_map_key=False,
                             max_buffer_size=0)
    outer.feed(buf[8:])
    meta = outer.unpack()
    if not isinstance(meta, bytes):
        raise ValueError("xl.meta metadata is not a msgpack bin")
    outer.unpack()  # CRC of the metadata; the .bin SHA-256 guards ours
    rest = buf[8 + outer.tell():]
    inline = {}
    if rest:
        if rest[0] != 1:
            raise ValueError(f"inline section version {rest[0]} not handled")
        if len(rest) > 1:
            inline = {k.decode(): v for k, v in
                      msgpack.unpackb(rest[1:], raw=True).items()}
    bodies = []
    if minor >= 3:
        inner = msgpack.Unpacker(raw=True, strict_map_key=False,
                                 max_buffer_size=0)
        inner.feed(meta)
        inner.unpack()  # header version
        inner.unpack()  # meta version
        for _ in range(inner.unpack()):
            inner.unpack()  # per-version header
            bodies.append(msgpack.unpackb(inner.unpack(), raw=True,
                                          strict_map_key=False))
    else:
        bodies = msgpack.unpackb(meta, raw=True,
                                 strict_map_key=False)[b"Versions"]
    versions = []
    for body in bodies:
        obj = body.get(b"V2Obj")
        if body.get(b"Type") == 1 and obj:
            versions.append({k.decode(): v for k, v in obj.items()})
    return versions, inline


def inline_key(ver):
    vid = uuid.UUID(bytes=ver["ID"])
    return "null" if vid.int == 0 else str(vid)


def describe(ver):
    """The settings of one version that a manifest entry records."""
    if ver["EcAlgo"] != 1 or ver["CSumAlgo"] != 1:
        raise ValueError("not ReedSolomon + HighwayHash256S")
    if len(ver["PartSizes"]) != 1:
        raise ValueError("multi-part objects are not handled")
    return {
        "d": ver["EcM"], "p": ver["EcN"], "block_size": ver["EcBSize"],
        "size": ver["Size"], "etag": ver["MetaUsr"][b"etag"].decode(),
        "dist": list(ver["EcDist"]),
    }


class Collector:
    def __init__(self, out_dir):
        self.out_dir = out_dir
        self.objects = {}

    def add(self, name, source, settings, ec_index, disk, blob):
        d, size = settings["d"], settings["size"]
        if size > settings["block_size"]:
            raise ValueError(f"{name}: more than one block")
        S = _ceil(size, d)
        if len(blob) != HASH + S:
            raise ValueError(f"{name}: row {ec_index - 1} holds {len(blob)} "
                             f"bytes, want {HASH + S}")
        obj = self.objects.setdefault(
            name, dict(name=name, source=source, **settings,
                       shard_size=S, rows=[]))
        for k, v in settings.items():
            if obj[k] != v:
                raise ValueError(f"{name}: drives disagree on {k}")
        if any(r["ec_index"] == ec_index for r in obj["rows"]):
            raise ValueError(f"{name}: EcIndex {ec_index} twice")
        fname = f"{name}.row{ec_index - 1}.bin"
        with open(os.path.join(self.out_dir, fname), "wb") as f:
            f.write(blob)
        obj["rows"].append({
            "file": fname, "ec_index": ec_index, "row": ec_index - 1,
            "disk": disk, "sha256": hashlib.sha256(blob).hexdigest(),
        })

    def finish(self):
        objs = []
        for obj in self.objects.values():
            obj["rows"].sort(key=lambda r: r["row"])
            obj["complete"] = len(obj["rows"]) == obj["d"] + obj["p"]
            objs.append(obj)
        with open(os.path.join(self.out_dir, "manifest.json"), "w") as f:
            json.dump({"objects": objs}, f, indent=1)
            f.write("\n")
        return objs


def from_merge_zip(ref, col):
    rel = "cmd/testdata/xl-meta-merge.zip"
    with zipfile.ZipFile(os.path.join(ref, rel)) as z:
        for n in range(1, 9):
            disk = f"xl{n}"
            member = f"{disk}/testbucket/hosts/xl.meta"
            versions, inline = parse_xl_meta(z.read(member))
            for ver in versions:
                key = inline_key(ver)
                st = describe(ver)
                tag = "null" if key == "null" else key[:8]
                col.add(f"merge-hosts-{st['size']}-{tag}",
                        f"{rel}:xl*/testbucket/hosts/xl.meta inline {key}",
                        st, ver["EcIndex"], disk, inline[key])


def from_inline_notinline_zip(ref, col):
    rel = "cmd/testdata/xl-meta-inline-notinline.zip"
    with zipfile.ZipFile(os.path.join(ref, rel)) as z:
        for disk in ("disk1", "disk2"):
            base = f"{disk}/testbucket/file/"
            versions, inline = parse_xl_meta(z.read(base + "xl.meta"))
            (ver,) = versions
            key = inline_key(ver)
            if key in inline:
                blob = inline[key]
            else:
                blob = z.read(f"{base}{uuid.UUID(bytes=ver['DDir'])}/part.1")
            st = describe(ver)
            col.add(f"inline-notinline-file-{st['size']}",
                    f"{rel}:disk*/testbucket/file", st, ver["EcIndex"],
                    disk, blob)


def from_cicd_corpus(ref, col):
    """Five drives of one set; the version whose data directory every
    drive holds.  The corpus leaves xl.meta, or this version's entry in it,
    out on some drives (its own test heals them), so such a drive's EcIndex
    comes from EcDist: drive k of the
    set holds row EcDist[k-1], which the other drives confirm."""
    rel = "buildscripts/cicd-corpus"
    ddir = "2b4f7e41-df82-4a5e-a3c1-8df87f83332f"
    found, st = {}, None
    for n in range(1, 6):
        base = os.path.join(ref, rel, f"disk{n}", "bucket", "testobj")
        if not os.path.exists(os.path.join(base, "xl.meta")):
            found[n] = None
            continue
        with open(os.path.join(base, "xl.meta"), "rb") as f:
            versions, _ = parse_xl_meta(f.read())
        match = [v for v in versions
                 if str(uuid.UUID(bytes=v["DDir"])) == ddir]
        if not match:  # this drive's xl.meta lost the version as well
            found[n] = None
            continue
        (ver,) = match
        st = describe(ver)
        if ver["EcIndex"] != st["dist"][n - 1]:
            raise ValueError(f"disk{n}: EcIndex is not EcDist[{n - 1}]")
        found[n] = ver["EcIndex"]
    for n, ec_index in found.items():
        path = os.path.join(ref, rel, f"disk{n}", "bucket", "testobj", ddir,
                            "part.1")
        with open(path, "rb") as f:
            blob = f.read()
        col.add(f"cicd-testobj-{st['size']}", f"{rel}/disk*/bucket/testobj",
                st, ec_index or st["dist"][n - 1], f"disk{n}", blob)


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    ref, out_dir = argv[1], argv[2]
    os.makedirs(out_dir, exist_ok=True)
    col = Collector(out_dir)
    from_merge_zip(ref, col)
    from_inline_notinline_zip(ref, col)
    from_cicd_corpus(ref, col)
    for obj in col.finish():
        print(f"{obj['name']}: EC{obj['d']}+{obj['p']} size {obj['size']} "
              f"S {obj['shard_size']} rows "
              f"{[r['row'] for r in obj['rows']]}")


if __name__ == "__main__":
    main(sys.argv)
