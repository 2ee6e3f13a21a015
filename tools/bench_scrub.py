#!/usr/bin/env python3
"""Measure mec_bitrot_verify_files* (the batch scrub) against what a caller
can do without it, on one MI355X.

HighwayHash256S shard files in the on-disk [hash||shard]* format, resident
in HBM (cases A, B) or in host memory (case C), a host clock around calls
that end in a stream synchronise, the contenders of a case alternating in
one process.  Cases:

  A   aligned, large: EC8+4's S = 131072, 1024 files of 32 full frames at
      multiples of the file size, 4 GiB of messages.  The contender is what a
      caller with device-resident files can do without the call: one
      mec_bitrot_sum_batch_dev over all frames (base + 32, stride 131104),
      one mec_memcpy_d2h of the digests, a host compare with the frame
      headers.  The headers are strided through the files buffer and the
      library has no strided copy, so the contender compares with a host
      copy of them made beforehand, untimed: that favours the contender.
      Its hash call is also timed on its own, which gives
      hh256_batch4_kernel's rate beside hh256_frames_verify's.
  A+1 the same files one byte further on: every chain is sheared.  No
      contender; against case A on the same frames.
  B   sheared, large: EC12+4's S = 87382, 1024 files of 48 full frames at
      64-byte-aligned offsets; the frame phases cycle 0, 6, 4, 2, so a
      quarter of the chains is aligned.  No device contender exists (the
      pitch 87414 is no multiple of 16); against case A on equal bytes.
  C   small files: 4096 one-frame files, seeded log-uniform part sizes in
      [512 B, 128 KiB], in host memory.  The contender is one
      mec_bitrot_verify_stream per file, PCIe-inclusive as the host-pointer
      variant beside it is; the device call over the same files resident in
      HBM is printed for reference.

The large cases repeat one seeded group of 64 files 16 times at different
addresses; every file verifies.  Prints median, min and max per contender
and case.  A case counts as faster or slower only where the gap between the
medians exceeds the larger of the two min-max spreads.  Needs a GPU; exits
non-zero without one.  Output of record: profiles/r11_scrub.txt.
"""
import argparse
import ctypes
import math
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import minio_amd  # noqa: E402
import oracle  # noqa: E402

lib = minio_amd._lib
HH = minio_amd.HIGHWAYHASH256S
MiB = 1 << 20
GROUP = 64  # files built on the host per large case, then repeated


def check(st):
    if st != 0:
        raise RuntimeError(f"mec status {st}: {lib.mec_last_error()}")


def i64arr(v):
    return (ctypes.c_int64 * len(v))(*v)


def build_file(part, S, seed):
    data = oracle.fill_random(part, seed)
    out = bytearray()
    for k in range(0, part, S):
        msg = data[k:k + S]
        out += oracle.bitrot_sum(HH, msg) + msg
    return np.frombuffer(bytes(out), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", type=int, default=1024,
                    help="files of the large cases, a multiple of 64")
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--case", choices=("A", "B", "C", "all"), default="all")
    args = ap.parse_args()
    if args.warm < 5 or args.iters < 30:
        ap.error("at least 5 warm and 30 timed iterations per case")
    if args.files % GROUP:
        ap.error("--files must be a multiple of 64")
    if minio_amd.device_count() == 0:
        print("bench_scrub: no GPU visible", file=sys.stderr)
        return 2

    with minio_amd.Erasure(8, 4, MiB) as e:
        ctx = e._ctx

        def alloc(size):
            ptr = ctypes.c_void_p()
            check(lib.mec_dev_alloc(ctx, max(size, 1), ctypes.byref(ptr)))
            return ptr

        def h2d(dst, off, src):
            check(lib.mec_memcpy_h2d(
                ctx, ctypes.c_void_p(dst.value + off),
                ctypes.c_char_p(src.ctypes.data), src.nbytes))

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def series(fns):
            """5 warm + 30 timed iterations, the contenders alternating."""
            tm = {k: [] for k in fns}
            for _ in range(args.warm):
                for k in fns:
                    fns[k]()
            for _ in range(args.iters):
                for k in fns:
                    tm[k].append(timed(fns[k]))
            return tm

        def report(tm, nbytes):
            med = {}
            for k, v in tm.items():
                med[k] = statistics.median(v)
                rate = (f"{nbytes[k] / med[k] / 1e9:7.3f} TB/s"
                        if nbytes.get(k) else " " * 12)
                print(f"  {k:<34s} median {med[k]:9.3f} ms   "
                      f"min {min(v):9.3f}   max {max(v):9.3f}   "
                      f"spread {max(v) - min(v):8.3f}   {rate}")
            return med

        def verdict(tm, med, a, c):
            spread = max(max(tm[k]) - min(tm[k]) for k in (a, c))
            gap = med[c] - med[a]
            word = ("faster" if gap > spread else
                    "slower" if -gap > spread else
                    "inside the larger min-max spread")
            print(f"  {a} / {c} = {med[a] / med[c]:.3f}   median gap "
                  f"{gap:+.3f} ms, larger spread {spread:.3f} ms: {word}")

        class Large:
            """files files of `frames` full frames at shard size S; file f
            at f*step + shift."""

            def __init__(self, S, frames, shift, files):
                self.S, self.frames, self.n = S, frames, files
                part = S * frames
                self.fsize = frames * (32 + S)
                self.step = (self.fsize + 63) // 64 * 64
                group = np.zeros(GROUP * self.step, dtype=np.uint8)
                for g in range(GROUP):
                    group[g * self.step:g * self.step + self.fsize] = \
                        build_file(part, S, 0x5C0 + g)
                self.group = group
                self.bytes = files * self.step + 64
                self.dev = alloc(self.bytes)
                for r in range(files // GROUP):
                    h2d(self.dev, shift + r * group.nbytes, group)
                self.off = i64arr([f * self.step + shift
                                   for f in range(files)])
                self.sizes = i64arr([self.fsize] * files)
                self.parts = i64arr([part] * files)
                self.shards = i64arr([S] * files)
                self.status = ctypes.create_string_buffer(files)
                self.fb = i64arr([0] * files)
                self.msg_bytes = files * part

            def scrub(self):
                check(lib.mec_bitrot_verify_files_dev(
                    ctx, self.n, self.dev, self.bytes, self.off, self.sizes,
                    self.parts, self.shards, HH, self.status, self.fb))

            def all_ok(self):
                return self.status.raw == bytes(self.n) and \
                    list(self.fb) == [-1] * self.n

            def free(self):
                lib.mec_dev_free(ctx, self.dev)

        print(f"HighwayHash256S batch scrub, host-clock ms around "
              f"synchronous calls, {args.iters} timed + {args.warm} warm per "
              f"contender, alternating")
        a = None
        med_a = None
        if args.case in ("A", "B", "all"):
            a = Large(131072, 32, 0, args.files)
            assert a.step == a.fsize
        if args.case in ("A", "all"):
            nfr = a.n * a.frames
            pitch = 32 + a.S
            sums = alloc(nfr * 32)
            got = np.empty(nfr * 32, dtype=np.uint8)
            # the contender's host copy of the headers, made beforehand
            hdr = np.tile(a.group.reshape(GROUP * a.frames, pitch)[:, :32]
                          .reshape(-1), a.n // GROUP)
            msgs = ctypes.c_void_p(a.dev.value + 32)
            split = []

            def contender():
                t0 = time.perf_counter()
                check(lib.mec_bitrot_sum_batch_dev(ctx, HH, nfr, msgs, a.S,
                                                   pitch, sums))
                split.append((time.perf_counter() - t0) * 1e3)
                check(lib.mec_memcpy_d2h(
                    ctx, got.ctypes.data_as(ctypes.c_char_p), sums,
                    got.nbytes))
                bad = (got.reshape(nfr, 32) != hdr.reshape(nfr, 32)).any(1)
                if bad.any():
                    raise RuntimeError("case A: the contender found bitrot")

            a1 = Large(131072, 32, 1, args.files)
            names = ("scrub call", "sum_batch_dev + d2h + compare",
                     "scrub call, files + 1 byte")
            tm = series(dict(zip(names, (a.scrub, contender, a1.scrub))))
            if not (a.all_ok() and a1.all_ok()):
                raise RuntimeError("case A: a file did not verify")
            tm["  of which mec_bitrot_sum_batch_dev"] = split[-args.iters:]
            print(f"case A: S = {a.S}, {a.n} files of {a.frames} full "
                  f"frames, {nfr} chains, {a.msg_bytes / 2**30:.3f} GiB of "
                  f"messages; TB/s over message bytes")
            med_a = report(tm, {k: a.msg_bytes for k in tm})
            verdict(tm, med_a, names[0], names[1])
            print("case A+1: the same frames, every chain sheared")
            verdict(tm, med_a, names[2], names[0])
            lib.mec_dev_free(ctx, sums)
            a1.free()
        if args.case in ("B", "all"):
            b = Large(87382, 48, 0, args.files)
            phases = sorted({(k * (32 + b.S) + 32) % 8
                             for k in range(b.frames)})
            names = ("scrub call, S = 87382", "scrub call, S = 131072")
            tm = series(dict(zip(names, (b.scrub, a.scrub))))
            if not (b.all_ok() and a.all_ok()):
                raise RuntimeError("case B: a file did not verify")
            print(f"case B: S = {b.S}, {b.n} files of {b.frames} full "
                  f"frames, {b.n * b.frames} chains at phases {phases} (a "
                  f"quarter aligned), {b.msg_bytes / 2**30:.3f} GiB of "
                  f"messages against case A's {a.msg_bytes / 2**30:.3f}; "
                  f"TB/s over message bytes")
            med = report(tm, dict(zip(names, (b.msg_bytes, a.msg_bytes))))
            verdict(tm, med, names[0], names[1])
            b.free()
        if a is not None:
            a.free()
        if args.case in ("C", "all"):
            n = args.small
            rng = random.Random(0x5C)
            lo, hi = math.log(512), math.log(131072)
            parts = [min(131072, max(512, int(math.exp(rng.uniform(lo, hi)))))
                     for _ in range(n)]
            S = 131072
            files = [build_file(pt, S, 0xC00 + i)
                     for i, pt in enumerate(parts)]
            sizes = [f.nbytes for f in files]
            plist = [f.ctypes.data_as(ctypes.c_char_p) for f in files]
            ptrs = (ctypes.c_char_p * n)(*plist)
            la, pa, sa = i64arr(sizes), i64arr(parts), i64arr([S] * n)
            status = ctypes.create_string_buffer(n)
            fb = i64arr([0] * n)
            off = minio_amd.scrub_file_offsets(sizes)
            dev = alloc(off[-1])
            for f, o in zip(files, off):
                h2d(dev, o, f)
            oa = i64arr(off[:-1])

            def host_call():
                check(lib.mec_bitrot_verify_files(ctx, n, ptrs, la, pa, sa,
                                                  HH, status, fb))

            def dev_call():
                check(lib.mec_bitrot_verify_files_dev(
                    ctx, n, dev, off[-1], oa, la, pa, sa, HH, status, fb))

            def per_file():
                for f, sz, pt in zip(plist, sizes, parts):
                    check(lib.mec_bitrot_verify_stream(ctx, f, sz, pt, HH,
                                                       None, S))

            names = ("mec_bitrot_verify_files (host)",
                     "mec_bitrot_verify_stream per file",
                     "mec_bitrot_verify_files_dev")
            tm = series(dict(zip(names, (host_call, per_file, dev_call))))
            if status.raw != bytes(n) or list(fb) != [-1] * n:
                raise RuntimeError("case C: a file did not verify")
            print(f"case C: {n} one-frame files, log-uniform part sizes in "
                  f"[512 B, 128 KiB], {sum(parts) / 2**20:.1f} MiB of "
                  f"messages; the first two from host memory "
                  f"(PCIe-inclusive), the third resident in HBM")
            med = report(tm, {})
            verdict(tm, med, names[0], names[1])
            print(f"  per file: {med[names[0]] / n * 1e3:.2f} us in the "
                  f"batch, {med[names[1]] / n * 1e3:.2f} us per "
                  f"mec_bitrot_verify_stream call")
            lib.mec_dev_free(ctx, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
