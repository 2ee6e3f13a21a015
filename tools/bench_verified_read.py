#!/usr/bin/env python3
"""Measure mec_verify_reconstruct_batch_dev against what a caller with
device-resident shards has to do without it, on one MI355X.

EC8+4 / 1 MiB blocks, n=4096 items resident in HBM (seeded bytes, digests
computed on the device), a host clock around calls that end in a stream
synchronise (the contender includes host work), both contenders alternating
in one process.  The contender is the composition of the existing calls:

  1. mec_bitrot_sum_batch_dev over all n*12 rows,
  2. mec_memcpy_d2h of the digests,
  3. a host compare that builds the present mask,
  4. mec_reconstruct_batch_mixed_dev,
  5. (heal only) a second mec_bitrot_sum_batch_dev for the fresh digests.

Three cases:

  V1  healthy GET: the 8 data rows read, nothing corrupt, data_only=1.
  V2  one drive down: the 12 single-erasure positions round-robin, the 8
      lowest surviving rows read, data_only=1.
  V3  heal: one drive down, all 11 survivors read, one corrupt row in 1% of
      the items (seeded), data_only=0, rehash=1.

The expected digests are restored before every call, untimed, so every
iteration sees the same damage.  Prints median and min-max per contender
and case.  Needs a GPU; exits non-zero without one.  Output of record:
profiles/r4_verified_read.txt.
"""
import argparse
import ctypes
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


def check(st):
    if st != 0:
        raise RuntimeError(f"mec status {st}: {lib.mec_last_error()}")


def cptr(a):
    return a.ctypes.data_as(ctypes.c_char_p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--case", choices=("V1", "V2", "V3", "all"),
                    default="all")
    args = ap.parse_args()
    if args.warm < 5 or args.iters < 30:
        ap.error("at least 5 warm and 30 timed iterations per case")
    if minio_amd.device_count() == 0:
        print("bench_verified_read: no GPU visible", file=sys.stderr)
        return 2

    d, p, bs, n = 8, 4, 1 << 20, args.n
    total = d + p
    rows_n = n * total
    with minio_amd.Erasure(d, p, bs) as e:
        ctx = e._ctx
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        item = total * stride
        nbytes = n * item

        def alloc(size):
            ptr = ctypes.c_void_p()
            check(lib.mec_dev_alloc(ctx, size, ctypes.byref(ptr)))
            return ptr

        def alloc_filled(seed):
            ptr = alloc(nbytes)
            slab = oracle.fill_random(min(nbytes, 256 << 20), seed)
            for off in range(0, nbytes, len(slab)):
                m = min(len(slab), nbytes - off)
                check(lib.mec_memcpy_h2d(
                    ctx, ctypes.c_void_p(ptr.value + off), slab, m))
            return ptr

        buf_new = alloc_filled(0xEC)
        buf_old = alloc_filled(0xEC)
        sums_new = alloc(rows_n * 32)   # expected digests, new call
        sums_old = alloc(rows_n * 32)   # composition: rehash target
        scratch = alloc(rows_n * 32)    # composition: digests of all rows

        # digests of the seeded rows, from the device
        good = np.empty((n, total, 32), dtype=np.uint8)
        check(lib.mec_bitrot_sum_batch_dev(ctx, HH, rows_n, buf_new, S,
                                           stride, scratch))
        check(lib.mec_memcpy_d2h(ctx, cptr(good), scratch, good.nbytes))
        row0 = ctypes.create_string_buffer(S)
        check(lib.mec_memcpy_d2h(ctx, row0, buf_new, S))
        if bytes(good[0, 0]) != oracle.bitrot_sum(HH, row0.raw):
            raise RuntimeError("device digest of row 0 differs from oracle")

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def make_case(read, want, data_only, rehash):
            """read: (n, total) uint8; want: expected digests per row."""
            read_b = read.tobytes()
            readb = read != 0
            pres_new = ctypes.create_string_buffer(rows_n)
            st_new = ctypes.create_string_buffer(n)
            st_old = ctypes.create_string_buffer(n)
            got = np.empty((n, total, 32), dtype=np.uint8)
            last = {}

            def reset():
                check(lib.mec_memcpy_h2d(ctx, sums_new, cptr(want),
                                         want.nbytes))
                check(lib.mec_memcpy_h2d(ctx, sums_old, cptr(want),
                                         want.nbytes))

            def new():
                check(lib.mec_verify_reconstruct_batch_dev(
                    ctx, n, buf_new, sums_new, read_b, S, HH, data_only,
                    rehash, pres_new, st_new))

            def composition():
                check(lib.mec_bitrot_sum_batch_dev(ctx, HH, rows_n, buf_old,
                                                   S, stride, scratch))
                check(lib.mec_memcpy_d2h(ctx, cptr(got), scratch, got.nbytes))
                present = (readb & (got == want).all(axis=2)).astype(np.uint8)
                check(lib.mec_reconstruct_batch_mixed_dev(
                    ctx, n, buf_old, present.tobytes(), S, data_only, st_old))
                if rehash:
                    check(lib.mec_bitrot_sum_batch_dev(
                        ctx, HH, rows_n, buf_old, S, stride, sums_old))
                last["present"] = present

            def same_result():
                pn = np.frombuffer(pres_new.raw, dtype=np.uint8)
                if not (pn.reshape(n, total) == last["present"]).all():
                    return False
                if st_new.raw != st_old.raw:
                    return False
                a = ctypes.create_string_buffer(item)
                b = ctypes.create_string_buffer(item)
                for i in (0, 1, n // 2, n - 1):
                    check(lib.mec_memcpy_d2h(
                        ctx, a, ctypes.c_void_p(buf_new.value + i * item),
                        item))
                    check(lib.mec_memcpy_d2h(
                        ctx, b, ctypes.c_void_p(buf_old.value + i * item),
                        item))
                    if a.raw != b.raw:
                        return False
                return True

            return reset, {"verified read": new,
                           "composition": composition}, same_result

        def report(case, what, reset, fns, same_result):
            names = ("verified read", "composition")
            t = {k: [] for k in names}
            for _ in range(args.warm):
                for k in names:
                    reset()
                    fns[k]()
            if not same_result():
                raise RuntimeError(f"case {case}: the two paths disagree")
            for _ in range(args.iters):
                for k in names:
                    reset()
                    t[k].append(timed(fns[k]))
            print(f"case {case}: {what}")
            med = {}
            for k in names:
                med[k] = statistics.median(t[k])
                print(f"  {k:<16s} median {med[k]:8.3f} ms   "
                      f"min {min(t[k]):8.3f}   max {max(t[k]):8.3f}   "
                      f"spread {max(t[k]) - min(t[k]):7.3f}   "
                      f"({args.iters} timed, {args.warm} warm)")
            spread = max(max(v) - min(v) for v in t.values())
            a, b = names
            print(f"  {a} / {b} = {med[a] / med[b]:.3f}   "
                  f"median gap {med[b] - med[a]:+.3f} ms, "
                  f"larger spread {spread:.3f} ms")
            return med[b] - med[a] > spread

        print(f"EC{d}+{p} block {bs} n={n} shard_len={S} stride={stride} "
              f"({nbytes / 2**30:.2f} GiB per buffer), host-clock ms around "
              f"synchronous calls")
        idx = np.arange(n)
        met = {}

        if args.case in ("V1", "all"):
            read = np.zeros((n, total), dtype=np.uint8)
            read[:, :d] = 1
            met["V1"] = report(
                "V1", "healthy GET: 8 data rows read, data_only=1 "
                f"(hashes {n * d} of {rows_n} rows)",
                *make_case(read, good, 1, 0))

        if args.case in ("V2", "all"):
            read = np.zeros((n, total), dtype=np.uint8)
            for i in range(total):
                alive = [s for s in range(total) if s != i][:d]
                read[np.ix_(idx[idx % total == i], alive)] = 1
            met["V2"] = report(
                "V2", "one drive down, 8 lowest survivors read, data_only=1",
                *make_case(read, good, 1, 0))

        if args.case in ("V3", "all"):
            read = np.ones((n, total), dtype=np.uint8)
            read[idx, idx % total] = 0
            want = good.copy()
            rng = random.Random(0xB17)
            hit = rng.sample(range(n), max(1, n // 100))
            for i in hit:
                s = rng.choice([s for s in range(total) if s != i % total])
                want[i, s, rng.randrange(32)] ^= 1 << rng.randrange(8)
            met["V3"] = report(
                "V3", f"heal: one drive down, 11 survivors read, corrupt row "
                f"in {len(hit)} items, data_only=0, rehash=1",
                *make_case(read, want, 0, 1))

        for ptr in (buf_new, buf_old, sums_new, sums_old, scratch):
            lib.mec_dev_free(ctx, ptr)
    print("acceptance (verified-read median below the composition's median "
          "by more than the larger spread): " +
          ", ".join(f"{k} {'met' if v else 'NOT met'}"
                    for k, v in met.items()))
    return 0 if all(met.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
