#!/usr/bin/env python3
"""Measure mec_reconstruct_batch_mixed_dev_async against the uniform
mec_reconstruct_batch_dev_async on one MI355X.

EC8+4 / 1 MiB blocks, n=4096 items resident in HBM (seeded bytes), device
events on the context's stream (mec_timer_start/stop), both contenders
alternating in one process.  Three cases:

  A  one 3-erased mask (bench.py's decode workload), data_only=1:
     uniform call vs mixed call.
  B  one drive down: the 12 single-erasure masks round-robin, data_only=0.
     Mixed call vs the uniform API used as a caller must use it today:
     one async call per mask over a copy pre-sorted into contiguous
     buckets, then one sync.  The sort is not timed.
  C  all 220 three-erasure masks, seeded shuffle, data_only=1.  Same
     contender, 220 calls.

Prints median and min-max per contender and case.  Needs a GPU; exits
non-zero without one.  Output of record: profiles/r3_reconstruct_mixed.txt.
"""
import argparse
import ctypes
import itertools
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import minio_amd  # noqa: E402
import oracle  # noqa: E402

lib = minio_amd._lib


def check(st):
    if st != 0:
        raise RuntimeError(f"mec status {st}: {lib.mec_last_error()}")


def erasure_masks(total, k):
    out = []
    for gone in itertools.combinations(range(total), k):
        out.append(bytes(0 if s in gone else 1 for s in range(total)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    if args.warm < 5 or args.iters < 30:
        ap.error("at least 5 warm and 30 timed iterations per case")
    if minio_amd.device_count() == 0:
        print("bench_reconstruct_mixed: no GPU visible", file=sys.stderr)
        return 2

    d, p, bs, n = 8, 4, 1 << 20, args.n
    total = d + p
    with minio_amd.Erasure(d, p, bs) as e:
        ctx = e._ctx
        S, stride = e.shard_size(), lib.mec_shard_stride(bs, d)
        item = total * stride
        nbytes = n * item

        def alloc_filled(seed):
            ptr = ctypes.c_void_p()
            check(lib.mec_dev_alloc(ctx, nbytes, ctypes.byref(ptr)))
            slab = oracle.fill_random(min(nbytes, 256 << 20), seed)
            for off in range(0, nbytes, len(slab)):
                m = min(len(slab), nbytes - off)
                check(lib.mec_memcpy_h2d(
                    ctx, ctypes.c_void_p(ptr.value + off), slab, m))
            return ptr

        buf_mixed = alloc_filled(0xEC)
        buf_other = alloc_filled(0xEC)

        def timed(fn):
            ms = ctypes.c_float()
            check(lib.mec_timer_start(ctx))
            fn()
            check(lib.mec_timer_stop(ctx, ctypes.byref(ms)))
            return ms.value

        def mixed_call(present_all, data_only):
            def run():
                check(lib.mec_reconstruct_batch_mixed_dev_async(
                    ctx, n, buf_mixed, present_all, S, data_only, None))
            return run

        def bucketed_loop(item_masks, data_only):
            """The parent API: items pre-sorted by mask into contiguous
            buckets of buf_other, one uniform async call per bucket."""
            counts = {}
            for m in item_masks:
                counts[m] = counts.get(m, 0) + 1
            buckets, first = [], 0
            for m, c in counts.items():
                buckets.append(
                    (m, ctypes.c_void_p(buf_other.value + first * item), c))
                first += c

            def run():
                for m, ptr, c in buckets:
                    check(lib.mec_reconstruct_batch_dev_async(
                        ctx, c, ptr, m, S, data_only))
            return run, len(buckets)

        def report(case, what, names, fns):
            t = {k: [] for k in names}
            for _ in range(args.warm):
                for k in names:
                    timed(fns[k])
            for _ in range(args.iters):
                for k in names:
                    t[k].append(timed(fns[k]))
            print(f"case {case}: {what}")
            med = {}
            for k in names:
                med[k] = statistics.median(t[k])
                print(f"  {k:<28s} median {med[k]:8.3f} ms   "
                      f"min {min(t[k]):8.3f}   max {max(t[k]):8.3f}   "
                      f"spread {max(t[k]) - min(t[k]):7.3f}   "
                      f"({args.iters} timed, {args.warm} warm)")
            spread = max(max(v) - min(v) for v in t.values())
            a, b = names
            print(f"  {a} / {b} = {med[a] / med[b]:.3f}   "
                  f"median gap {med[b] - med[a]:+.3f} ms, "
                  f"larger spread {spread:.3f} ms")
            return med, spread

        print(f"EC{d}+{p} block {bs} n={n} shard_len={S} stride={stride} "
              f"({nbytes / 2**30:.2f} GiB per buffer), device-event ms")

        # A: one mask, both calls
        mask_a = bytes([0] * 3 + [1] * (total - 3))
        report("A", "one 3-erased mask, data_only=1",
               ("mixed", "uniform"),
               {"mixed": mixed_call(mask_a * n, 1),
                "uniform": lambda: check(lib.mec_reconstruct_batch_dev_async(
                    ctx, n, buf_other, mask_a, S, 1))})

        # B: one drive down
        ones = erasure_masks(total, 1)
        masks_b = [ones[i % len(ones)] for i in range(n)]
        loop_b, nb = bucketed_loop(masks_b, 0)
        med, spread = report(
            "B", f"12 single-erasure masks round-robin, data_only=0 "
            f"(bucketed loop = {nb} uniform calls)",
            ("mixed", "bucketed loop"),
            {"mixed": mixed_call(b"".join(masks_b), 0), "bucketed loop": loop_b})
        ok_b = med["bucketed loop"] - med["mixed"] > spread

        # C: every 3-erasure mask
        threes = erasure_masks(total, 3)
        rng = random.Random(220)
        masks_c = [threes[i % len(threes)] for i in range(n)]
        rng.shuffle(masks_c)
        loop_c, nc = bucketed_loop(masks_c, 1)
        med, spread = report(
            "C", f"220 three-erasure masks shuffled, data_only=1 "
            f"(bucketed loop = {nc} uniform calls)",
            ("mixed", "bucketed loop"),
            {"mixed": mixed_call(b"".join(masks_c), 1), "bucketed loop": loop_c})
        ok_c = med["bucketed loop"] - med["mixed"] > spread

        check(lib.mec_stream_sync(ctx))
        lib.mec_dev_free(ctx, buf_mixed)
        lib.mec_dev_free(ctx, buf_other)
    print(f"acceptance (mixed median below bucketed-loop median by more than "
          f"the larger spread): B {'met' if ok_b else 'NOT met'}, "
          f"C {'met' if ok_c else 'NOT met'}")
    return 0 if ok_b and ok_c else 1


if __name__ == "__main__":
    sys.exit(main())
