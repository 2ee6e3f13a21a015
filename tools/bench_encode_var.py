#!/usr/bin/env python3
"""Measure mec_encode_batch_var_dev against what a caller with
device-resident blocks of different lengths has to do without it, on one
MI355X.

EC8+4, 1 MiB context, HighwayHash256S, seeded inputs resident in HBM, a
host clock around calls that end in a stream synchronise, both contenders
alternating in one process.  Three cases:

  U  n = 1024, all 1 MiB.  The contender is mec_encode_batch_dev on the
     same data buffer (with equal lengths the packed layout IS the uniform
     one).
  M  n = 4096, seeded log-uniform lengths in [4 KiB, 1 MiB].
  S  n = 16384, seeded uniform lengths in [1 KiB, 16 KiB].

For M and S the contender is one mec_encode_batch_dev_async per distinct
length over a copy of the rows laid out at the context's fixed stride, then
one mec_stream_sync.  The re-layout is done once, untimed.

Prints median, min and max per contender and case, GiB/s of input bytes,
and the planner's host time on its own (the pure-host row-offset call, which
runs the same planner).  A case counts as faster or slower only where the
gap between the medians exceeds the larger of the two min-max spreads.
Needs a GPU; exits non-zero without one.  Output of record:
profiles/r5_encode_var.txt.
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


def check(st):
    if st != 0:
        raise RuntimeError(f"mec status {st}: {lib.mec_last_error()}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--case", choices=("U", "M", "S", "all"), default="all")
    args = ap.parse_args()
    if args.warm < 5 or args.iters < 30:
        ap.error("at least 5 warm and 30 timed iterations per case")
    if minio_amd.device_count() == 0:
        print("bench_encode_var: no GPU visible", file=sys.stderr)
        return 2

    d, p, bs = 8, 4, MiB
    t = d + p
    slab = np.frombuffer(oracle.fill_random(256 << 20, 0xEC5), dtype=np.uint8)

    with minio_amd.Erasure(d, p, bs) as e:
        ctx = e._ctx
        ustride = lib.mec_shard_stride(bs, d)

        def alloc(size):
            ptr = ctypes.c_void_p()
            check(lib.mec_dev_alloc(ctx, max(size, 1), ctypes.byref(ptr)))
            return ptr

        def h2d(dst, off, src):
            check(lib.mec_memcpy_h2d(
                ctx, ctypes.c_void_p(dst.value + off),
                ctypes.c_char_p(src.ctypes.data), src.nbytes))

        def d2h(src, off, size):
            out = np.empty(size, dtype=np.uint8)
            check(lib.mec_memcpy_d2h(
                ctx, out.ctypes.data_as(ctypes.c_char_p),
                ctypes.c_void_p(src.value + off), size))
            return out

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def run_case(case, what, lens):
            n = len(lens)
            R = minio_amd.var_row_offsets(d, bs, lens)
            S = [-(-ln // d) for ln in lens]
            in_bytes = sum(lens)
            la = (ctypes.c_int64 * n)(*lens)
            # packed input: seeded bytes everywhere (the rows' zero padding
            # is the caller's business and does not change the work)
            data = alloc(d * R[-1])
            for off in range(0, d * R[-1], slab.nbytes):
                h2d(data, off, slab[:min(slab.nbytes, d * R[-1] - off)])
            par = alloc(p * R[-1])
            sums = alloc(n * t * 32)

            # contender: items grouped by length, each group at the fixed
            # stride in its own slice of one allocation
            groups = {}
            for i, ln in enumerate(lens):
                groups.setdefault(ln, []).append(i)
            uniform = len(groups) == 1 and lens[0] == bs
            if uniform:
                cdata, slot = data, {i: i for i in range(n)}
            else:
                cdata, slot, k = alloc(n * d * ustride), {}, 0
                for ln in sorted(groups):
                    for i in groups[ln]:
                        slot[i] = k
                        k += 1
                for i in range(n):
                    st = (S[i] + 63) // 64 * 64
                    img = d2h(data, d * R[i], d * st).reshape(d, st)
                    for r in range(d):
                        h2d(cdata, (slot[i] * d + r) * ustride,
                            np.ascontiguousarray(img[r, :S[i]]))
            cpar = alloc(n * p * ustride)
            csums = alloc(n * t * 32)
            calls, k = [], 0
            for ln in sorted(groups):
                m = len(groups[ln])
                calls.append((m, ctypes.c_void_p(cdata.value + k * d * ustride),
                              ln, ctypes.c_void_p(cpar.value + k * p * ustride),
                              ctypes.c_void_p(csums.value + k * t * 32)))
                k += m

            def new():
                check(lib.mec_encode_batch_var_dev(ctx, n, data, la, par, HH,
                                                   sums))

            def old():
                if uniform:
                    check(lib.mec_encode_batch_dev(ctx, n, cdata, bs, cpar,
                                                   HH, csums))
                    return
                for m, pd, ln, pp, ps in calls:
                    check(lib.mec_encode_batch_dev_async(ctx, m, pd, ln, pp,
                                                         HH, ps))
                check(lib.mec_stream_sync(ctx))

            row_off = (ctypes.c_int64 * (n + 1))()

            def plan():
                check(lib.mec_var_row_offsets(d, bs, n, la, row_off))

            def same_result():
                rng = random.Random(n)
                for i in [0, n - 1] + rng.sample(range(n), min(n, 30)):
                    st = (S[i] + 63) // 64 * 64
                    a = d2h(par, p * R[i], p * st).reshape(p, st)[:, :S[i]]
                    b = d2h(cpar, slot[i] * p * ustride,
                            p * ustride).reshape(p, ustride)[:, :S[i]]
                    if not (a == b).all():
                        return False
                    if not (d2h(sums, i * t * 32, t * 32) ==
                            d2h(csums, slot[i] * t * 32, t * 32)).all():
                        return False
                return True

            names = ("per-item lengths", "per-length calls")
            fns = dict(zip(names, (new, old)))
            tm = {k: [] for k in names}
            for _ in range(args.warm):
                for k in names:
                    fns[k]()
            if not same_result():
                raise RuntimeError(f"case {case}: the two paths disagree")
            for _ in range(args.iters):
                for k in names:
                    tm[k].append(timed(fns[k]))
            tp = [timed(plan) for _ in range(args.warm + args.iters)][args.warm:]
            print(f"case {case}: {what}")
            print(f"  n={n}, {len(groups)} distinct lengths, input "
                  f"{in_bytes / 2**30:.3f} GiB, packed rows "
                  f"{d * R[-1] / 2**30:.3f} GiB vs "
                  f"{n * d * ustride / 2**30:.3f} GiB at the fixed stride")
            med = {}
            for k in names:
                med[k] = statistics.median(tm[k])
                print(f"  {k:<17s} median {med[k]:9.3f} ms   "
                      f"min {min(tm[k]):9.3f}   max {max(tm[k]):9.3f}   "
                      f"spread {max(tm[k]) - min(tm[k]):8.3f}   "
                      f"{in_bytes / 2**30 / (med[k] * 1e-3):8.1f} GiB/s input"
                      f"   ({args.iters} timed, {args.warm} warm)")
            print(f"  planner alone     median "
                  f"{statistics.median(tp):9.3f} ms   min {min(tp):9.3f}   "
                  f"max {max(tp):9.3f}   (host only, included in the "
                  f"per-item call above)")
            spread = max(max(v) - min(v) for v in tm.values())
            a, b = names
            gap = med[b] - med[a]
            verdict = ("faster" if gap > spread else
                       "slower" if -gap > spread else "no difference")
            print(f"  {a} / {b} = {med[a] / med[b]:.3f}   median gap "
                  f"{gap:+.3f} ms, larger spread {spread:.3f} ms: {verdict}")
            for ptr in {data.value, par.value, sums.value, cdata.value,
                        cpar.value, csums.value}:
                lib.mec_dev_free(ctx, ctypes.c_void_p(ptr))

        print(f"EC{d}+{p} block {bs} HighwayHash256S, fixed stride {ustride},"
              f" host-clock ms around calls that end in a synchronise")
        if args.case in ("U", "all"):
            run_case("U", "all 1 MiB, against mec_encode_batch_dev",
                     [bs] * 1024)
        if args.case in ("M", "all"):
            rng = random.Random(0x4D)
            lo, hi = math.log(4096), math.log(MiB)
            run_case("M", "log-uniform lengths in [4 KiB, 1 MiB]",
                     [min(MiB, max(4096, int(math.exp(rng.uniform(lo, hi)))))
                      for _ in range(4096)])
        if args.case in ("S", "all"):
            rng = random.Random(0x53)
            run_case("S", "uniform lengths in [1 KiB, 16 KiB]",
                     [rng.randint(1024, 16384) for _ in range(16384)])
    return 0


if __name__ == "__main__":
    sys.exit(main())
