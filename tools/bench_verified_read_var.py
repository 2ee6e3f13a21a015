#!/usr/bin/env python3
"""Measure mec_verify_reconstruct_batch_var_dev against what a caller with
device-resident rows of different lengths has to do without it, on one
MI355X.

EC8+4, 1 MiB context, HighwayHash256S, seeded rows resident in HBM (encoded
and hashed on the device by mec_encode_batch_var_dev, then re-laid into the
read side's single rows buffer), a host clock around calls that end in a
stream synchronise, both contenders alternating in one process.  Cases:

  U/V1  n = 4096, all 1 MiB, healthy GET: the 8 data rows read, data_only=1.
  U/V2  n = 4096, all 1 MiB, one drive down: the 12 single-erasure positions
        round-robin, the 8 lowest surviving rows read, data_only=1.
        For both the contender is mec_verify_reconstruct_batch_dev on the
        same layout (with equal lengths the packed layout IS the uniform
        one): the difference is the cost of the tables.
  M     n = 4096, bench_encode_var.py's seeded log-uniform lengths in
        [4 KiB, 1 MiB], one drive down as in V2.
  S     n = 4096, small objects only: that tool's seeded uniform lengths in
        [1 KiB, 16 KiB], one drive down as in V2.
        For M and S the contender is one mec_verify_reconstruct_batch_dev
        per distinct length over a copy of the rows laid out at the
        context's fixed stride.  The re-layout is done once, untimed.

Every call rebuilds the same unread rows from the same survivors, so every
iteration sees the same work.  Prints median, min and max per contender and
case.  A case counts as faster or slower only where the gap between the
medians exceeds the larger of the two min-max spreads.  Needs a GPU; exits
non-zero without one.  Output of record: profiles/r7_verified_read_var.txt.
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
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--case", choices=("U", "M", "S", "all"), default="all")
    args = ap.parse_args()
    if args.warm < 5 or args.iters < 30:
        ap.error("at least 5 warm and 30 timed iterations per case")
    if minio_amd.device_count() == 0:
        print("bench_verified_read_var: no GPU visible", file=sys.stderr)
        return 2

    d, p, bs, n = 8, 4, MiB, args.n
    t = d + p
    slab = np.frombuffer(oracle.fill_random(256 << 20, 0xEC7), dtype=np.uint8)

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

        def v1_mask():
            read = np.zeros((n, t), dtype=np.uint8)
            read[:, :d] = 1
            return read

        def v2_mask():
            idx = np.arange(n)
            read = np.zeros((n, t), dtype=np.uint8)
            for i in range(t):
                alive = [s for s in range(t) if s != i][:d]
                read[np.ix_(idx[idx % t == i], alive)] = 1
            return read

        def build(lens):
            """Rows and digests of n seeded blocks in the read side's packed
            layout, and the same at the fixed stride grouped by length."""
            R = minio_amd.var_row_offsets(d, bs, lens)
            S = [-(-ln // d) for ln in lens]
            la = (ctypes.c_int64 * n)(*lens)
            data, par = alloc(d * R[-1]), alloc(p * R[-1])
            sums = alloc(n * t * 32)
            for off in range(0, d * R[-1], slab.nbytes):
                h2d(data, off, slab[:min(slab.nbytes, d * R[-1] - off)])
            check(lib.mec_encode_batch_var_dev(ctx, n, data, la, par, HH,
                                               sums))
            groups = {}
            for i, ln in enumerate(lens):
                groups.setdefault(ln, []).append(i)
            uniform = len(groups) == 1 and lens[0] == bs
            order = [i for ln in sorted(groups) for i in groups[ln]]
            slot = {i: k for k, i in enumerate(order)}
            rows = alloc(t * R[-1])
            crows = alloc(n * t * ustride)
            csums = alloc(n * t * 32)
            for i in range(n):
                st = (S[i] + 63) // 64 * 64
                img = np.concatenate([d2h(data, d * R[i], d * st),
                                      d2h(par, p * R[i], p * st)])
                h2d(rows, t * R[i], img)
                if uniform:
                    h2d(crows, slot[i] * t * ustride, img)
                else:
                    wide = np.zeros((t, ustride), dtype=np.uint8)
                    wide[:, :st] = img.reshape(t, st)
                    h2d(crows, slot[i] * t * ustride, wide)
            hsums = d2h(sums, 0, n * t * 32).reshape(n, t * 32)
            h2d(csums, 0, np.ascontiguousarray(hsums[order]))
            for ptr in (data, par):
                lib.mec_dev_free(ctx, ptr)
            return dict(lens=lens, la=la, R=R, S=S, rows=rows, sums=sums,
                        crows=crows, csums=csums, groups=groups, order=order,
                        slot=slot, uniform=uniform)

        def run_case(case, what, b, read, data_only):
            lens, S, R, slot = b["lens"], b["S"], b["R"], b["slot"]
            read_b = read.tobytes()
            pres = ctypes.create_string_buffer(n * t)
            st_new = ctypes.create_string_buffer(n)
            cpres = ctypes.create_string_buffer(n * t)
            st_old = ctypes.create_string_buffer(n)
            cread = np.ascontiguousarray(read[b["order"]])
            calls, k = [], 0
            for ln in sorted(b["groups"]):
                m = len(b["groups"][ln])
                calls.append((
                    m, ctypes.c_void_p(b["crows"].value + k * t * ustride),
                    ctypes.c_void_p(b["csums"].value + k * t * 32),
                    cread[k:k + m].tobytes(), -(-ln // d),
                    ctypes.cast(ctypes.addressof(cpres) + k * t,
                                ctypes.c_char_p),
                    ctypes.cast(ctypes.addressof(st_old) + k,
                                ctypes.c_char_p)))
                k += m

            def new():
                check(lib.mec_verify_reconstruct_batch_var_dev(
                    ctx, n, b["rows"], b["sums"], b["la"], read_b, HH,
                    data_only, 0, pres, st_new))

            def old():
                for m, pr, ps, mask, sl, po, so in calls:
                    check(lib.mec_verify_reconstruct_batch_dev(
                        ctx, m, pr, ps, mask, sl, HH, data_only, 0, po, so))

            def same_result():
                pn = np.frombuffer(pres.raw, dtype=np.uint8).reshape(n, t)
                po = np.frombuffer(cpres.raw, dtype=np.uint8).reshape(n, t)
                if not (pn[b["order"]] == po).all() or \
                        not (pn == (read != 0)).all():
                    return False
                if st_new.raw != bytes(n) or st_old.raw != bytes(n):
                    return False
                rng = random.Random(n)
                for i in [0, n - 1] + rng.sample(range(n), min(n, 30)):
                    st = (S[i] + 63) // 64 * 64
                    a = d2h(b["rows"], t * R[i], t * st).reshape(t, st)
                    c = d2h(b["crows"], slot[i] * t * ustride,
                            t * ustride).reshape(t, ustride)
                    if not (a[:, :S[i]] == c[:, :S[i]]).all():
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
            row_bytes = sum(S) * t
            print(f"case {case}: {what}")
            print(f"  n={n}, {len(b['groups'])} distinct lengths "
                  f"({len(calls)} uniform calls), valid row bytes "
                  f"{row_bytes / 2**30:.3f} GiB, packed rows "
                  f"{t * R[-1] / 2**30:.3f} GiB vs "
                  f"{n * t * ustride / 2**30:.3f} GiB at the fixed stride")
            med = {}
            for k in names:
                med[k] = statistics.median(tm[k])
                print(f"  {k:<17s} median {med[k]:9.3f} ms   "
                      f"min {min(tm[k]):9.3f}   max {max(tm[k]):9.3f}   "
                      f"spread {max(tm[k]) - min(tm[k]):8.3f}   "
                      f"({args.iters} timed, {args.warm} warm)")
            spread = max(max(v) - min(v) for v in tm.values())
            a, c = names
            gap = med[c] - med[a]
            verdict = ("faster" if gap > spread else
                       "slower" if -gap > spread else
                       "inside the larger min-max spread")
            print(f"  {a} / {c} = {med[a] / med[c]:.3f}   median gap "
                  f"{gap:+.3f} ms, larger spread {spread:.3f} ms: {verdict}")

        def free(b):
            for k in ("rows", "sums", "crows", "csums"):
                lib.mec_dev_free(ctx, b[k])

        print(f"EC{d}+{p} block {bs} HighwayHash256S n={n}, fixed stride "
              f"{ustride}, host-clock ms around synchronous calls")
        if args.case in ("U", "all"):
            b = build([bs] * n)
            run_case("U/V1", "all 1 MiB, healthy GET: 8 data rows read, "
                     "data_only=1, against mec_verify_reconstruct_batch_dev",
                     b, v1_mask(), 1)
            run_case("U/V2", "all 1 MiB, one drive down, 8 lowest survivors "
                     "read, data_only=1, against "
                     "mec_verify_reconstruct_batch_dev", b, v2_mask(), 1)
            free(b)
        if args.case in ("M", "all"):
            rng = random.Random(0x4D)
            lo, hi = math.log(4096), math.log(MiB)
            b = build([min(MiB, max(4096, int(math.exp(rng.uniform(lo, hi)))))
                       for _ in range(n)])
            run_case("M", "log-uniform lengths in [4 KiB, 1 MiB], one drive "
                     "down, 8 lowest survivors read, data_only=1", b,
                     v2_mask(), 1)
            free(b)
        if args.case in ("S", "all"):
            rng = random.Random(0x53)
            b = build([rng.randint(1024, 16384) for _ in range(n)])
            run_case("S", "uniform lengths in [1 KiB, 16 KiB], one drive "
                     "down, 8 lowest survivors read, data_only=1", b,
                     v2_mask(), 1)
            free(b)
    return 0


if __name__ == "__main__":
    sys.exit(main())
