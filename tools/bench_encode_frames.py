#!/usr/bin/env python3
"""Measure mec_encode_frames_batch_var* (batch encode straight into on-disk
[hash||shard] frames) against what the library could do before it, on one
MI355X.

EC8+4, 1 MiB context, HighwayHash256S, seeded inputs, a host clock around
calls that end in a stream synchronise, the contenders alternating in one
process.  Cases U, M and S are tools/bench_encode_var.py's length sets with
the input resident in HBM:

  U  n = 1024, all 1 MiB.
  M  n = 4096, seeded log-uniform lengths in [4 KiB, 1 MiB].
  S  n = 16384, seeded uniform lengths in [1 KiB, 16 KiB].

There the contenders are mec_encode_frames_batch_var_dev and
mec_encode_batch_var_dev alone on the same input: parity at a stride and a
digest table, which no drive stores.  The gap between the two medians is the
price of framing, and the pack kernel's implied rate is its
2*(d+p)*sum(S_i) + 64*n*(d+p) bytes over that gap.

  C  host pointers, PCIe included: case M's 4096 lengths as 4096 one-block
     objects, one mec_encode_frames_batch_var call against one
     mec_encode_stream call per object.

Prints median, min and max per contender and case.  A case counts as faster
or slower only where the gap between the medians exceeds the larger of the
two min-max spreads.  Needs a GPU; exits non-zero without one.  Output of
record: profiles/r12_encode_frames.txt.
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


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def report(names, tm, in_bytes, args):
    med = {}
    for k in names:
        med[k] = statistics.median(tm[k])
        print(f"  {k:<24s} median {med[k]:9.3f} ms   "
              f"min {min(tm[k]):9.3f}   max {max(tm[k]):9.3f}   "
              f"spread {max(tm[k]) - min(tm[k]):8.3f}   "
              f"{in_bytes / 2**30 / (med[k] * 1e-3):8.1f} GiB/s input"
              f"   ({args.iters} timed, {args.warm} warm)")
    spread = max(max(v) - min(v) for v in tm.values())
    a, b = names
    gap = med[b] - med[a]
    verdict = ("faster" if gap > spread else
               "slower" if -gap > spread else "no difference")
    print(f"  {a} / {b} = {med[a] / med[b]:.3f}   median gap "
          f"{gap:+.3f} ms, larger spread {spread:.3f} ms: {verdict}")
    return med, spread


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--case", choices=("U", "M", "S", "C", "all"),
                    default="all")
    args = ap.parse_args()
    if args.warm < 5 or args.iters < 30:
        ap.error("at least 5 warm and 30 timed iterations per case")
    if minio_amd.device_count() == 0:
        print("bench_encode_frames: no GPU visible", file=sys.stderr)
        return 2

    d, p, bs = 8, 4, MiB
    t = d + p
    slab = np.frombuffer(oracle.fill_random(256 << 20, 0xEC5), dtype=np.uint8)

    with minio_amd.Erasure(d, p, bs) as e:
        ctx = e._ctx

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

        def run_dev_case(case, what, lens):
            n = len(lens)
            R = minio_amd.var_row_offsets(d, bs, lens)
            F = minio_amd.frame_offsets(d, bs, lens)
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
            frames = alloc(t * F[-1])

            def framed():
                check(lib.mec_encode_frames_batch_var_dev(ctx, n, data, la,
                                                          frames, HH))

            def rows():
                check(lib.mec_encode_batch_var_dev(ctx, n, data, la, par, HH,
                                                   sums))

            def same_result():
                rng = random.Random(n)
                for i in [0, n - 1] + rng.sample(range(n), min(n, 30)):
                    st = (S[i] + 63) // 64 * 64
                    dr = d2h(data, d * R[i], d * st).reshape(d, st)[:, :S[i]]
                    pr = d2h(par, p * R[i], p * st).reshape(p, st)[:, :S[i]]
                    dig = d2h(sums, i * t * 32, t * 32).reshape(t, 32)
                    for s in range(t):
                        fr = d2h(frames, s * F[-1] + F[i], 32 + S[i])
                        row = dr[s] if s < d else pr[s - d]
                        if not ((fr[:32] == dig[s]).all() and
                                (fr[32:] == row).all()):
                            return False
                return True

            names = ("frames", "rows + digest table")
            fns = dict(zip(names, (framed, rows)))
            tm = {k: [] for k in names}
            for _ in range(args.warm):
                for k in names:
                    fns[k]()
            if not same_result():
                raise RuntimeError(f"case {case}: the two paths disagree")
            for _ in range(args.iters):
                for k in names:
                    tm[k].append(timed(fns[k]))
            print(f"case {case}: {what}")
            print(f"  n={n}, input {in_bytes / 2**30:.3f} GiB, packed rows "
                  f"{d * R[-1] / 2**30:.3f} GiB, frames "
                  f"{t * F[-1] / 2**30:.3f} GiB")
            med, spread = report(names, tm, in_bytes, args)
            gap = med[names[0]] - med[names[1]]
            moved = 2 * t * sum(S) + 64 * n * t
            if gap > spread:
                print(f"  price of framing {gap:.3f} ms = "
                      f"{100 * gap / med[names[1]]:.1f}% of the encode; pack "
                      f"kernel implied {moved / (gap * 1e-3) / 1e12:.2f} TB/s "
                      f"over {moved / 2**30:.3f} GiB read + written")
            else:
                print(f"  price of framing {gap:+.3f} ms is inside the "
                      f"spread: no implied rate")
            for ptr in (data, par, sums, frames):
                lib.mec_dev_free(ctx, ptr)

        def run_host_case(lens):
            n = len(lens)
            F = minio_amd.frame_offsets(d, bs, lens)
            in_bytes = sum(lens)
            la = (ctypes.c_int64 * n)(*lens)
            reps = -(-in_bytes // slab.nbytes)
            blob = np.tile(slab, reps)[:in_bytes].tobytes()
            starts = [0]
            for ln in lens:
                starts.append(starts[-1] + ln)
            out = np.empty(t * F[-1], dtype=np.uint8)
            fmax = 32 + -(-bs // d)
            drives = [ctypes.create_string_buffer(fmax) for _ in range(t)]
            arr = (ctypes.c_char_p * t)(*[
                ctypes.cast(b, ctypes.c_char_p) for b in drives])
            view = memoryview(blob)
            objs = [bytes(view[starts[i]:starts[i + 1]]) for i in range(n)]

            def batch():
                check(lib.mec_encode_frames_batch_var(
                    ctx, n, blob, la,
                    out.ctypes.data_as(ctypes.c_char_p), HH))

            def per_object():
                for i in range(n):
                    check(lib.mec_encode_stream(ctx, objs[i], lens[i], HH,
                                                arr, None))

            def same_result():
                rng = random.Random(n)
                for i in [0, n - 1] + rng.sample(range(n), 30):
                    check(lib.mec_encode_stream(ctx, objs[i], lens[i], HH,
                                                arr, None))
                    for s in range(t):
                        lo = s * F[-1] + F[i]
                        want = drives[s].raw[:F[i + 1] - F[i]]
                        if out[lo:lo + len(want)].tobytes() != want:
                            return False
                return True

            names = ("one frames call", "encode_stream per object")
            fns = dict(zip(names, (batch, per_object)))
            tm = {k: [] for k in names}
            for _ in range(args.warm):
                for k in names:
                    fns[k]()
            if not same_result():
                raise RuntimeError("case C: the two paths disagree")
            for _ in range(args.iters):
                for k in names:
                    tm[k].append(timed(fns[k]))
            print("case C: host pointers, PCIe included, 4096 one-block "
                  "objects, log-uniform lengths in [4 KiB, 1 MiB]")
            print(f"  n={n}, input {in_bytes / 2**30:.3f} GiB, frames "
                  f"{t * F[-1] / 2**30:.3f} GiB")
            med, _ = report(names, tm, in_bytes, args)
            for k in names:
                print(f"  {k:<24s} {med[k] * 1e3 / n:9.2f} us per object")

        print(f"EC{d}+{p} block {bs} HighwayHash256S, host-clock ms around "
              f"calls that end in a synchronise")
        rng = random.Random(0x4D)
        lo, hi = math.log(4096), math.log(MiB)
        m_lens = [min(MiB, max(4096, int(math.exp(rng.uniform(lo, hi)))))
                  for _ in range(4096)]
        if args.case in ("U", "all"):
            run_dev_case("U", "all 1 MiB", [bs] * 1024)
        if args.case in ("M", "all"):
            run_dev_case("M", "log-uniform lengths in [4 KiB, 1 MiB]", m_lens)
        if args.case in ("S", "all"):
            rng = random.Random(0x53)
            run_dev_case("S", "uniform lengths in [1 KiB, 16 KiB]",
                         [rng.randint(1024, 16384) for _ in range(16384)])
        if args.case in ("C", "all"):
            run_host_case(m_lens)
    return 0


if __name__ == "__main__":
    sys.exit(main())
