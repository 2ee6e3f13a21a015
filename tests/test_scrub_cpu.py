"""CPU-side checks of the batch scrub (mec_bitrot_verify_files*): the host
planner, exercised by the stand-alone sanitised program
tools/scrub_plan_check.cpp, the offsets helper, and the null-context check
of the two entry points.  Nothing here needs a GPU, and nothing sanitised is
loaded into Python: the planner check runs in its own process."""
import ctypes
import os
import subprocess

import pytest

import minio_amd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "minio_amd", "csrc")


def test_planner_sanitised_program(tmp_path):
    """Every frame of every size-consistent file is in exactly one chain
    list, split by its message address modulo 8; each list is in descending
    length order with ties in ascending (file, frame) order; the early
    verdicts; the reduction, with two bad frames of one file giving the
    lower index; a refusal for each argument error, the 32-bit frame bound
    through an injected limit.  The checks live in
    tools/scrub_plan_check.cpp."""
    exe = str(tmp_path / "scrub_plan_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", CSRC,
         os.path.join(REPO, "tools", "scrub_plan_check.cpp"),
         os.path.join(CSRC, "scrub_plan.cpp"),
         "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    for line in ("small: ok", "offsets: ok",
                 "random a: n=400 aligned=661 sheared=4601 bad=549 ok",
                 "random b: n=1500", "random c: n=1", "refusals: ok"):
        assert line in r.stdout, r.stdout


def test_planner_has_no_hip_dependency():
    """The planner is a host-only translation unit beside var_plan.cpp."""
    for name in ("scrub_plan.cpp", "scrub_plan.h"):
        incs = [ln for ln in open(os.path.join(CSRC, name))
                if ln.lstrip().startswith("#include")]
        assert incs and not any("hip" in ln or "kernels.h" in ln
                                for ln in incs), (name, incs)


def test_scrub_file_offsets():
    """mec_scrub_file_offsets against its definition: F_0 = 0,
    F_{f+1} = F_f + align64(size_f)."""
    sizes = [0, 1, 63, 64, 65, 87414, 131104 * 32, 40 + 32, 2 ** 40 + 1]
    want = [0]
    for s in sizes:
        want.append(want[-1] + (s + 63) // 64 * 64)
    assert minio_amd.scrub_file_offsets(sizes) == want
    assert minio_amd.scrub_file_offsets([7]) == [0, 64]


def test_scrub_file_offsets_refusals():
    lib = minio_amd._lib
    out = (ctypes.c_int64 * 4)(*[-5] * 4)
    ok = (ctypes.c_int64 * 3)(1, 2, 3)
    assert lib.mec_scrub_file_offsets(0, ok, out) == 6
    assert lib.mec_scrub_file_offsets(-1, ok, out) == 6
    assert lib.mec_scrub_file_offsets(3, None, out) == 6
    assert lib.mec_scrub_file_offsets(3, ok, None) == 6
    neg = (ctypes.c_int64 * 3)(1, -2, 3)
    assert lib.mec_scrub_file_offsets(3, neg, out) == 6
    big = (ctypes.c_int64 * 3)(2 ** 62, 2 ** 62, 2 ** 62)
    assert lib.mec_scrub_file_offsets(3, big, out) == 6
    assert list(out) == [-5] * 4, "a refusal wrote offsets"
    for bad in ([], [4, -1]):
        with pytest.raises(minio_amd.MecError) as ei:
            minio_amd.scrub_file_offsets(bad)
        assert ei.value.status == 6


def test_null_ctx_is_invalid_arg():
    lib = minio_amd._lib
    one = (ctypes.c_int64 * 1)
    off, size, part, shard = one(0), one(72), one(40), one(64)
    status = ctypes.create_string_buffer(b"\x77", 1)
    fb = one(-9)
    buf = ctypes.create_string_buffer(72)
    assert lib.mec_bitrot_verify_files_dev(
        None, 1, ctypes.cast(buf, ctypes.c_void_p), 72, off, size, part,
        shard, minio_amd.HIGHWAYHASH256S, status, fb) == 6
    ptrs = (ctypes.c_char_p * 1)(ctypes.cast(buf, ctypes.c_char_p))
    assert lib.mec_bitrot_verify_files(
        None, 1, ptrs, size, part, shard, minio_amd.HIGHWAYHASH256S, status,
        fb) == 6
    assert lib.mec_bitrot_verify_files(
        None, 1, ptrs, size, part, shard, minio_amd.HIGHWAYHASH256S, status,
        None) == 6
    assert status.raw == b"\x77" and fb[0] == -9
