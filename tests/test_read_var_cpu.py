"""CPU-side checks of the per-item-length verified batch read
(mec_verify_reconstruct_batch_var*): the host planner, exercised by the
stand-alone sanitised program tools/read_var_plan_check.cpp, and the
null-context check of the two entry points.  Nothing here needs a GPU, and
nothing sanitised is loaded into Python: the planner check runs in its own
process."""
import ctypes
import os
import subprocess

import minio_amd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "minio_amd", "csrc")


def test_planner_sanitised_program(tmp_path):
    """The ordered verify and rehash lists hold exactly the ids of
    build_verify_list / build_rehash_list, grouped by item in the plan's
    descending-S order with rows ascending; the tile prefixes equal a
    brute-force count of 2 KiB steps per pair, for both data_only values,
    with an EC4+10 geometry that rebuilds more than 8 rows; an item outside
    the plan and a tile total past its bound are refused.  The checks live
    in tools/read_var_plan_check.cpp."""
    exe = str(tmp_path / "read_var_plan_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", CSRC,
         os.path.join(REPO, "tools", "read_var_plan_check.cpp"),
         os.path.join(CSRC, "read_var_plan.cpp"),
         os.path.join(CSRC, "var_plan.cpp"),
         os.path.join(CSRC, "recon_plan.cpp"),
         os.path.join(CSRC, "verify_list.cpp"),
         os.path.join(CSRC, "gf_host.cpp"),
         "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    for line in ("small: ok",
                 "lists+tiles ec8+4: n=300 verify=3074 rehash=411/277 "
                 "tiles=4227/3668 too_few=16 ok",
                 "lists+tiles ec2+1: n=500", "lists+tiles ec4+10: n=120",
                 "lists+tiles ec12+4: n=200", "refusals: ok"):
        assert line in r.stdout, r.stdout


def test_planner_has_no_hip_dependency():
    """The planner is a host-only translation unit beside var_plan.cpp."""
    for name in ("read_var_plan.cpp", "read_var_plan.h"):
        incs = [ln for ln in open(os.path.join(CSRC, name))
                if ln.lstrip().startswith("#include")]
        assert incs and not any("hip" in ln or "kernels.h" in ln
                                for ln in incs), (name, incs)


def test_null_ctx_is_invalid_arg():
    lib = minio_amd._lib
    mask = bytes([1] * 12)
    lens = (ctypes.c_int64 * 1)(8 * 64)
    buf = ctypes.create_string_buffer(12 * 64)
    sums = ctypes.create_string_buffer(12 * 32)
    present = ctypes.create_string_buffer(12)
    status = ctypes.create_string_buffer(1)
    for fn in (lib.mec_verify_reconstruct_batch_var_dev,
               lib.mec_verify_reconstruct_batch_var):
        assert fn(None, 1, buf, sums, lens, mask, minio_amd.HIGHWAYHASH256S,
                  0, 0, present, status) == 6
        assert fn(None, 1, buf, sums, lens, mask, minio_amd.HIGHWAYHASH256S,
                  1, 1, None, None) == 6
