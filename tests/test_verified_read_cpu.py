"""CPU-side checks of the verified batch read
(mec_verify_reconstruct_batch*): the host list builder, exercised by the
stand-alone sanitised program tools/verify_list_check.cpp, and the argument
checks of the two C-ABI entry points.  Nothing here needs a GPU, and nothing
sanitised is loaded into Python: the list builder runs in its own process."""
import ctypes
import os
import subprocess

import minio_amd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "minio_amd", "csrc")


def test_list_builder_sanitised_program(tmp_path):
    """The verify list is exactly the set bits of read_mask in order; the
    merge is read & ok; the rehash list equals the destination rows of the
    plan's own work lists for both data_only values, with a (9,9) item that
    rebuilds 9 rows and TOO_FEW items that contribute nothing; n*(d+p) past
    32 bits is refused.  The checks live in tools/verify_list_check.cpp."""
    exe = str(tmp_path / "verify_list_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", CSRC,
         os.path.join(REPO, "tools", "verify_list_check.cpp"),
         os.path.join(CSRC, "verify_list.cpp"),
         os.path.join(CSRC, "recon_plan.cpp"),
         os.path.join(CSRC, "gf_host.cpp"),
         "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    for line in ("verify list: ok", "merge: ok", "32-bit guard: ok",
                 "rehash list ec9+9 data_only=0: 27 rows, too_few=1 ok",
                 "rehash list ec9+9 data_only=1: 14 rows, too_few=1 ok"):
        assert line in r.stdout, r.stdout


def test_list_builder_has_no_hip_dependency():
    """The list builder is a host-only translation unit beside
    recon_plan.cpp."""
    for name in ("verify_list.cpp", "verify_list.h"):
        incs = [ln for ln in open(os.path.join(CSRC, name))
                if ln.lstrip().startswith("#include")]
        assert incs and not any("hip" in ln or "kernels.h" in ln
                                for ln in incs), (name, incs)


def test_null_ctx_is_invalid_arg():
    lib = minio_amd._lib
    mask = bytes([1] * 12)
    buf = ctypes.create_string_buffer(12 * 64)
    sums = ctypes.create_string_buffer(12 * 32)
    present = ctypes.create_string_buffer(12)
    status = ctypes.create_string_buffer(1)
    for fn in (lib.mec_verify_reconstruct_batch_dev,
               lib.mec_verify_reconstruct_batch):
        assert fn(None, 1, buf, sums, mask, 64, minio_amd.HIGHWAYHASH256S,
                  0, 0, present, status) == 6
        assert fn(None, 1, buf, sums, mask, 64, minio_amd.HIGHWAYHASH256S,
                  1, 1, None, None) == 6
