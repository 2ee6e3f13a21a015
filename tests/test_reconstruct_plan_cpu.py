"""CPU-side checks of the mixed-pattern batch reconstruct
(mec_reconstruct_batch_mixed*): the host planner, exercised by the
stand-alone sanitised program tools/plan_check.cpp, and the argument checks
of the three C-ABI entry points.  Nothing here needs a GPU, and nothing
sanitised is loaded into Python: the planner runs in its own process."""
import ctypes
import os
import subprocess

import minio_amd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "minio_amd", "csrc")


def test_planner_sanitised_program(tmp_path):
    """EC8+4 with all 793 masks of 1..4 erasures + the all-present mask +
    two 5-erased masks, each 3x in shuffled order, both data_only values:
    one table entry per distinct mask that needs work, the E lists
    partition exactly the recoverable items that need work, every entry's
    rows and bit matrices equal build_decode_plan's, 5-erased items are
    TOO_FEW; (9,9) with 9 data rows erased chunks into 8 + 1 rows over the
    same sources.  The checks themselves live in tools/plan_check.cpp."""
    exe = str(tmp_path / "plan_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", CSRC,
         os.path.join(REPO, "tools", "plan_check.cpp"),
         os.path.join(CSRC, "recon_plan.cpp"),
         os.path.join(CSRC, "gf_host.cpp"),
         "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    assert "entries=793" in r.stdout and "entries=778" in r.stdout


def test_planner_has_no_hip_dependency():
    """The planner is a host-only translation unit next to gf_host.cpp."""
    for name in ("recon_plan.cpp", "recon_plan.h"):
        incs = [ln for ln in open(os.path.join(CSRC, name))
                if ln.lstrip().startswith("#include")]
        assert incs and not any("hip" in ln or "kernels.h" in ln
                                for ln in incs), (name, incs)


def test_null_ctx_is_invalid_arg():
    lib = minio_amd._lib
    present = bytes([1] * 12)
    buf = ctypes.create_string_buffer(12 * 64)
    status = ctypes.create_string_buffer(1)
    for fn in (lib.mec_reconstruct_batch_mixed_dev,
               lib.mec_reconstruct_batch_mixed_dev_async,
               lib.mec_reconstruct_batch_mixed):
        assert fn(None, 1, buf, present, 64, 0, status) == 6
        assert fn(None, 1, buf, present, 64, 1, None) == 6
