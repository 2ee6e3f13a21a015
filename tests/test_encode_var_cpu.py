"""CPU-side checks of the per-item-length batch encode
(mec_encode_batch_var*): the host planner, exercised by the stand-alone
sanitised program tools/var_plan_check.cpp, the pure-host row-offset helper,
and the null-context check of the three encode entry points.  Nothing here
needs a GPU, and nothing sanitised is loaded into Python: the planner check
runs in its own process."""
import ctypes
import os
import random
import subprocess

import pytest

import minio_amd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "minio_amd", "csrc")


def test_planner_sanitised_program(tmp_path):
    """Row offsets, shard lengths and column prefixes equal a brute-force
    recomputation for seeded lengths at five geometries; the hash order is a
    stable descending permutation; lengths outside [1, block_size] are
    refused wherever they stand; n*(d+p) past 32 bits, a column total past
    its bound and row bytes past int64 are refused.  The checks live in
    tools/var_plan_check.cpp."""
    exe = str(tmp_path / "var_plan_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", CSRC,
         os.path.join(REPO, "tools", "var_plan_check.cpp"),
         os.path.join(CSRC, "var_plan.cpp"),
         "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    for line in ("tables ec8+4: n=302", "tables ec5+2: n=302",
                 "tables single: n=1 rows=87552 cols=2735 ok",
                 "tables equal: n=100 rows=51200 cols=1600 ok",
                 "tables ascending: n=200", "refusals: ok", "guards: ok"):
        assert line in r.stdout, r.stdout


def test_planner_has_no_hip_dependency():
    """The planner is a host-only translation unit beside recon_plan.cpp."""
    for name in ("var_plan.cpp", "var_plan.h"):
        incs = [ln for ln in open(os.path.join(CSRC, name))
                if ln.lstrip().startswith("#include")]
        assert incs and not any("hip" in ln or "kernels.h" in ln
                                for ln in incs), (name, incs)


@pytest.mark.parametrize("d", [1, 2, 5, 8, 12, 16])
def test_var_row_offsets_formula(d):
    bs = 1 << 20
    rng = random.Random(0x7661 + d)
    lens = [rng.choice((1, d, d + 1, bs, rng.randint(1, 300),
                        rng.randint(1, bs))) for _ in range(500)]
    want = [0]
    for ln in lens:
        want.append(want[-1] + (-(-ln // d) + 63) // 64 * 64)
    assert minio_amd.var_row_offsets(d, bs, lens) == want
    assert minio_amd.var_row_offsets(d, bs, [bs]) == \
        [0, minio_amd._lib.mec_shard_stride(bs, d)]


def test_var_row_offsets_refuses_invalid_input():
    bs = 4096
    for lens in ([], [0], [bs + 1], [5, -1, 5], [5, 5, bs + 1], [0, 5]):
        with pytest.raises(minio_amd.MecError) as ei:
            minio_amd.var_row_offsets(8, bs, lens)
        assert ei.value.status == 6, lens
    lib = minio_amd._lib
    one = (ctypes.c_int64 * 1)(5)
    out = (ctypes.c_int64 * 2)(-7, -7)
    assert lib.mec_var_row_offsets(0, bs, 1, one, out) == 6      # d = 0
    assert lib.mec_var_row_offsets(8, 0, 1, one, out) == 6       # block 0
    assert lib.mec_var_row_offsets(8, bs, 1, None, out) == 6
    assert lib.mec_var_row_offsets(8, bs, 1, one, None) == 6
    # chain ids past 32 bits: refused before the lengths are read
    assert lib.mec_var_row_offsets(8, bs, 2**31 - 1, one, out) == 6
    assert list(out) == [-7, -7]                 # nothing was written
    assert lib.mec_var_row_offsets(8, bs, 1, one, out) == 0
    assert list(out) == [0, 64]


def test_null_ctx_is_invalid_arg():
    lib = minio_amd._lib
    lens = (ctypes.c_int64 * 1)(64)
    data = ctypes.create_string_buffer(8 * 64)
    parity = ctypes.create_string_buffer(4 * 64)
    sums = ctypes.create_string_buffer(12 * 32)
    for fn in (lib.mec_encode_batch_var_dev,
               lib.mec_encode_batch_var_dev_async,
               lib.mec_encode_batch_var):
        assert fn(None, 1, data, lens, parity, minio_amd.HIGHWAYHASH256S,
                  sums) == 6
        assert fn(None, 1, data, lens, parity, 0, None) == 6
