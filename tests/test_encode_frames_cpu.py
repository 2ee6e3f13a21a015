"""CPU-side checks of the batch encode into on-disk [hash||shard] frames
(mec_encode_frames_batch_var*): the pure-host frame-offset helper, the host
planner and the granule mapping the pack kernel shares with the stand-alone
sanitised program tools/frames_plan_check.cpp, and the null-context check of
the three encode entry points.  Nothing here needs a GPU, and nothing
sanitised is loaded into Python: the checker runs in its own process."""
import ctypes
import os
import random
import subprocess

import pytest

import minio_amd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "minio_amd", "csrc")


def test_planner_and_mapping_sanitised_program(tmp_path):
    """The F prefix equals a brute-force recomputation; every argument error
    is refused with nothing written; and the pack kernel, emulated granule
    by granule through the mapping header it shares with the checker,
    reproduces a naive frame-after-frame assembler at every output phase
    with every load inside its row stride or digest and every store inside
    the output.  The checks live in tools/frames_plan_check.cpp."""
    exe = str(tmp_path / "frames_plan_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", CSRC,
         os.path.join(REPO, "tools", "frames_plan_check.cpp"),
         os.path.join(CSRC, "frames_plan.cpp"),
         os.path.join(CSRC, "var_plan.cpp"),
         "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
    for line in ("offsets: 6 geometries x 400 lengths ok", "refusals: ok",
                 "emulate single-33: ec8+4 n=1 bytes=396 phases=16 body=0",
                 "emulate all-33: ec8+4 n=700", "emulate S-mod-64:",
                 "emulate tiny-long-tiny: ec12+4 n=81",
                 "emulate random-3: ec16+4 n=60"):
        assert line in r.stdout, r.stdout
    assert r.stdout.count(" ok\n") == 12, r.stdout


def test_planner_has_no_hip_dependency():
    """The planner is a host-only translation unit beside scrub_plan.cpp,
    and the mapping header compiles without HIP."""
    for name in ("frames_plan.cpp", "frames_plan.h", "frames_map.h"):
        incs = [ln for ln in open(os.path.join(CSRC, name))
                if ln.lstrip().startswith("#include")]
        assert incs and not any("hip" in ln or "kernels.h" in ln
                                for ln in incs), (name, incs)


@pytest.mark.parametrize("d", [1, 2, 5, 8, 12, 16])
def test_frame_offsets_formula(d):
    bs = 1 << 20
    rng = random.Random(0x6672 + d)
    lens = [rng.choice((1, d, d + 1, bs, rng.randint(1, 300),
                        rng.randint(1, bs))) for _ in range(500)]
    want = [0]
    for ln in lens:
        want.append(want[-1] + 32 + -(-ln // d))
    assert minio_amd.frame_offsets(d, bs, lens) == want
    assert minio_amd.frame_offsets(d, bs, [bs]) == \
        [0, 32 + minio_amd.shard_size(bs, d)]
    # a whole object's blocks as consecutive items: the row stream is the
    # object's shard file
    size = 2 * bs + 300001
    blocks = [bs, bs, 300001]
    assert minio_amd.frame_offsets(d, bs, blocks)[-1] == \
        minio_amd.bitrot_shard_file_size(
            minio_amd.shard_file_size(bs, d, size),
            minio_amd.shard_size(bs, d), minio_amd.HIGHWAYHASH256S)


def test_frame_offsets_refuses_invalid_input():
    bs = 4096
    for lens in ([], [0], [bs + 1], [5, -1, 5], [5, 5, bs + 1], [0, 5]):
        with pytest.raises(minio_amd.MecError) as ei:
            minio_amd.frame_offsets(8, bs, lens)
        assert ei.value.status == 6, lens
    lib = minio_amd._lib
    one = (ctypes.c_int64 * 1)(5)
    three = (ctypes.c_int64 * 3)(5, 5, bs + 1)
    out = (ctypes.c_int64 * 4)(-7, -7, -7, -7)
    assert lib.mec_frame_offsets(0, bs, 1, one, out) == 6      # d = 0
    assert lib.mec_frame_offsets(8, 0, 1, one, out) == 6       # block 0
    assert lib.mec_frame_offsets(8, bs, 0, one, out) == 6
    assert lib.mec_frame_offsets(8, bs, -1, one, out) == 6
    assert lib.mec_frame_offsets(8, bs, 1, None, out) == 6
    assert lib.mec_frame_offsets(8, bs, 1, one, None) == 6
    # a bad length behind good ones: still nothing written
    assert lib.mec_frame_offsets(8, bs, 3, three, out) == 6
    assert list(out) == [-7, -7, -7, -7]
    assert lib.mec_frame_offsets(8, bs, 1, one, out) == 0
    assert list(out) == [0, 33, -7, -7]


def test_null_ctx_is_invalid_arg():
    lib = minio_amd._lib
    lens = (ctypes.c_int64 * 1)(64)
    data = ctypes.create_string_buffer(8 * 64)
    frames = ctypes.create_string_buffer(12 * 40)
    for fn in (lib.mec_encode_frames_batch_var_dev,
               lib.mec_encode_frames_batch_var_dev_async,
               lib.mec_encode_frames_batch_var):
        assert fn(None, 1, data, lens, frames,
                  minio_amd.HIGHWAYHASH256S) == 6
        assert fn(None, 1, data, lens, frames, 0) == 6
    assert frames.raw == b"\0" * (12 * 40)
