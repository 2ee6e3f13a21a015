"""bench.py's command line (GPU): a plain run is lean and its
--dump-outputs arrays are what the timed path computed, bit-exact against
the CPU oracle; --full adds the roofline split."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x6D696E696F  # bench.py's input seed: block b is fill_random(bs, SEED + b)


def run_bench(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--batch", "8", *extra],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines  # one JSON result line, nothing else
    return json.loads(lines[0])


def test_plain_run_dumps_last_step_outputs(tmp_path):
    out = run_bench("--dump-outputs", str(tmp_path))
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "GiB/s" and out["dtype"] == "u8"
    assert out["higher_is_better"] is True
    # the extra measurements live behind --full
    assert out["roofline"] is None and out["cpu_baseline"] is None

    d, p, bs, n = 8, 4, 1 << 20, 8
    parity = np.load(tmp_path / "parity.npy")
    sums = np.load(tmp_path / "sums.npy")
    assert parity.dtype == np.float32 and sums.dtype == np.float32
    # 8 blocks fit the dump budget, so both arrays are complete
    S = bs // d
    assert parity.shape == (n * p * S,) and sums.shape == (n * (d + p) * 32,)
    rs = oracle.RS(d, p)
    want_par, want_sum = bytearray(), bytearray()
    for b in range(n):
        shards = rs.encode_data(oracle.fill_random(bs, SEED + b))
        for sh in shards[d:]:
            want_par += sh
        for sh in shards:
            want_sum += oracle.bitrot_sum(oracle.HIGHWAYHASH256S, sh)
    assert parity.astype(np.uint8).tobytes() == bytes(want_par)
    assert sums.astype(np.uint8).tobytes() == bytes(want_sum)


def test_decode_run_dumps_rebuilt_rows(tmp_path):
    out = run_bench("--op", "decode", "--dump-outputs", str(tmp_path))
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    d, bs, n, n_erased = 8, 1 << 20, 8, 3
    S = bs // d
    rebuilt = np.load(tmp_path / "reconstructed.npy")
    assert rebuilt.dtype == np.float32 and rebuilt.shape == (n * n_erased * S,)
    # the erased rows are the first data shards: the input's leading bytes
    want = b"".join(oracle.fill_random(bs, SEED + b)[:n_erased * S]
                    for b in range(n))
    assert rebuilt.astype(np.uint8).tobytes() == want


def test_full_run_adds_roofline():
    out = run_bench("--full", "--no-cpu-baseline")
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    roof = out["roofline"]
    assert roof is not None and roof["achieved"] > 0
    assert set(roof["legs_ms"]) == {"gf", "hash"}
    assert out["cpu_baseline"] is None  # --no-cpu-baseline
