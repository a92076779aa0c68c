"""bench.py's multi-rank path on real hardware, on a one-GPU box: `--gpus 2` relaunches itself under
torch.distributed.run, both ranks land on cuda:0 (--share-gpus: bench_device wraps LOCAL_RANK and the
line is marked shared, n_gpus = 1 distinct device; without the flag the run exits), the gloo group
carries the barrier and the scalar max/sum of the timing rule, and rank 0 prints one JSON line
whose value is the whole-job rate (codewords of both ranks / max-over-ranks time)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_on_one_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
                        "--warmup", "1", "--ncw", str(1 << 16), "--no-cpu-baseline", "--no-extras", "--share-gpus"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    ndev = torch.cuda.device_count()
    if ndev >= 2:
        assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    else:                                   # both ranks on one GPU: marked, never a scaling line
        assert line["n_gpus"] == 1 and line["ranks"] == 2 and line["shared_gpus"] is True
        assert not line["scaling"].startswith("weak")
    assert line["config"]["global_codewords"] == 2 << 16
    # value = both ranks' codewords / the max-over-ranks time
    assert abs(line["value"] - 2 * 3 * (1 << 16) * 255 / (line["ms_per_step"] * 3e-3) / 1e9) < 0.02 * line["value"]


def test_plain_run_dumps_its_outputs(tmp_path):
    """A plain `--gpus 1 --steps K --warmup W` run with --dump-outputs: the line carries only the
    headline (no roofline pass, extras or CPU baseline), and DIR holds what the last timed step left
    with the caller, float32: `result` (every codeword decoded clean) and a seeded row sample of
    `codewords` (40 000 rows are more than one array's share of the dump) whose parity columns equal
    the oracle's encode of their data columns."""
    import numpy as np
    import torch
    import oracle as O
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ncw, out = 40000, tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--spinup", "0", "--ncw", str(ncw), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "GB/s"
    assert abs(line["value"] - ncw * 255 / (line["ms_per_step"] * 1e-3) / 1e9) < 0.02 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and "c2_4m" not in line
    assert sorted(os.listdir(out)) == ["codewords.npy", "codewords_rows.npy", "result.npy"]
    res = np.load(out / "result.npy")
    assert res.dtype == np.float32 and res.shape == (ncw,) and not res.any()
    cw, rows = np.load(out / "codewords.npy"), np.load(out / "codewords_rows.npy")
    assert cw.dtype == np.float32 and cw.shape == (len(rows), 255) and len(rows) < ncw
    assert rows.dtype == np.float64 and (np.diff(rows) > 0).all() and 0 <= rows[0] and rows[-1] < ncw
    got = cw.astype(np.uint8)
    assert np.array_equal(got, cw) and len(np.unique(got[:, :223])) == 256
    exp = got.copy()
    exp[:, 223:] = 0
    O.Codec(*O.rs_params(255, 223)).encode_batch(exp, 223)
    assert np.array_equal(got, exp)
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
