"""The driver depends on bench.py's exact CLI + JSON contract — test it on
CPU with a tiny model so contract breaks are caught before round end."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    env = dict(os.environ, KF_BENCH_MODEL="llama-tiny", KF_BENCH_SEQ="64",
               KF_BENCH_MB="2", PYTHONPATH=REPO)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2",
         "--warmup", "1"], env=env, capture_output=True, text=True,
        timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines()
             if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["value"] > 0
    cfg = d["config"]
    assert cfg["seq_len"] == 64 and cfg["global_batch"] == 2
    assert "model" in cfg and "parallelism" in cfg


def _run_bench(*extra):
    env = dict(os.environ, KF_BENCH_MODEL="llama-tiny", KF_BENCH_SEQ="128",
               KF_BENCH_MB="2", PYTHONPATH=REPO)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", *extra], env=env,
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float .npy,
    identically from run to run; --full keeps the result line's contract."""
    import numpy as np
    a, b = tmp_path / "a", tmp_path / "b"
    da = _run_bench("--dump-outputs", str(a))
    db = _run_bench("--full", "--dump-outputs", str(b))
    for d in (da, db):
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        assert d["metric"] == "pytorchjob_train_tokens_per_s"
        assert d["unit"] == "tokens/s" and d["higher_is_better"] is True
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    assert "loss.npy" in names and "params_sample.npy" in names
    total = 0
    for n in names:
        xa, xb = np.load(a / n), np.load(b / n)
        assert xa.dtype in (np.float32, np.float64), (n, xa.dtype)
        assert np.isfinite(xa).all(), n
        if da["dtype"] == "fp32":
            # CPU path: same seed, same arithmetic, same bits
            assert np.array_equal(xa, xb), n
        elif n in ("loss.npy", "params_sample.npy"):
            # bf16 GPU path: the norm/CE backward kernels accumulate with
            # fp32 atomics, so summation order (not the inputs) may differ
            # between runs; that can move a bf16 parameter by one ulp
            # (2^-7 relative) or one lr-sized (3e-4) AdamW step near zero
            assert np.allclose(xa, xb, rtol=2.0 ** -7, atol=3e-4), n
        total += xa.nbytes
    assert total <= 64 * 1024 * 1024
    assert abs(float(np.load(a / "loss.npy")[0]) - da["config"]["loss"]) < 1e-3
