"""The driver contract: bench.py must run multi-rank (weak scaling along T
with real halo exchange). Exercised here as a 2-process gloo job on a tiny
CPU lattice — the same code path the round-end 8-GPU RCCL run takes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch_two_rank(port):
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    env["MASTER_PORT"] = str(port)
    procs = []
    for r in range(2):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
             "--steps", "1", "--warmup", "0", "--maxiter", "4",
             "--lattice", "4,4,4,8", "--sloppy", "double", "--device", "cpu"],
            env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return procs, outs


def test_bench_two_ranks_gloo():
    import socket
    # the free-port probe is racy against lingering TCPStores from earlier
    # gloo tests in the same session: retry with a fresh port
    for attempt in range(3):
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        sock.close()
        procs, outs = _launch_two_rank(port)
        if all(p.returncode == 0 for p in procs):
            break
    for p in procs:
        assert p.returncode == 0, outs
    line = [l for l in outs[0][0].splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2
    assert rec["ms_per_step"] > 0 and rec["value"] > 0


def test_bench_single_rank_cpu():
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1",
         "--warmup", "0", "--maxiter", "4", "--lattice", "4,4,4,8",
         "--sloppy", "double", "--device", "cpu"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 1


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs writes the last timed solve's solution and statistics;
    the same arguments give the same inputs, so two runs agree (the CPU
    oracle path is deterministic, so they agree bit for bit). --full is
    accepted and leaves the result line's fields in place."""
    import numpy as np

    def run(out_dir, *extra):
        out = subprocess.run(
            [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2",
             "--warmup", "0", "--maxiter", "4", "--lattice", "4,4,4,8",
             "--sloppy", "double", "--device", "cpu",
             "--dump-outputs", str(out_dir), *extra],
            capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        return json.loads(
            [l for l in out.stdout.splitlines() if l.startswith("{")][-1])

    rec = run(tmp_path / "a")
    rec_full = run(tmp_path / "b", "--full")
    for r in (rec, rec_full):
        assert r["steps"] == 2 and r["ms_per_step"] > 0
        for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert k in r
    sol = np.load(tmp_path / "a" / "solution.npy")
    assert sol.dtype == np.float64 and sol.shape == (4 * 4 * 4 * 8 // 2, 4, 3, 2)
    assert np.isfinite(sol).all() and np.abs(sol).max() > 0
    stats = np.load(tmp_path / "a" / "solve_stats.npy")
    assert stats.dtype == np.float64 and stats[0] == rec["config"]["iters_per_solve"]
    assert np.array_equal(sol, np.load(tmp_path / "b" / "solution.npy"))
    assert np.array_equal(stats, np.load(tmp_path / "b" / "solve_stats.npy"))
