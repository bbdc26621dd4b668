"""bench.py contract (driver-facing): one JSON line from rank 0 with the required keys, for N=1 and for
N=2 ranks under torch.distributed.run (gloo + the CPU oracle engine, so it runs without a GPU)."""
from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}
SMALL = ["--engine", "cpu", "--msgs", "1500", "--devices", "1500", "--steps", "2", "--warmup", "1", "--store", "65536",
         "--batches", "2"]


def _json_lines(out: str):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def test_bench_single_rank_json():
    r = subprocess.run([sys.executable, "bench.py", *SMALL], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    d = lines[0]
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["metric"] == "device_events_per_sec" and d["value"] > 0 and d["higher_is_better"] is True
    assert {"model", "global_batch", "seq_len", "parallelism"} <= set(d["config"])
    # the timed region ends with every block of the run durable on disk
    dd = d["detail"]["durable"]
    assert d["config"]["durable"] and dd["all_durable"] and dd["rows"] == d["detail"]["persisted"]
    assert dd["bytes_per_event"] > 0 and dd["durable_bytes_per_s"] > 0 and dd["fdatasyncs"] >= 1
    assert d["detail"]["conservation"]["ok"]
    assert dd["disk_probe"] is None                 # a plain run times its steps only; the probe needs --full


def test_bench_dump_outputs_repeat(tmp_path):
    """``--dump-outputs``: two runs with the same arguments write the same arrays (seeded inputs dated
    from a fixed epoch), with or without ``--full``, which adds the disk probe to the result line."""
    import numpy as np
    runs = []
    for name, extra in (("a", []), ("b", ["--full", "--disk-probe-mb", "8"])):
        # three batches: the host engines replay their batches unstamped, and a replay is all duplicates
        r = subprocess.run([sys.executable, "bench.py", *SMALL, "--batches", "3", *extra,
                            "--dump-outputs", str(tmp_path / name)],
                           cwd=REPO, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(_json_lines(r.stdout)[0])
    assert runs[0]["detail"]["durable"]["disk_probe"] is None
    assert runs[1]["detail"]["durable"]["disk_probe"]["rank0_gbps"] > 0
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    cols = {"etype", "assignment", "event_date", "name_hash_hi", "name_hash_lo", "level", "flags", "v0", "v1", "v2"}
    assert {f[:-4] for f in files if f.endswith(".npy")} == cols | {"summary", "counters"}
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in files if f.endswith(".npy")}
    for k, v in a.items():
        assert v.dtype == np.float64 and np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy")), equal_nan=True), k
    # the rows of the last timed step's block, all kept at this size; the counters cover both timed steps
    n = int(a["summary"][0])
    assert 0 < n == int(a["summary"][1]) and all(len(a[k]) == n for k in cols)
    names = (tmp_path / "a" / "counter_names.txt").read_text().split()
    counters = dict(zip(names, a["counters"]))
    assert counters["persisted"] == runs[0]["detail"]["persisted"] and counters["messages"] == 2 * 1500
    assert set(np.unique(a["etype"])) <= set(range(8)) and a["name_hash_lo"].max() > 0


@pytest.mark.slow
def test_bench_two_ranks_torchrun(tmp_path):
    """Two ranks on gloo, each with its own segment directory (one per disk: ``--durable-dir a,b``):
    conservation holds over both ranks and each rank's blocks are in its own directory."""
    d1, d2 = str(tmp_path / "disk1"), str(tmp_path / "disk2")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", *SMALL,
                        "--full", "--durable-dir", f"{d1},{d2}", "--disk-probe-mb", "8"],
                       cwd=REPO, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 3000 and d["config"]["parallelism"].startswith("dp2")
    assert d["detail"]["payloads"] == 2 * 2 * 1500
    # self-checking multi-rank record: the backend and world the process group really had, per-rank time
    det = d["detail"]
    assert det["backend"] == "gloo" and det["world"] == 2 and len(det["rank_elapsed_s"]) == 2
    assert det["exchange_bytes_per_rank_step"] > 0 and det["shuffle_overflow"] == 0
    assert det["conservation"]["ok"] and det["conservation"]["checked"] >= 4
    assert det["durable"]["disk_probe"]["dirs"] == 2 and det["durable"]["disk_probe"]["node_gbps"] > 0
    # local rank r writes to dirs[r % 2]
    for d, r in ((d1, 0), (d2, 1)):
        files = os.listdir(os.path.join(d, f"rank{r}"))
        assert any(f.endswith(".sweg") for f in files), (d, files)
