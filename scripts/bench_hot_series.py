"""Bucketed measurement series (288 buckets x 8 names) over a full HBM event ring.

Fills a 2^27-event ring on the MI355X with the bench.py fleet (as scripts/bench_hot_query.py does),
then times, for one assignment, 1,000 assignments and one customer (~1/97 of the fleet):

  (a) ``aggregate_store`` on the GPU: scan, sort and reduction in HBM, only the cells cross PCIe;
  (b) the route there was before it: ``query_store(page_size=0)`` (every matching measurement row
      crosses PCIe) followed by ``bucket_series`` on the host;
  (c) with ``--cpu``, the numpy oracle on a host copy of the same ring.

(a) and (b) alternate within each repetition, so both see the same machine.  The GPU cells are checked
against the others' (exact fields equal, sums close) before any time is reported.

    python scripts/bench_hot_series.py --store 134217728 --cpu
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

EXACT = ("count", "min", "max", "first", "last", "first_date", "last_date", "first_id", "last_id")


def same_cells(a, b) -> bool:
    return all(np.array_equal(a[f], b[f]) for f in EXACT) and np.allclose(a["sum"], b["sum"], rtol=1e-12, atol=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 27)
    ap.add_argument("--devices", type=int, default=1 << 20)
    ap.add_argument("--msgs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--buckets", type=int, default=288)
    ap.add_argument("--names", type=int, default=8)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy oracle on a host copy of the ring")
    ap.add_argument("--gpu-only", action="store_true", help="time (a) alone (for a profiler run)")
    args = ap.parse_args()
    import torch

    from sitewhere_amd.models.columnar import EV_MEASUREMENT
    from sitewhere_amd.pipeline.config import EngineConfig
    from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
    from sitewhere_amd.pipeline.fleet import FleetSpec, fingerprints, gen_payloads, gen_tokens, hash64
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine
    from sitewhere_amd.pipeline.series import bucket_series

    cfg = EngineConfig(max_msgs=args.msgs, rec_cap=args.msgs + 4096, max_devices=int(args.devices * 1.1) + 1024,
                       max_assignments=int(args.devices * 1.1) + 1024, store_cap=args.store, dedup_slots=1 << 20,
                       name_slots=1 << 12, state_slots=2 * 20 * int(args.devices * 1.1))
    g = GpuInboundEngine(cfg)
    heap, offs = gen_tokens("dev-", 0, args.devices)
    lo, hi = fingerprints(heap, offs)
    d = g.register_devices(lo, hi)
    g.set_assignments(d, d, customer=d % 97, area=d % 31, asset=d % 1009)
    spec = FleetSpec(prefix="dev-", n_devices=args.devices, p_location=0.25, p_alert=0.05, mx_per_msg=1, n_names=16)
    now0 = int(time.time() * 1000)
    start = now0 - 3_600_000                                # the payloads' dates spread over 60 s from here
    end = start + 59_999
    bucket_ms = -(-60_000 // args.buckets)
    assert (end - start) // bucket_ms + 1 == args.buckets
    batches = []
    for b in range(4):
        raw, o = gen_payloads(spec, args.msgs, start, seed=100 + b)
        batches.append((np.concatenate([raw, np.zeros(64, np.uint8)]), o))
    t0 = time.time()
    k = 0
    while g.cursor < args.store + args.msgs:              # fill and wrap the ring once
        raw, o = batches[k % 4]
        g.step(raw, o, now0 + k, presence=False)
        k += 1
    fill_s = time.time() - t0
    rng = np.random.default_rng(5)
    one = [int(rng.integers(0, args.devices))]
    thousand = rng.choice(args.devices, 1000, replace=False).tolist()
    customer = np.nonzero(d % 97 == 13)[0].tolist()
    queries = {"1 assignment": one, "1000 assignments": thousand, "1 customer (~10.8K assignments)": customer}
    names = [hash64(f"mx.metric{i}") for i in range(args.names)]
    pos = {h: i for i, h in enumerate(names)}

    def gpu(asg):
        return g.aggregate_store(asg, names, start, end, bucket_ms)

    def paged(asg):
        """(b): every matching measurement row to the host, names filtered and bucketed there."""
        _, cols, eids = g.query_store(EV_MEASUREMENT, asg, start, end, page_size=0)
        keep = np.isin(cols["name"], np.asarray(names, np.uint64))
        idx = np.fromiter((pos[int(h)] for h in cols["name"][keep]), np.int64, int(keep.sum()))
        return bucket_series(idx, cols["date"][keep], eids[keep], cols["v0"][keep], start, bucket_ms, len(names),
                             args.buckets)[0]

    out = {"store_events": int(min(g.cursor, args.store)), "fill_s": round(fill_s, 1), "buckets": args.buckets,
           "names": args.names, "bucket_ms": bucket_ms, "reps": args.reps, "queries": {}}
    cells_gpu = {}
    for name, asg in queries.items():
        cells, info = gpu(asg)                              # warm (buffers, code objects)
        cells_gpu[name] = cells
        if not args.gpu_only:
            assert same_cells(cells, paged(asg)), name
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.reps):
            s = time.perf_counter()
            again = gpu(asg)[0]                             # ends in the cells' device-to-host copy: synchronous
            ta.append(1000 * (time.perf_counter() - s))
            assert again.tobytes() == cells.tobytes()
            if not args.gpu_only:
                s = time.perf_counter()
                paged(asg)
                tb.append(1000 * (time.perf_counter() - s))
        q = out["queries"][name] = {"rows": info["rows"], "cells_filled": int((cells["count"] > 0).sum()),
                                    "gpu_ms_p50": round(float(np.median(ta)), 3), "gpu_ms_min": round(float(np.min(ta)), 3),
                                    "gpu_ms_max": round(float(np.max(ta)), 3)}
        if tb:
            q.update(paged_ms_p50=round(float(np.median(tb)), 3), paged_ms_min=round(float(np.min(tb)), 3),
                     paged_ms_max=round(float(np.max(tb)), 3))
    if args.cpu:
        c = CpuInboundEngine.__new__(CpuInboundEngine)       # the numpy oracle over a host copy of the same ring
        c.cfg, c.cursor, c.world, c.rank = cfg, g.cursor, 1, 0
        c.store = {k2: g.store[k2].cpu().numpy() for k2 in ("etype", "asg", "date", "recv", "name", "v0")}
        c.store["name"] = c.store["name"].view(np.uint64)
        for name, asg in queries.items():
            ts = []
            for _ in range(3):
                s = time.perf_counter()
                cells, info = c.aggregate_store(asg, names, start, end, bucket_ms)
                ts.append(1000 * (time.perf_counter() - s))
            assert info["rows"] == out["queries"][name]["rows"] and same_cells(cells_gpu[name], cells), name
            out["queries"][name]["cpu_numpy_ms_p50"] = round(float(np.median(ts)), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
