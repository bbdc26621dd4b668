"""Rankings of groups over a full HBM event ring.

Fills a 2^27-event ring on the MI355X with the bench.py fleet (as scripts/bench_hot_grid.py does), then
appends ``--hot-steps`` steps that one device alone sends, so the ring's newest rows are one hot key in
runs as long as a wave.  Then times, per call:

  (a) ``rank_store`` on the GPU: scan, group-by and ordering in HBM, only the first k cells and four
      counters cross PCIe;
  (b) the route there was before it: ``query_store(type, every assignment, page_size=0)`` (every row of the
      type, all 16 columns, crosses PCIe) followed by ``rank.rank_select`` on the host.  Run for alerts and
      locations only: paging every measurement of the ring takes tens of gigabytes of host memory.

(a) and (b) alternate within a repetition; ``--paged-reps`` bounds how many repetitions also run (b).
Before any time is taken (a) is checked against (b): the cells' bytes and the counters equal.

``--forms`` adds what ``SW_RANK_LDS_KEYS`` rests on, (a) alone, alternated within a repetition: the LDS
form against the global form (limit 0) grouping by a few-key dimension and by the hot device's customer.

    python scripts/bench_hot_rank.py --store 134217728 --forms
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 27)
    ap.add_argument("--devices", type=int, default=1 << 20)
    ap.add_argument("--msgs", type=int, default=1 << 20)
    ap.add_argument("--hot-steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--paged-reps", type=int, default=2, help="repetitions that also run (b)")
    ap.add_argument("--gpu-only", action="store_true", help="time (a) alone (for a profiler run)")
    ap.add_argument("--forms", action="store_true", help="compare the fold's LDS and global forms")
    args = ap.parse_args()
    import torch

    from sitewhere_amd._native import gpu
    from sitewhere_amd.models.columnar import EV_ALERT, EV_LOCATION, EV_MEASUREMENT
    from sitewhere_amd.pipeline.config import EngineConfig
    from sitewhere_amd.pipeline.fleet import FleetSpec, fingerprints, gen_payloads, gen_tokens
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine
    from sitewhere_amd.pipeline.rank import rank_select

    cfg = EngineConfig(max_msgs=args.msgs, rec_cap=args.msgs + 4096, max_devices=int(args.devices * 1.1) + 1024,
                       max_assignments=int(args.devices * 1.1) + 1024, store_cap=args.store, dedup_slots=1 << 20,
                       name_slots=1 << 12, state_slots=2 * 20 * int(args.devices * 1.1))
    g = GpuInboundEngine(cfg)
    heap, offs = gen_tokens("dev-", 0, args.devices)
    lo, hi = fingerprints(heap, offs)
    d = g.register_devices(lo, hi)
    g.set_assignments(d, d, customer=d % 97, area=d % 31, asset=d % 1009)
    spec = FleetSpec(prefix="dev-", n_devices=args.devices, p_location=0.25, p_alert=0.05, mx_per_msg=1, n_names=16)
    hot_spec = FleetSpec(prefix="dev-", n_devices=1, p_location=0.25, p_alert=0.05, mx_per_msg=1, n_names=16)
    now0 = int(time.time() * 1000)
    start = now0 - 3_600_000
    batches = []
    for b in range(4):
        raw, o = gen_payloads(spec, args.msgs, start, seed=100 + b)
        batches.append((np.concatenate([raw, np.zeros(64, np.uint8)]), o))
    raw, o = gen_payloads(hot_spec, args.msgs, start, seed=200)
    hot_batch = (np.concatenate([raw, np.zeros(64, np.uint8)]), o)
    t0 = time.time()
    k = 0
    while g.cursor < args.store + args.msgs:              # fill and wrap the ring once
        raw, o = batches[k % 4]
        g.step(raw, o, now0 + k, presence=False)
        k += 1
    for _ in range(args.hot_steps):                       # the newest rows: device 0 alone
        g.step(*hot_batch, now0 + k, presence=False)
        k += 1
    fill_s = time.time() - t0
    every = np.asarray(d, np.int64)
    lib = gpu()
    compiled = int(lib.sw_rank_lds_keys(-1))
    # the generator's names: whichever measurement name the ring holds most of
    _, cols, _ = g.query_store(EV_MEASUREMENT, [0], page_size=65536)
    names, counts = np.unique(cols["name"], return_counts=True)
    name = int(names[np.argmax(counts)])
    del cols

    M, L, A = EV_MEASUREMENT, EV_LOCATION, EV_ALERT
    queries = {
        "alerts by customer, info and above, top 10": dict(event_type=A, group="customer", k=10, min_level=0),
        "locations by area, quietest 10": dict(event_type=L, group="area", k=10, ascending=True),
        "measurements by asset, top 10": dict(event_type=M, group="asset", k=10),
        "max of one name by assignment, top 10": dict(event_type=M, group="assignment", stat="max", k=10, name_hash=name),
        "last of one name by customer, all": dict(event_type=M, group="customer", stat="last", k=None, name_hash=name),
        "count by assignment, all groups": dict(event_type=M, group="assignment", k=None),
    }
    col = {"assignment": "asg", "customer": "cust", "area": "area", "asset": "asset"}

    def paged(q):
        """(b): the type's rows to the host, the filter, the fold and the ordering there."""
        _, cols, eids = g.query_store(q["event_type"], every, page_size=0)
        keep = np.ones(len(eids), bool)
        if "min_level" in q:
            keep &= cols["level"] >= q["min_level"]
        n_keys = g.rank_key_space(q["group"])[1]
        cells, rows, nan, ung, groups = rank_select(cols[col[q["group"]]][keep], cols["date"][keep], eids[keep], None, n_keys,
                                                    q.get("stat", "count"), q["k"], q.get("ascending", False))
        return cells, {"candidates": int(keep.sum()), "rows": rows, "nan": nan, "ungrouped": ung, "groups": groups}

    def stats(ts, unit=3):
        return {"p50": round(float(np.median(ts)), unit), "min": round(float(np.min(ts)), unit),
                "max": round(float(np.max(ts)), unit)}

    def same(a, b):
        return a[0].tobytes() == b[0].tobytes() and a[1] == b[1]

    out = {"store_events": int(min(g.cursor, args.store)), "fill_s": round(fill_s, 1), "reps": args.reps,
           "paged_reps": 0 if args.gpu_only else args.paged_reps, "lds_keys_compiled": compiled,
           "key_spaces": {grp: g.rank_key_space(grp)[1] for grp in col}, "queries": {}, "forms": {}}
    for qname, q in queries.items():
        first = g.rank_store(**q)                                     # warm (buffers, code objects)
        can_page = not args.gpu_only and q["event_type"] != M
        if can_page:
            cb, ib = paged(q)
            assert first[0].tobytes() == cb.tobytes() and {k2: first[1][k2] for k2 in ib} == ib, (qname, first[1], ib)
        torch.cuda.synchronize()
        ta, tb = [], []
        for rep in range(args.reps):
            s = time.perf_counter()
            again = g.rank_store(**q)                                 # ends in device-to-host copies: synchronous
            ta.append(1000 * (time.perf_counter() - s))
            assert same(again, first), qname
            if can_page and rep < args.paged_reps:
                s = time.perf_counter()
                paged(q)
                tb.append(1000 * (time.perf_counter() - s))
                print(f"{qname}: repetition {rep + 1}: (a) {ta[-1]:.2f} ms, (b) {tb[-1]:.0f} ms", file=sys.stderr, flush=True)
        info = first[1]
        r = out["queries"][qname] = {k2: info[k2] for k2 in ("candidates", "rows", "nan", "ungrouped", "groups")}
        r["form"] = "lds" if g.rank_key_space(q["group"])[1] <= compiled else "global"
        r["gpu_ms"] = stats(ta)
        if tb:
            r["paged_ms"] = stats(tb, 1)

    def alternate(q, settings, apply):
        """(a) alone under each setting in turn within a repetition; the first turn warms each."""
        want = g.rank_store(**q)
        ts = {s_: [] for s_ in settings}
        for rep in range(args.reps + 1):
            for s_ in settings:
                apply(s_)
                t = time.perf_counter()
                again = g.rank_store(**q)
                if rep:
                    ts[s_].append(1000 * (time.perf_counter() - t))
                assert same(again, want), (q, s_)
        return {str(s_): stats(ts[s_]) for s_ in settings}, want[1]

    if args.forms:
        shapes = {
            "measurements by area (31 keys)": dict(event_type=M, group="area", k=None),
            "max of one name by asset (1009 keys)": dict(event_type=M, group="asset", stat="max", k=None, name_hash=name),
            "hot device by customer (one key)": dict(event_type=M, group="customer", k=None, asg_idx=[0]),
        }
        for sname, q in shapes.items():
            res, info = alternate(q, [compiled, 0], lambda lim: lib.sw_rank_lds_keys(lim))
            lib.sw_rank_lds_keys(compiled)
            out["forms"][sname] = {"rows": info["rows"], "groups": info["groups"], "lds": res[str(compiled)], "global": res["0"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
