"""Location density grids over a full HBM event ring.

Fills a 2^27-event ring on the MI355X with the bench.py fleet (as scripts/bench_hot_zone.py does), whose
locations spread over lat 33.75 - 34.25, lon -84.39 - -83.89, then times, tenant-wide, grids of 1 x 1,
64 x 64 and 256 x 256 cells over a box around the fleet, each plain and with ``latest=True``:

  (a) ``grid_store`` on the GPU: scan, cell formula and histogram in HBM, only the cell table (16 B a
      cell) and three counters cross PCIe;
  (b) the route there was before it: ``query_store(EV_LOCATION, every assignment, page_size=0)`` (every
      location row, all 16 columns, crosses PCIe) followed by ``grid.grid_select`` on the host.

(a) and (b) alternate within a repetition, so both see the same machine; ``--paged-reps`` bounds how
many of the repetitions also run (b), which takes seconds per call.  Before any time is taken (a) is
checked against (b): the cells' bytes, candidates, invalid and outside equal -- there is no band.

``--lds`` adds the comparison ``SW_GRID_LDS_CELLS`` rests on: each grid again, (a) alone, with the
workgroups' LDS tables at the given limits of cells (0: every increment goes to the global table),
the limits alternating within a repetition.  A limit above what the library was compiled with is
clipped to it, and a grid above the limit takes the global table either way.

    python scripts/bench_hot_grid.py --store 134217728 --lds 0,1024,4096
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--paged-reps", type=int, default=None, help="repetitions that also run (b) (default: all)")
    ap.add_argument("--gpu-only", action="store_true", help="time (a) alone (for a profiler run)")
    ap.add_argument("--lds", default="", help="LDS table limits in cells to compare (comma list; 0: global only)")
    args = ap.parse_args()
    import torch

    from sitewhere_amd._native import gpu
    from sitewhere_amd.models.columnar import EV_LOCATION
    from sitewhere_amd.pipeline.config import EngineConfig
    from sitewhere_amd.pipeline.fleet import FleetSpec, fingerprints, gen_payloads, gen_tokens
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine
    from sitewhere_amd.pipeline.grid import grid_select

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
    start = now0 - 3_600_000
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
    pad = spec.span_deg / 10
    box = (spec.lat0 - pad, spec.lat0 + spec.span_deg + pad, spec.lon0 - pad, spec.lon0 + spec.span_deg + pad)
    grids = {"1 x 1": (1, 1), "64 x 64": (64, 64), "256 x 256": (256, 256)}
    variants = {"": False, ", latest": True}
    every = np.asarray(d, np.int64)
    paged_reps = args.reps if args.paged_reps is None else min(args.paged_reps, args.reps)
    lib = gpu()
    compiled = int(lib.sw_grid_lds_cells(-1))

    def paged(rows, cols_, latest):
        """(b): the location rows to the host, the cell formula and the histogram there."""
        _, cols, eids = g.query_store(EV_LOCATION, every, page_size=0)
        cells, bad, outside = grid_select(cols["asg"], cols["date"], eids, cols["v0"], cols["v1"], box, rows, cols_, latest)
        return cells, len(eids), bad, outside

    def stats(ts, unit=3):
        return {"p50": round(float(np.median(ts)), unit), "min": round(float(np.min(ts)), unit),
                "max": round(float(np.max(ts)), unit)}

    out = {"store_events": int(min(g.cursor, args.store)), "fill_s": round(fill_s, 1), "box": box, "reps": args.reps,
           "paged_reps": 0 if args.gpu_only else paged_reps, "lds_cells_compiled": compiled, "queries": {}, "lds": {}}
    for gname, (rows, cols_) in grids.items():
        for vname, latest in variants.items():
            name = gname + vname
            cells, info = g.grid_store(*box, rows, cols_, latest=latest)              # warm (buffers, code objects)
            if not args.gpu_only:
                cb, cand_b, bad_b, out_b = paged(rows, cols_, latest)
                assert (info["candidates"], info["invalid"], info["outside"]) == (cand_b, bad_b, out_b), (name, info)
                assert cells.tobytes() == cb.tobytes(), name
            torch.cuda.synchronize()
            ta, tb = [], []
            for rep in range(args.reps):
                s = time.perf_counter()
                again = g.grid_store(*box, rows, cols_, latest=latest)      # ends in device-to-host copies: synchronous
                ta.append(1000 * (time.perf_counter() - s))
                assert again[0].tobytes() == cells.tobytes() and again[1] == info
                if not args.gpu_only and rep < paged_reps:
                    s = time.perf_counter()
                    paged(rows, cols_, latest)
                    tb.append(1000 * (time.perf_counter() - s))
                    print(f"{name}: repetition {rep + 1} of {args.reps}: (a) {ta[-1]:.2f} ms, (b) {tb[-1]:.0f} ms",
                          file=sys.stderr, flush=True)          # (b) takes seconds: show that the run is alive
            r = out["queries"][name] = {"candidates": info["candidates"], "invalid": info["invalid"],
                                        "outside": info["outside"], "counted": int(cells["count"].sum()),
                                        "cells_filled": int((cells["count"] > 0).sum()),
                                        "max_cell": int(cells["count"].max()), "gpu_ms": stats(ta)}
            if tb:
                r["paged_ms"] = stats(tb, 1)
            limits = [int(x) for x in args.lds.split(",") if x]
            if limits:
                tl = {lim: [] for lim in limits}
                for rep in range(args.reps + 1):
                    for lim in limits:
                        lib.sw_grid_lds_cells(lim)
                        s = time.perf_counter()
                        again = g.grid_store(*box, rows, cols_, latest=latest)
                        if rep:                                 # the first turn warms each form
                            tl[lim].append(1000 * (time.perf_counter() - s))
                        assert again[0].tobytes() == cells.tobytes() and again[1] == info, (name, lim)
                lib.sw_grid_lds_cells(compiled)
                out["lds"][name] = {str(lim): dict(stats(tl[lim]), form="lds" if rows * cols_ <= min(lim, compiled) else "global")
                                    for lim in limits}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
