"""Locations in a zone over a full HBM event ring.

Fills a 2^27-event ring on the MI355X with the bench.py fleet (as scripts/bench_hot_near.py does),
whose locations spread over lat 33.75 - 34.25, lon -84.39 - -83.89, then times, tenant-wide, three
zones -- a 4-vertex rectangle (the middle half of that square each way), a 14-vertex concave star and
a 1024-vertex polygon inscribed in the square, so that its box is the whole fleet -- each plain, with
``latest=True`` and with ``outside=True``:

  (a) ``zone_store`` on the GPU: scan, box test, crossing loop and ordering in HBM, only the page (100
      rows) crosses PCIe;
  (b) the route there was before it: ``query_store(EV_LOCATION, every assignment, page_size=0)`` (every
      location row, all 16 columns, crosses PCIe) followed by ``zone.zone_select`` on the host.

(a) and (b) alternate within a repetition, so both see the same machine; ``--paged-reps`` bounds how
many of the repetitions also run (b), which takes seconds per call.  Before any time is taken (a) is
checked against (b): total, candidates, invalid and the page's event ids equal -- there is no band.
With 1024 vertices (b) takes minutes over every location row, so there both the check and (b)'s time
are taken over every ``--sample``-th assignment (the same query on both sides); (a)'s times are
tenant-wide throughout.

    python scripts/bench_hot_zone.py --store 134217728
"""
from __future__ import annotations

import argparse
import json
import math
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
    ap.add_argument("--sample", type=int, default=64, help="(b) with 1024 vertices: every n-th assignment")
    ap.add_argument("--gpu-only", action="store_true", help="time (a) alone (for a profiler run)")
    ap.add_argument("--polygons", default="", help="only the polygons whose name starts with one of these (comma list)")
    args = ap.parse_args()
    import torch

    from sitewhere_amd.models.columnar import EV_LOCATION
    from sitewhere_amd.pipeline.config import EngineConfig
    from sitewhere_amd.pipeline.fleet import FleetSpec, fingerprints, gen_payloads, gen_tokens
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine
    from sitewhere_amd.pipeline.zone import zone_select

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
    c = (spec.lat0 + spec.span_deg / 2, spec.lon0 + spec.span_deg / 2)
    h = spec.span_deg / 2
    polygons = {
        "rectangle, 4": np.array([[c[0] - h / 2, c[1] - h / 2], [c[0] + h / 2, c[1] - h / 2], [c[0] + h / 2, c[1] + h / 2],
                                  [c[0] - h / 2, c[1] + h / 2]]),
        "star, 14": np.array([[c[0] + (h if i % 2 == 0 else 0.36 * h) * math.cos(math.pi * i / 7),
                               c[1] + (h if i % 2 == 0 else 0.36 * h) * math.sin(math.pi * i / 7)] for i in range(14)]),
        "polygon, 1024": np.array([[c[0] + h * math.cos(2 * math.pi * i / 1024), c[1] + h * math.sin(2 * math.pi * i / 1024)]
                                   for i in range(1024)]),
    }
    variants = {"": dict(), ", latest": dict(latest=True), ", outside": dict(outside=True)}
    every = np.asarray(d, np.int64)
    paged_reps = args.reps if args.paged_reps is None else min(args.paged_reps, args.reps)

    def paged(poly, q, asg):
        """(b): the location rows to the host, the zone test and the ordering there."""
        _, cols, eids = g.query_store(EV_LOCATION, asg, page_size=0)
        sel, bad = zone_select(cols["asg"], cols["date"], eids, cols["v0"], cols["v1"], poly, q.get("outside", False),
                               q.get("latest", False))
        return len(sel), eids[sel[:100]], len(eids), bad

    out = {"store_events": int(min(g.cursor, args.store)), "fill_s": round(fill_s, 1), "centre": c,
           "reps": args.reps, "paged_reps": 0 if args.gpu_only else paged_reps, "sample": args.sample, "queries": {}}
    only = tuple(p for p in args.polygons.split(",") if p)
    for pname, poly in polygons.items():
        if only and not pname.startswith(only):
            continue
        sampled = len(poly) > 100 and args.sample > 1
        asg_b = every[::args.sample] if sampled else every
        for vname, q in variants.items():
            name = pname + vname
            total, cols, eids, info = g.zone_store(poly, **q)              # warm (buffers, code objects)
            if not args.gpu_only:
                n_b, ids_b, cand_b, bad_b = paged(poly, q, asg_b)
                ta_, _, ea_, ia_ = g.zone_store(poly, asg_idx=asg_b, **q) if sampled else (total, cols, eids, info)
                assert (ta_, ia_["candidates"], ia_["invalid"]) == (n_b, cand_b, bad_b), (name, ta_, ia_, n_b, cand_b, bad_b)
                assert np.array_equal(ea_, ids_b), name
            torch.cuda.synchronize()
            ta, tb = [], []
            for rep in range(args.reps):
                s = time.perf_counter()
                again = g.zone_store(poly, **q)                 # ends in the page's device-to-host copies: synchronous
                ta.append(1000 * (time.perf_counter() - s))
                assert again[0] == total and again[2].tobytes() == eids.tobytes()
                if not args.gpu_only and rep < paged_reps:
                    s = time.perf_counter()
                    paged(poly, q, asg_b)
                    tb.append(1000 * (time.perf_counter() - s))
                    print(f"{name}: repetition {rep + 1} of {args.reps}: (a) {ta[-1]:.2f} ms, (b) {tb[-1]:.0f} ms",
                          file=sys.stderr, flush=True)          # (b) takes seconds: show that the run is alive
            r = out["queries"][name] = {"candidates": info["candidates"], "invalid": info["invalid"], "matches": total,
                                        "gpu_ms_p50": round(float(np.median(ta)), 3),
                                        "gpu_ms_min": round(float(np.min(ta)), 3), "gpu_ms_max": round(float(np.max(ta)), 3)}
            if tb:
                r.update(paged_ms_p50=round(float(np.median(tb)), 1), paged_ms_min=round(float(np.min(tb)), 1),
                         paged_ms_max=round(float(np.max(tb)), 1), paged_assignments=int(len(asg_b)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
