"""Locations near a point over a full HBM event ring.

Fills a 2^27-event ring on the MI355X with the bench.py fleet (as scripts/bench_hot_series.py does),
whose locations spread over lat 33.75 - 34.25, lon -84.39 - -83.89, then times, tenant-wide from the
middle of that square, a 1 km, a 25 km and a 250 km radius and one ``latest=True`` query (25 km):

  (a) ``near_store`` on the GPU: scan, box test, haversine and ordering in HBM, only the page (100 rows)
      and its distances cross PCIe;
  (b) the route there was before it: ``query_store(EV_LOCATION, every assignment, page_size=0)`` (every
      location row, all 16 columns, crosses PCIe) followed by ``near.near_select`` on the host.

(a) and (b) alternate within each repetition, so both see the same machine; ``--paged-reps`` bounds how
many of the repetitions also run (b), which takes seconds per call.  Before any time is taken (a) is
checked against (b) under the contract of ``EngineBase.near_store``: a row within ``NEAR_BAND_M`` of the
radius may fall either way, every other row agrees, page distances within the band.

    python scripts/bench_hot_near.py --store 134217728
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
    args = ap.parse_args()
    import torch

    from sitewhere_amd.models.columnar import EV_LOCATION
    from sitewhere_amd.pipeline.config import EngineConfig
    from sitewhere_amd.pipeline.fleet import FleetSpec, fingerprints, gen_payloads, gen_tokens
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine
    from sitewhere_amd.pipeline.near import NEAR_BAND_M, haversine_np, near_select, valid_position

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
    centre = (spec.lat0 + spec.span_deg / 2, spec.lon0 + spec.span_deg / 2)
    queries = {"1 km": dict(radius_m=1000.0), "25 km": dict(radius_m=25000.0), "250 km": dict(radius_m=250000.0),
               "25 km, latest": dict(radius_m=25000.0, latest=True)}
    every = np.asarray(d, np.int64)
    paged_reps = args.reps if args.paged_reps is None else min(args.paged_reps, args.reps)

    def gpu(q):
        return g.near_store(centre[0], centre[1], **q)

    def paged(q):
        """(b): every location row to the host, the row test and the ordering there; (total, page ids,
        page distances, every candidate's distance)."""
        _, cols, eids = g.query_store(EV_LOCATION, every, page_size=0)
        sel, dist, _ = near_select(cols["asg"], cols["date"], eids, cols["v0"], cols["v1"], centre[0], centre[1],
                                   q["radius_m"], q.get("latest", False), "date")
        return len(sel), eids[sel[:100]], dist[:100], cols

    out = {"store_events": int(min(g.cursor, args.store)), "fill_s": round(fill_s, 1), "centre": centre,
           "reps": args.reps, "paged_reps": 0 if args.gpu_only else paged_reps, "queries": {}}
    for name, q in queries.items():
        total, cols, eids, dist, info = gpu(q)              # warm (buffers, code objects)
        worst = None
        if not args.gpu_only:
            n_b, ids_b, dist_b, all_cols = paged(q)
            ok = valid_position(all_cols["v0"], all_cols["v1"])
            every_d = haversine_np(centre[0], centre[1], all_cols["v0"][ok], all_cols["v1"][ok])
            in_band = int((np.abs(every_d - q["radius_m"]) <= NEAR_BAND_M).sum())
            assert abs(total - n_b) <= in_band, (name, total, n_b, in_band)
            assert info["candidates"] == len(ok) and info["invalid"] == int(len(ok) - ok.sum()), name
            if in_band == 0:
                assert np.array_equal(eids, ids_b), name
                worst = float(np.abs(dist - dist_b).max()) if len(dist) else 0.0
                assert worst <= NEAR_BAND_M, (name, worst)
            del all_cols, every_d
        torch.cuda.synchronize()
        ta, tb = [], []
        for rep in range(args.reps):
            s = time.perf_counter()
            again = gpu(q)                                  # ends in the page's device-to-host copies: synchronous
            ta.append(1000 * (time.perf_counter() - s))
            assert again[0] == total and again[2].tobytes() == eids.tobytes() and again[3].tobytes() == dist.tobytes()
            if not args.gpu_only and rep < paged_reps:
                s = time.perf_counter()
                paged(q)
                tb.append(1000 * (time.perf_counter() - s))
                print(f"{name}: repetition {rep + 1} of {args.reps}: (a) {ta[-1]:.2f} ms, (b) {tb[-1]:.0f} ms",
                      file=sys.stderr, flush=True)          # (b) takes seconds: show that the run is alive
        r = out["queries"][name] = {"candidates": info["candidates"], "invalid": info["invalid"], "matches": total,
                                    "page_worst_abs_err_m": worst,
                                    "gpu_ms_p50": round(float(np.median(ta)), 3), "gpu_ms_min": round(float(np.min(ta)), 3),
                                    "gpu_ms_max": round(float(np.max(ta)), 3)}
        if tb:
            r.update(paged_ms_p50=round(float(np.median(tb)), 1), paged_ms_min=round(float(np.min(tb)), 1),
                     paged_ms_max=round(float(np.max(tb)), 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
