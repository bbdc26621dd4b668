"""Cost of measurement (threshold) tests in the engine stage, at the benchmark's shape.

The engine stage alone (decode + process on device-resident batches, rows kept in HBM; no bus, no
durable store) with the fleet, sizing and 16 zone tests of ``bench.py``, run with 0 and with 16
measurement tests.  The two configurations alternate in one process (``--rounds`` blocks each): a
block sets the rules, runs ``--warmup`` untimed steps (the process graph is re-captured on a rule
change) and then its share of the ``--steps`` timed steps.  Every timed step is a host clock around
``step_async`` + a device synchronise; its batch gets fresh alternate ids and is copied to the
device before the clock starts.  Prints one JSON line.  Needs an MI355X: fails without one.

    python scripts/bench_measurement_rules.py [--steps 200] [--warmup 5] [--rounds 4] [--configs 0,16]

Kernel times come from a separate run under ``rocprofv3 --kernel-trace --stats`` (one configuration,
few steps: ``--configs 16 --rounds 1 --steps 20``); ``k_mx_mask_bytes`` below is what the kernel has
to move per step, to set against its kernel time there.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def zone_polys(n, lat0, lon0, span, rng):
    """The benchmark's zones (bench.py zone_polys): n 32-gons, one "inside" test each."""
    from sitewhere_amd.pipeline.engine_base import Zone, ZoneTest
    zones, tests = [], []
    for z in range(n):
        cx, cy = lat0 + rng.uniform(0.1, 0.9) * span, lon0 + rng.uniform(0.1, 0.9) * span
        r = span * 0.08
        k = 32
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = r * rng.uniform(0.6, 1.0, k)
        verts = [(cx + rad[i] * np.cos(ang[i]), cy + rad[i] * np.sin(ang[i])) for i in range(k)]
        zones.append(Zone(f"zone-{z}", verts))
        tests.append(ZoneTest(f"zone-{z}", "inside", f"zone.{z}.enter", 2, "entered restricted zone"))
    return zones, tests


def measurement_tests(n, n_names=16):
    """n tests over the fleet's measurement names (values uniform in [0, 999.99]): each fires on
    ~2 % of its name's rows, as a threshold alert would."""
    from sitewhere_amd.pipeline.engine_base import MeasurementTest
    return [MeasurementTest(f"mx.metric{i % n_names}", min=10.0, max=990.0, alert_type=f"mx.{i}.range", alert_level=1)
            for i in range(n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="timed steps per configuration")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps at the start of every block")
    ap.add_argument("--rounds", type=int, default=4, help="blocks per configuration (alternating)")
    ap.add_argument("--configs", default="0,16", help="measurement-test counts to compare")
    ap.add_argument("--msgs", type=int, default=1 << 20)
    ap.add_argument("--devices", type=int, default=1 << 20)
    ap.add_argument("--zones", type=int, default=16)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--store", type=int, default=1 << 27)
    ap.add_argument("--dedup-filter-ids", type=int, default=(1 << 29) - (1 << 22))
    args = ap.parse_args()
    configs = [int(x) for x in args.configs.split(",")]

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_measurement_rules.py needs an MI355X (no GPU visible): nothing measured")
    from sitewhere_amd.pipeline.config import EngineConfig
    from sitewhere_amd.pipeline.fleet import (FleetSpec, alt_positions, fingerprints, gen_payloads, gen_tokens,
                                              stamp_positions)
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

    dev = torch.device("cuda", 0)
    # bench.py's fleet and engine sizing at --gpus 1
    spec = FleetSpec(prefix="dev-", n_devices=args.devices, p_location=0.25, p_alert=0.05, p_unregistered=0.005,
                     mx_per_msg=1, n_names=16, with_alternate_id=True, lat0=33.0, lon0=-85.0, span_deg=2.0,
                     p_register=0.0005, p_ack=0.0005, p_meta=0.1, alt_base=0)
    cfg = EngineConfig(max_msgs=args.msgs, rec_cap=args.msgs + 4096, gen_cap=max(1 << 16, args.msgs // 2),
                       max_devices=int(args.devices * 1.1) + 1024, max_assignments=int(args.devices * 1.1) + 1024,
                       store_cap=args.store, dedup_slots=1 << 24, name_slots=1 << 12,
                       dedup_filter_ids=args.dedup_filter_ids, dedup_filter_gens=4,
                       state_slots=2 * (16 + 4 + args.zones + max(configs)) * int(args.devices * 1.1),
                       presence_missing_ms=8 * 3600 * 1000)
    eng = GpuInboundEngine(cfg, device=dev)
    heap, offs = gen_tokens("dev-", 0, args.devices)
    lo, hi = fingerprints(heap, offs)
    d = eng.register_devices(lo, hi)
    eng.set_assignments(d, d, customer=d % 97, area=d % 31, asset=d % 1009)
    zones, ztests = zone_polys(args.zones, spec.lat0, spec.lon0, spec.span_deg, np.random.default_rng(1234))
    eng.set_zone_rules(zones, ztests)

    now0 = 1_700_000_000_000
    host, devb = [], []
    for b in range(args.batches):
        raw, off = gen_payloads(spec, args.msgs, now0 - 30_000, seed=1 + b)
        raw = np.concatenate([raw, np.zeros(64, np.uint8)])
        pin = torch.from_numpy(raw).pin_memory()
        host.append((pin, off, alt_positions(pin.numpy(), off)))
        devb.append((torch.empty_like(pin, device=dev), torch.from_numpy(off.view(np.int32)).to(dev)))

    k = [0]

    def step(timed: bool) -> float:
        i = k[0] % args.batches
        pin, off, pos = host[i]
        stamp_positions(pin.numpy(), pos, (0x5717 << 48) | k[0], threads=8)     # fresh alternate ids
        devb[i][0].copy_(pin, non_blocking=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.step_async(devb[i][0], devb[i][1], len(off) - 1, now0 + k[0], presence=False, out_to_device=True)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        k[0] += 1
        return dt

    times = {c: [] for c in configs}
    shape = {}
    per_block = -(-args.steps // args.rounds)
    for _ in range(args.rounds):
        for c in configs:
            if c or eng.__dict__.get("mtests"):
                eng.set_measurement_rules(measurement_tests(c))
            for _ in range(args.warmup):
                step(False)
            before = eng.stats_dict()
            for _ in range(per_block):
                times[c].append(step(True))
            after = eng.stats_dict()
            # the rows of the block's last step, for the bytes k_mx_mask has to move
            sc = eng.t["scalars"].cpu().numpy().view(np.uint32)
            n_ok = int(sc[4])
            c0 = int(eng.t["cursor"][1].item())
            rows = (c0 + torch.arange(n_ok, device=dev)) % cfg.store_cap
            n_mx = int((eng.store["etype"][rows] == 0).sum().item())
            fired = int(((eng.t["zmask"][:n_ok] >> args.zones) != 0).sum().item()) if c else 0
            shape[c] = {"persisted_device_rows": n_ok, "measurement_rows": n_mx, "rows_fired": fired,
                        "rule_alerts_per_step": (after["rule_alerts"] - before["rule_alerts"]) / per_block,
                        "events_per_step": (after["events"] - before["events"]) / per_block,
                        # etype of every row, name + v0 of measurement rows, zmask read-modify-write of
                        # the rows that fired (after k_zone_mask; alone it writes every row's mask)
                        "k_mx_mask_bytes": (n_ok + 16 * n_mx + (16 * fired if args.zones else 8 * n_ok)) if c else 0}
    out = {"metric": "engine_stage_step_ms", "msgs_per_step": args.msgs, "zone_tests": args.zones,
           "timed_steps_per_config": per_block * args.rounds, "warmup_per_block": args.warmup, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "configs": {}}
    for c in configs:
        t = np.asarray(times[c]) * 1e3
        out["configs"][str(c)] = {"measurement_tests": c, "mean_ms": round(float(t.mean()), 4),
                                  "median_ms": round(float(np.median(t)), 4),
                                  "p10_ms": round(float(np.percentile(t, 10)), 4),
                                  "p90_ms": round(float(np.percentile(t, 90)), 4),
                                  "events_per_s": round(shape[c]["events_per_step"] / (float(np.median(t)) / 1e3)),
                                  **shape[c]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
