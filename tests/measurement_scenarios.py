"""Shared scenarios for the measurement (threshold) rule tests, CPU and GPU."""
import numpy as np

from sitewhere_amd.models import wire
from sitewhere_amd.models.columnar import EV_ALERT, EV_MEASUREMENT
from sitewhere_amd.pipeline.engine_base import MeasurementTest
from sitewhere_amd.pipeline.fleet import hash64, pack_messages

from pipeline_scenarios import NOW

# the three rules of the fleet scenarios (fleet_batch names mx.metric0..7, values uniform in [0, 999.99])
FLEET_RULES = [MeasurementTest("mx.metric0", max=900.0),
               MeasurementTest("mx.metric3", min=100.0),
               MeasurementTest("mx.metric5", min=100.0, max=900.0, alert_type="metric5.range", alert_level=3)]

# boundary batch: with setup_fleet's two zone tests in front, these take test indices 2..6
HAND_RULES = [MeasurementTest("temp", max=20.0, alert_level=2),                       # 2
              MeasurementTest("hum", min=5.0, alert_type="hum.low", alert_level=0),   # 3
              MeasurementTest("absent", max=0.0),                                     # 4: no such measurement
              MeasurementTest("temp", max=10.0, alert_type="temp.high", alert_level=3),   # 5
              MeasurementTest("temp", min=19.995, alert_type="temp.low")]             # 6


def boundary_batch():
    """One message per device, devices ascending (the persist order is stable by assignment)."""
    msgs = [
        wire.location("dev-0000000000", 33.5, -84.5, event_date=NOW - 10),          # inside z1: zone.enter
        wire.measurements("dev-0000000001", {"temp": 20.0}, event_date=NOW - 9),    # on the bound: temp.high only
        wire.measurements("dev-0000000002", {"temp": 20.01}, event_date=NOW - 8),   # above: tests 2 and 5
        wire.measurements("dev-0000000003", {"temp": 19.99}, event_date=NOW - 7),   # below 19.995: 5 and 6
        wire.measurements("dev-0000000004", {"hum": 5.0}, event_date=NOW - 6),      # on the bound: nothing
        wire.measurements("dev-0000000005", {"hum": 4.99}, event_date=NOW - 5),     # below: test 3
        wire.measurements("dev-0000000006", {"hum": 5.01}, event_date=NOW - 4),     # above: nothing
        wire.measurements("dev-0000000007", {"temp": float("nan")}, event_date=NOW - 3),   # NaN never fires
        wire.measurements("dev-0000000008", {"other": 1e9, "temp": 5.0}, event_date=NOW - 2),  # temp 5.0: test 6
    ]
    return pack_messages(msgs)


# (assignment, alert type, level, test index) in emission order: row-major, test index ascending
BOUNDARY_ALERTS = [
    (0, "zone.enter", 2, 0),
    (1, "temp.high", 3, 5),
    (2, "temp.threshold", 2, 2), (2, "temp.high", 3, 5),
    (3, "temp.high", 3, 5), (3, "temp.low", 1, 6),
    (5, "hum.low", 0, 3),
    (8, "temp.low", 1, 6),
]


def intern_of(e) -> dict:
    return e.intern_table() if hasattr(e, "intern_table") else e.intern


def rows(e, res):
    """Outbound rows with names as hashes (each engine interns its own ids), in order."""
    inv = {i: h for h, i in intern_of(e).items()}
    o = res.out
    return [(int(o["etype"][i]), int(o["assignment"][i]), int(o["event_date"][i]), float(o["v0"][i]).hex(),
             float(o["v1"][i]).hex(), int(o["level"][i]), inv.get(int(o["name_id"][i]), 0)) for i in range(len(o))]


def alerts_of(e, res, n_gen):
    """(assignment, alert type, level) of the last ``n_gen`` (generated) rows, in order."""
    return [(r[1], e.names[r[6]], r[5]) for r in rows(e, res)[len(res.out) - n_gen:] if r[0] == EV_ALERT]


def count_hits(prec, rules) -> int:
    """Independent numpy count of measurement-test hits over decoded records of persisted rows."""
    p = prec[prec["etype"] == EV_MEASUREMENT]
    total = 0
    for t in rules:
        v = p["v0"][p["name_hash"] == np.uint64(hash64(t.measurement))]
        lo = -np.inf if t.min is None else t.min
        hi = np.inf if t.max is None else t.max
        total += int(((v < lo) | (v > hi)).sum())
    return total


def many_rules(n):
    """``n`` rules over fleet_batch's 8 names with varied bounds: several tests per name, so a row
    can fire several and (with 2 zone tests and n = 62) bit 63 is used."""
    out = []
    for i in range(n):
        name = f"mx.metric{i % 8}"
        k = i // 8
        if i % 3 == 0:
            out.append(MeasurementTest(name, max=500.0 + 60.0 * k, alert_type=f"r{i}.high", alert_level=i % 4))
        elif i % 3 == 1:
            out.append(MeasurementTest(name, min=400.0 - 45.0 * k, alert_type=f"r{i}.low", alert_level=i % 4))
        else:
            out.append(MeasurementTest(name, min=50.0 * (k + 1), max=950.0 - 50.0 * k, alert_type=f"r{i}.band",
                                       alert_level=i % 4))
    return out
