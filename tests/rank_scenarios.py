"""Shared scenarios of the ranking tests (CPU oracle and GPU engine): the rings of
``series_scenarios.fill_ring``, the query lists, the hand-built batch with its expected cells written out,
a brute-force loop independent of ``pipeline/rank.py`` and the comparison under the contract of
``EngineBase.rank_store``: bytes, there is no band."""
import struct

import numpy as np

from sitewhere_amd.models import wire
from sitewhere_amd.models.columnar import EV_ALERT, EV_LOCATION, EV_MEASUREMENT, EV_STATE_CHANGE, RANK_CELL
from sitewhere_amd.pipeline.engine_base import MeasurementTest
from sitewhere_amd.pipeline.fleet import hash64, pack_messages

from near_scenarios import SUB_RANGE, SUBSET
from pipeline_scenarios import NOW, setup_fleet
from series_scenarios import NAMES

GROUPS = ("assignment", "customer", "area", "asset")
COLUMN = {"assignment": "asg", "customer": "cust", "area": "area", "asset": "asset"}
STATS = ("count", "min", "max", "last")
INFO_KEYS = ["candidates", "rows", "nan", "ungrouped", "groups", "hot_since"]

# What the oracle finds on the rings for the measurement name NAMES[0], asserted by tests/test_rank.py so
# that no case goes empty: ring slots -> (rows, assignment groups, distinct counts among them).
RING_FACTS = {1 << 12: (315, 142, 6), 1 << 14: (983, 180, None)}
KEY_SETS = {"customer": 7, "area": 5, "asset": 3}


def ring_queries():
    """Every query of a ring as ``rank_store`` keyword arguments: every group, every stat, both directions,
    k in {1, 10, None} (value stats on NAMES[0]; counts over every measurement), then an assignment subset,
    a date sub-range, locations, state changes, and alerts with and without ``min_level`` and a type."""
    out = []
    for group in GROUPS:
        for stat in STATS:
            base = dict(event_type=EV_MEASUREMENT, group=group, stat=stat)
            if stat != "count":
                base["name_hash"] = NAMES[0]
            for ascending in (False, True):
                out += [dict(base, ascending=ascending, k=k) for k in (1, 10, None)]
        out.append(dict(event_type=EV_MEASUREMENT, group=group, stat="count", name_hash=NAMES[0], k=None))
        out.append(dict(event_type=EV_MEASUREMENT, group=group, stat="max", name_hash=NAMES[0], k=None, asg_idx=SUBSET))
        out.append(dict(event_type=EV_MEASUREMENT, group=group, stat="last", name_hash=NAMES[0], k=10,
                        start=SUB_RANGE[0], end=SUB_RANGE[1]))
        out.append(dict(event_type=EV_LOCATION, group=group, k=None))
        out.append(dict(event_type=EV_STATE_CHANGE, group=group, k=None))
        out.append(dict(event_type=EV_ALERT, group=group, k=None))
        out += [dict(event_type=EV_ALERT, group=group, k=10, min_level=lv, ascending=lv == 2) for lv in (0, 1, 2, 3)]
        out.append(dict(event_type=EV_ALERT, group=group, k=None, min_level=1, name_hash=hash64("zone.exit")))
    return out


def bits(v) -> int:
    return struct.unpack("<q", struct.pack("<d", v))[0]


def total_order_key(v) -> int:
    """An integer whose order is the IEEE total order of non-NaN doubles, written without the xor of
    ``rank_key``: the magnitude's bits, negated (and one lower) under the sign."""
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    return -(b & (2 ** 63 - 1)) - 1 if b >> 63 else b


def brute_force_rank(cols, eids, n_keys, event_type, group, stat="count", k=10, asg_idx=None, start=None, end=None,
                     name_hash=None, min_level=None, ascending=False):
    """Plain loop over ``store_rows()``: (cells, info without ``hot_since``)."""
    asg = None if asg_idx is None else set(asg_idx)
    cand = nan = ungrouped = rows = 0
    groups: dict = {}
    for r in range(len(eids)):
        if int(cols["etype"][r]) != event_type or (asg is not None and int(cols["asg"][r]) not in asg):
            continue
        d = int(cols["date"][r])
        if (start is not None and d < start) or (end is not None and d > end):
            continue
        if name_hash is not None and int(cols["name"][r]) != name_hash:
            continue
        if min_level is not None and int(cols["level"][r]) < min_level:
            continue
        cand += 1
        v = float(cols["v0"][r]) if event_type == EV_MEASUREMENT else 0.0
        if v != v:
            nan += 1
            continue
        key = int(cols[COLUMN[group]][r])
        if not 0 <= key < n_keys:
            ungrouped += 1
            continue
        rows += 1
        groups.setdefault(key, []).append((d, int(eids[r]), v))
    found = []
    for key, recs in groups.items():
        newest = max(recs, key=lambda t: t[:2])
        lo = min((t[2] for t in recs), key=total_order_key)
        hi = max((t[2] for t in recs), key=total_order_key)
        found.append((key, len(recs), lo, hi, newest[2], newest[0], newest[1]))
    col = {"count": 1, "min": 2, "max": 3, "last": 4}[stat]
    sign = 1 if ascending else -1
    found.sort(key=lambda c: (sign * (c[1] if stat == "count" else total_order_key(c[col])), c[0]))
    cells = np.array(found[:k], RANK_CELL) if found[:k] else np.zeros(0, RANK_CELL)
    return cells, {"candidates": cand, "rows": rows, "nan": nan, "ungrouped": ungrouped, "groups": len(found)}


def assert_same_rank(got, want):
    """``got`` against ``want`` (each (cells, info)): the cells' bytes and the info equal."""
    (cg, ig), (cw, iw) = got, want
    assert cg.dtype == cw.dtype == RANK_CELL and cg.ndim == 1
    assert ig == iw and list(ig) == INFO_KEYS
    if cg.tobytes() != cw.tobytes():
        assert len(cg) == len(cw), f"{len(cg)} cells, not {len(cw)}"
        bad = [i for i in range(len(cg)) if cg[i].tobytes() != cw[i].tobytes()]
        raise AssertionError(f"{len(bad)} cells differ, first at {bad[0]}: {cg[bad[0]]} != {cw[bad[0]]}")


def assert_conserved(cells, info, k):
    assert info["rows"] + info["nan"] + info["ungrouped"] == info["candidates"]
    assert len(cells) == (info["groups"] if k is None else min(k, info["groups"]))
    if k is None:
        assert int(cells["count"].sum()) == info["rows"]
    assert (cells["count"] > 0).all()


# ------------------------------------------------------------------------------ the hand batch
TEMP, HUM, VOLT = hash64("temp"), hash64("hum"), hash64("volt")
NO_CUSTOMER = 7                # the assignment whose customer is taken away
LEVEL_TYPES = {0: "hum.high", 1: "zone.exit", 2: "zone.enter", 3: "temp.high"}


def hand_rank_fleet(eng):
    """``setup_fleet``'s 1000 devices (customer d % 7, area d % 5, asset d % 3; zone alerts at levels 2 and
    1), assignment 7 without a customer, and two threshold rules that raise alerts at levels 3 and 0."""
    setup_fleet(eng, n_dev=1000)
    eng.set_assignments([NO_CUSTOMER], [NO_CUSTOMER], customer=None, area=NO_CUSTOMER % 5, asset=NO_CUSTOMER % 3)
    eng.set_measurement_rules([MeasurementTest("temp", max=100.0, alert_type=LEVEL_TYPES[3], alert_level=3),
                               MeasurementTest("hum", max=90.0, alert_type=LEVEL_TYPES[0], alert_level=0)])
    return eng


def hand_rank_batch():
    """Less than one wave of rows.  ``temp``: a NaN; -0.0 and +0.0 as the only values of assignments 2 and
    3; three rows of assignment 4 at one date (``last`` goes by event id); assignment 5's largest value
    equals assignment 4's; assignment 7 has no customer; assignment 6's 150.0 raises the level-3 alert.
    ``hum`` 95.0 raises the level-0 one, the two locations the level-2 (inside the zone) and level-1
    (outside) ones.  ``volt``: two negative values of assignment 14, which raw bits would order the wrong
    way round; under another name they leave the ``temp`` rankings to the zeros."""
    m = wire.measurements
    return pack_messages([
        m("dev-0000000001", {"temp": float("nan")}, event_date=NOW - 100),
        m("dev-0000000002", {"temp": -0.0}, event_date=NOW - 90),
        m("dev-0000000003", {"temp": 0.0}, event_date=NOW - 90),
        m("dev-0000000004", {"temp": 5.0}, event_date=NOW - 80),
        m("dev-0000000004", {"temp": 7.0}, event_date=NOW - 80),
        m("dev-0000000004", {"temp": 6.0}, event_date=NOW - 80),
        m("dev-0000000005", {"temp": 7.0}, event_date=NOW - 70),
        m("dev-0000000005", {"temp": 1.0}, event_date=NOW - 60),
        m("dev-0000000007", {"temp": 3.0}, event_date=NOW - 50),
        m("dev-0000000006", {"temp": 150.0}, event_date=NOW - 40),
        m("dev-0000000013", {"hum": 95.0}, event_date=NOW - 30),
        m("dev-0000000014", {"volt": -1.0}, event_date=NOW - 96),
        m("dev-0000000014", {"volt": -2.5}, event_date=NOW - 95),
        wire.location("dev-0000000011", 33.5, -84.5, event_date=NOW - 20),
        wire.location("dev-0000000012", 10.0, 10.0, event_date=NOW - 10),
    ])


HAND_ROWS = 19                 # 13 measurements, 2 locations, 4 rule alerts


def _cells(*rows):
    return np.array(list(rows), RANK_CELL) if rows else np.zeros(0, RANK_CELL)


def hand_eids(cols, eids):
    """The event id of the device-sent row of assignment ``a`` with value (or latitude) ``v``: the one thing
    the expectations take from the engine, which hands ids out in persist order, a step's rows clustered by
    assignment.  Assignment 4's three rows at one date must have kept their message order."""
    def eid(a, v):
        hit = [int(eids[r]) for r in range(len(eids)) if int(cols["etype"][r]) in (EV_MEASUREMENT, EV_LOCATION) and
               int(cols["asg"][r]) == a and bits(float(cols["v0"][r])) == bits(v)]
        assert len(hit) == 1, (a, v, hit)
        return hit[0]
    assert eid(4, 5.0) < eid(4, 7.0) < eid(4, 6.0)
    return eid


def hand_expected(eid):
    """[(query, cells, info without ``hot_since``)], written out by hand.  ``eid``: ``hand_eids``'s lookup."""
    eids = {1: eid(2, -0.0), 2: eid(3, 0.0), 5: eid(4, 6.0), 7: eid(5, 1.0), 8: eid(7, 3.0), 9: eid(6, 150.0),
            11: eid(11, 33.5), 12: eid(12, 10.0)}             # by the row's place in the batch
    T = dict(event_type=EV_MEASUREMENT, name_hash=TEMP)
    # (key, count, min, max, last, last_date, last_id) of the temp groups by assignment
    a2 = (2, 1, -0.0, -0.0, -0.0, NOW - 90, eids[1])
    a3 = (3, 1, 0.0, 0.0, 0.0, NOW - 90, eids[2])
    a4 = (4, 3, 5.0, 7.0, 6.0, NOW - 80, eids[5])            # three rows at one date: the largest event id is last
    a5 = (5, 2, 1.0, 7.0, 1.0, NOW - 60, eids[7])
    a6 = (6, 1, 150.0, 150.0, 150.0, NOW - 40, eids[9])
    a7 = (7, 1, 3.0, 3.0, 3.0, NOW - 50, eids[8])
    info = {"candidates": 10, "rows": 9, "nan": 1, "ungrouped": 0, "groups": 6}
    out = [
        # -0.0 ranks below +0.0
        (dict(T, group="assignment", stat="min", ascending=True, k=None), _cells(a2, a3, a5, a7, a4, a6), info),
        (dict(T, group="assignment", stat="min", k=2), _cells(a6, a4), info),
        # assignments 4 and 5 tie on max 7.0: the key decides, in both directions
        (dict(T, group="assignment", stat="max", k=3), _cells(a6, a4, a5), info),
        (dict(T, group="assignment", stat="max", ascending=True, k=None), _cells(a2, a3, a7, a4, a5, a6), info),
        # 2, 3, 6 and 7 tie on count 1
        (dict(T, group="assignment", stat="count", k=None), _cells(a4, a5, a2, a3, a6, a7), info),
        (dict(T, group="assignment", stat="count", ascending=True, k=1), _cells(a2), info),
        (dict(T, group="assignment", stat="last", k=None), _cells(a6, a4, a7, a5, a3, a2), info),
        # customers d % 7: assignment 7 has none, so its row is ungrouped
        (dict(T, group="customer", stat="max", k=None),
         _cells((6, 1, 150.0, 150.0, 150.0, NOW - 40, eids[9]), (4, 3, 5.0, 7.0, 6.0, NOW - 80, eids[5]),
                (5, 2, 1.0, 7.0, 1.0, NOW - 60, eids[7]), (3, 1, 0.0, 0.0, 0.0, NOW - 90, eids[2]),
                (2, 1, -0.0, -0.0, -0.0, NOW - 90, eids[1])),
         {"candidates": 10, "rows": 8, "nan": 1, "ungrouped": 1, "groups": 5}),
        # assets d % 3: 0 <- {3, 6}, 1 <- {4, 7}, 2 <- {2, 5}
        (dict(T, group="asset", stat="min", ascending=True, k=None),
         _cells((2, 3, -0.0, 7.0, 1.0, NOW - 60, eids[7]), (0, 2, 0.0, 150.0, 150.0, NOW - 40, eids[9]),
                (1, 4, 3.0, 7.0, 3.0, NOW - 50, eids[8])),
         {"candidates": 10, "rows": 9, "nan": 1, "ungrouped": 0, "groups": 3}),
        # every measurement name: hum and volt join (assignment 14 lies in area 4), the NaN still counts apart
        (dict(event_type=EV_MEASUREMENT, group="area", k=1), _cells((4, 5, -2.5, 7.0, 6.0, NOW - 80, eids[5])),
         {"candidates": 13, "rows": 12, "nan": 1, "ungrouped": 0, "groups": 5}),
        # negative values: -2.5 is the smallest, though its bits are the larger integer
        (dict(event_type=EV_MEASUREMENT, name_hash=VOLT, group="assignment", stat="min", k=None),
         _cells((14, 2, -2.5, -1.0, -2.5, NOW - 95, eid(14, -2.5))),
         {"candidates": 2, "rows": 2, "nan": 0, "ungrouped": 0, "groups": 1}),
        (dict(event_type=EV_LOCATION, group="assignment", k=None),
         _cells((11, 1, 0.0, 0.0, 0.0, NOW - 20, eids[11]), (12, 1, 0.0, 0.0, 0.0, NOW - 10, eids[12])),
         {"candidates": 2, "rows": 2, "nan": 0, "ungrouped": 0, "groups": 2}),
        (dict(event_type=EV_STATE_CHANGE, group="assignment", k=None), _cells(),
         {"candidates": 0, "rows": 0, "nan": 0, "ungrouped": 0, "groups": 0}),
    ]
    return out


# The four rule alerts are dated by the step: (assignment that raised it) per level.
HAND_ALERT_ASG = {0: 13, 1: 12, 2: 11, 3: 6}
