"""Shared scenarios of the location density-grid tests (CPU oracle and GPU engine): the rings of
``series_scenarios.fill_ring``, the boxes and grids, the query cases, the hand-built batch, a brute-force
loop independent of ``pipeline/grid.py`` and the comparison under the contract of
``EngineBase.grid_store``: bytes, there is no band."""
import math

import numpy as np

from sitewhere_amd.models import wire
from sitewhere_amd.models.columnar import EV_LOCATION, GRID_CELL
from sitewhere_amd.pipeline.fleet import pack_messages

from near_scenarios import SUB_RANGE, SUBSET, hand_near_batch  # noqa: F401  (re-exported)
from pipeline_scenarios import NOW

# (lat_lo, lat_hi, lon_lo, lon_hi).  The fleet's locations lie in lat 32.80 - 34.30, lon -85.20 - -83.70.
AROUND = (31.5, 35.5, -86.5, -82.5)        # the whole fleet: 8 x 8 leaves the outer two rows and columns empty
CUT = (33.2, 34.0, -84.9, -84.1)           # cuts through the fleet: rows on every side of it are outside
CROSSING = (31.5, 35.5, 170.0, -84.5)      # crosses the antimeridian and cuts the fleet: every row has off < 0
BOXES = {"around": AROUND, "cut": CUT, "crossing": CROSSING}


def case_queries(box, n_rows, n_cols):
    """Every query of one grid as ``grid_store`` keyword arguments: plain, an assignment subset and a date
    sub-range, each without and with ``latest``."""
    out = []
    for latest in (False, True):
        base = dict(lat_lo=box[0], lat_hi=box[1], lon_lo=box[2], lon_hi=box[3], n_rows=n_rows, n_cols=n_cols,
                    latest=latest)
        out += [base, dict(base, asg_idx=SUBSET), dict(base, start=SUB_RANGE[0], end=SUB_RANGE[1])]
    return out


def _edge(x, up):
    return math.nextafter(x, math.inf if up else -math.inf)


# The hand box and its 2 x 2 grid: steps of exactly 0.5 degree, so 33.5 and -84.5 are the interior boundaries.
HAND_BOX = (33.0, 34.0, -85.0, -84.0)
# A 1 x 4 grid across the antimeridian: 0.004 degree wide, 0.001 a column.
HAND_CROSSING = (-1.0, 1.0, 179.998, -179.998)


def hand_grid_batch():
    """``near_scenarios.hand_near_batch``'s dozen rows (a tie by event id at (33.5, -84.5), exactly on both
    interior boundaries of HAND_BOX's 2 x 2 grid; both sides of the antimeridian; beside the pole; three
    invalid rows) and nine more on the 1000-device fleet (devices 9 and 19 are unassigned and not used):
    one on an interior column boundary, one on each edge of HAND_BOX and one an ulp outside each."""
    raw, offs = hand_near_batch()
    rows = [
        (11, 33.25, -84.5, NOW - 40),                        # on the boundary between the columns: the eastern one
        (12, 34.0, -84.75, NOW - 41),                        # north edge: the quotient is the row count, clamped
        (13, 33.0, -84.25, NOW - 42),                        # south edge
        (14, _edge(34.0, True), -84.5, NOW - 43),            # an ulp outside: north, south, west, east
        (15, _edge(33.0, False), -84.5, NOW - 44),
        (16, 33.75, _edge(-85.0, False), NOW - 45),
        (17, 33.75, _edge(-84.0, True), NOW - 46),
        (18, 33.75, -84.0, NOW - 47),                        # east edge: clamped into the last column
        (20, 33.75, -85.0, NOW - 48),                        # west edge (device 19 is unassigned)
    ]
    more = [wire.location(f"dev-{d:010d}", la, lo, event_date=t) for d, la, lo, t in rows]
    msgs = [bytes(raw[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)] + more
    return pack_messages(msgs)


def _cells(rows, cols, filled):
    c = np.zeros((rows, cols), GRID_CELL)
    for (i, j), v in filled.items():
        c[i, j] = v
    return c


# Written out by hand: (box, rows, cols, latest) -> (cells as {(row, col): (count, last_date)}, outside).
# 21 candidates, 3 of them invalid, 16 assignments with a valid one, throughout.
HAND_INFO = {"candidates": 21, "invalid": 3}
HAND_EXPECTED = [
    # plain: (1, 1) holds device 1's two rows at (33.5, -84.5) and 33.5001, device 8's valid row and the
    # east-edge row; (1, 0) device 2's older row (lon -84.5002), the north-edge and the west-edge rows;
    # (0, 1) the column-boundary and the south-edge rows.  Outside: device 2's newest row, devices 3, 4,
    # 5 and 10, and the four rows an ulp out.
    (HAND_BOX, 2, 2, False, {(0, 1): (2, NOW - 40), (1, 0): (3, NOW - 41), (1, 1): (4, NOW - 47)}, 9),
    # latest: device 1 counts once (the later event id, 33.5001), device 2's newest row is outside, device
    # 8's newest valid row is the one older than its NaN
    (HAND_BOX, 2, 2, True, {(0, 1): (2, NOW - 40), (1, 0): (2, NOW - 41), (1, 1): (3, NOW - 47)}, 9),
    (HAND_BOX, 1, 1, False, {(0, 0): (9, NOW - 40)}, 9),
    # device 3 at lon 179.9995: off 0.0015, column 1; device 4 at -179.9995: off -359.9975 + 360, column 2
    (HAND_CROSSING, 1, 4, False, {(0, 1): (1, NOW - 30), (0, 2): (1, NOW - 31)}, 16),
    (HAND_CROSSING, 1, 4, True, {(0, 1): (1, NOW - 30), (0, 2): (1, NOW - 31)}, 14),
]


def hand_expected():
    return [(box, r, c, latest, _cells(r, c, filled), outside) for box, r, c, latest, filled, outside in HAND_EXPECTED]


def brute_force_grid(cols, eids, lat_lo, lat_hi, lon_lo, lon_hi, n_rows, n_cols, asg_idx=None, start=None, end=None,
                     latest=False):
    """Plain loop over ``store_rows()`` in Python floats: (cells, candidates, invalid, outside, assignments
    that have a valid candidate)."""
    asg = None if asg_idx is None else set(asg_idx)
    cand, invalid, valid = 0, 0, []
    for r in range(len(eids)):
        if int(cols["etype"][r]) != EV_LOCATION or (asg is not None and int(cols["asg"][r]) not in asg):
            continue
        d = int(cols["date"][r])
        if (start is not None and d < start) or (end is not None and d > end):
            continue
        cand += 1
        la, lo = float(cols["v0"][r]), float(cols["v1"][r])
        if not (math.isfinite(la) and math.isfinite(lo) and abs(la) <= 90 and abs(lo) <= 180):
            invalid += 1
            continue
        valid.append((int(cols["asg"][r]), d, int(eids[r]), la, lo))
    n_asg = len({v[0] for v in valid})
    if latest:
        newest = {}
        for v in valid:
            if v[0] not in newest or v[1:3] > newest[v[0]][1:3]:
                newest[v[0]] = v
        valid = list(newest.values())
    crossing = lon_lo > lon_hi
    width = (lon_hi - lon_lo) + 360.0 if crossing else lon_hi - lon_lo
    d_lat, d_lon = (lat_hi - lat_lo) / n_rows, width / n_cols
    cells = np.zeros((n_rows, n_cols), GRID_CELL)
    outside = 0
    for _, d, _, la, lo in valid:
        in_lon = (lo >= lon_lo or lo <= lon_hi) if crossing else (lon_lo <= lo <= lon_hi)
        if not (lat_lo <= la <= lat_hi and in_lon):
            outside += 1
            continue
        i = min(int((la - lat_lo) / d_lat), n_rows - 1)
        off = lo - lon_lo
        if off < 0:
            off = off + 360.0
        j = min(int(off / d_lon), n_cols - 1)
        n, last = int(cells[i, j]["count"]), int(cells[i, j]["last_date"])
        cells[i, j] = (n + 1, d if n == 0 else max(last, d))
    return cells, cand, invalid, outside, n_asg


def assert_same_grid(got, want):
    """``got`` against ``want`` (each (cells, info)): the cells' bytes and the info equal."""
    (cg, ig), (cw, iw) = got, want
    assert cg.dtype == cw.dtype == GRID_CELL and cg.shape == cw.shape
    assert ig == iw and list(ig) == ["candidates", "invalid", "outside", "hot_since"]
    if cg.tobytes() != cw.tobytes():
        bad = np.argwhere((cg["count"] != cw["count"]) | (cg["last_date"] != cw["last_date"]))
        raise AssertionError(f"{len(bad)} cells differ, first {bad[0].tolist()}: {cg[tuple(bad[0])]} != {cw[tuple(bad[0])]}")
    assert not cg[cg["count"] == 0].tobytes().strip(b"\0")           # an empty cell is all zero


def assert_conserved(cells, info, latest, n_asg_valid=None):
    """The contract's conservation, both forms."""
    total = int(cells["count"].sum())
    if latest:
        assert n_asg_valid is None or total + info["outside"] == n_asg_valid
    else:
        assert total + info["outside"] + info["invalid"] == info["candidates"]
