"""Location density grid: the host side of ``EngineBase.grid_store``.

A lat/lon box cut into ``n_rows`` x ``n_cols`` cells, each with the number of locations in it and the
newest of their dates.  ``grid_cell_np`` is the one cell formula every engine shares (the MI355X
kernel ``k_grid_count`` spells it in HIP): single correctly rounded fp64 operations, none contracted,
with the two steps computed once on the host, so a row lands in the same cell everywhere.
``grid_select`` is validity, the ``latest`` rule (``near.looked_at``, the near and zone queries' own)
and the histogram every route shares: the CPU engines' ``grid_store`` (the oracle of the kernel) and
``host_grid`` (events listed through event management) both go through it.

The box is closed on all sides.  ``lon_lo > lon_hi`` means it crosses the antimeridian, as
``near.near_box`` may: its width is then ``lon_hi - lon_lo + 360.0``.  Longitude -180 and 180 are the
same meridian and are not special-cased: in a box from -180 to 180 they are its first and its last
column; in a crossing box both are inside, with ``off`` = ``-180 - lon_lo + 360.0`` and ``180 - lon_lo``,
equal before rounding, so they share a cell unless those roundings part them at a cell boundary.
"""
from __future__ import annotations

import math

import numpy as np

from ..models.columnar import GRID_CELL
from .near import looked_at

GRID_MAX_CELLS = 65536               # SW_GRID_MAX_CELLS: the series query's limit


def check_grid_args(lat_lo, lat_hi, lon_lo, lon_hi, n_rows, n_cols, start=None, end=None):
    """``grid_store``'s argument checks: ((lat_lo, lat_hi, lon_lo, lon_hi) as floats, n_rows, n_cols), or
    ``ValueError``."""
    try:
        box = tuple(float(x) for x in (lat_lo, lat_hi, lon_lo, lon_hi))
        rows, cols = int(n_rows), int(n_cols)
        same = rows == n_rows and cols == n_cols
    except (TypeError, ValueError, OverflowError):
        raise ValueError("the box must be four numbers and the cell counts two integers") from None
    if not same:
        raise ValueError("rows and cols must be integers")
    if not all(math.isfinite(x) for x in box):
        raise ValueError("the box must be finite")
    lat_lo, lat_hi, lon_lo, lon_hi = box
    if not (-90.0 <= lat_lo < lat_hi <= 90.0):
        raise ValueError("latitudes must satisfy -90 <= latMin < latMax <= 90")
    if not (abs(lon_lo) <= 180.0 and abs(lon_hi) <= 180.0 and lon_lo != lon_hi):
        raise ValueError("longitudes must lie in [-180, 180] and differ")
    if rows < 1 or cols < 1:
        raise ValueError("rows and cols must be at least 1")
    if rows * cols > GRID_MAX_CELLS:
        raise ValueError(f"a grid has at most {GRID_MAX_CELLS} cells")
    if start is not None and end is not None and int(start) > int(end):
        raise ValueError("end is before start")
    return box, rows, cols


def grid_steps(box, n_rows: int, n_cols: int) -> tuple[float, float, bool]:
    """(d_lat, d_lon, crossing): the cell's height and width in degrees, each one subtraction (and, for a
    crossing box, one addition) and one division, and whether the box crosses the antimeridian."""
    lat_lo, lat_hi, lon_lo, lon_hi = box
    crossing = lon_lo > lon_hi
    width = lon_hi - lon_lo + 360.0 if crossing else lon_hi - lon_lo
    return (lat_hi - lat_lo) / n_rows, width / n_cols, crossing


def grid_cell_np(box, n_rows: int, n_cols: int, lats, lons):
    """(inside, row, col) of positions (arrays) in the grid: row 0 is the south edge, column 0 the
    ``lon_lo`` one.  ``int`` truncates a quotient that is never negative; the ``min`` puts the closed north
    and east edges, and any quotient that rounds up to the cell count, into the last row or column.
    Row and column of a position outside the box mean nothing."""
    lat_lo, lat_hi, lon_lo, lon_hi = box
    d_lat, d_lon, crossing = grid_steps(box, n_rows, n_cols)
    lats, lons = np.asarray(lats, np.float64), np.asarray(lons, np.float64)
    in_lon = (lons >= lon_lo) | (lons <= lon_hi) if crossing else (lons >= lon_lo) & (lons <= lon_hi)
    inside = (lats >= lat_lo) & (lats <= lat_hi) & in_lon
    la, lo = np.where(inside, lats, lat_lo), np.where(inside, lons, lon_lo)
    i = np.minimum(((la - lat_lo) / d_lat).astype(np.int64), n_rows - 1)
    off = lo - lon_lo
    off = np.where(off < 0, off + 360.0, off)               # only a crossing box gets here with off < 0
    j = np.minimum((off / d_lon).astype(np.int64), n_cols - 1)
    return inside, i, j


def grid_select(groups, dates, ids, lats, lons, box, n_rows: int, n_cols: int, latest: bool):
    """The histogram over candidate rows (parallel arrays; ``groups``: the row's assignment, any integer
    key).  Invalid positions are dropped and counted.  ``latest``: of each group only the valid row with
    the largest (date, id) is looked at.  Returns (``GRID_CELL`` cells of shape (n_rows, n_cols), invalid
    rows, valid looked-at rows outside the box)."""
    groups, dates, ids = np.asarray(groups, np.int64), np.asarray(dates, np.int64), np.asarray(ids, np.int64)
    idx, n_invalid = looked_at(groups, dates, ids, lats, lons, latest)
    inside, i, j = grid_cell_np(box, n_rows, n_cols, np.asarray(lats, np.float64)[idx], np.asarray(lons, np.float64)[idx])
    cell = (i * n_cols + j)[inside]
    d = dates[idx][inside]
    cells = np.zeros(n_rows * n_cols, GRID_CELL)
    cells["count"] = np.bincount(cell, minlength=n_rows * n_cols)
    newest = np.full(n_rows * n_cols, np.iinfo(np.int64).min, np.int64)
    np.maximum.at(newest, cell, d)
    cells["last_date"] = np.where(cells["count"] > 0, newest, 0)
    return cells.reshape(n_rows, n_cols), n_invalid, int(len(idx) - len(cell))


def grid_response(cells, info, box, hot_since=None) -> dict:
    """The one response shape of both routes: the non-empty cells only, in row-major order."""
    n_rows, n_cols = cells.shape
    d_lat, d_lon, _ = grid_steps(box, n_rows, n_cols)
    rr, cc = np.nonzero(cells["count"])
    return {"hotSince": hot_since, "numResults": int(cells["count"].sum()), "outside": int(info["outside"]),
            "invalid": int(info["invalid"]), "rows": n_rows, "cols": n_cols, "latStep": d_lat, "lonStep": d_lon,
            "cells": [{"row": int(r), "col": int(c), "count": int(cells["count"][r, c]),
                       "lastDate": int(cells["last_date"][r, c])} for r, c in zip(rr, cc)]}


def host_grid(locations, lat_lo, lat_hi, lon_lo, lon_hi, n_rows, n_cols, start=None, end=None, latest=False) -> dict:
    """The host route: listed location events (``latitude``, ``longitude``, ``event_date``,
    ``device_assignment_id``) counted by the same function as the hot route, in the same response shape
    (``hotSince`` None).  Ties at an equal date go by listing order, newest listed first."""
    box, n_rows, n_cols = check_grid_args(lat_lo, lat_hi, lon_lo, lon_hi, n_rows, n_cols, start, end)
    evs = [e for e in locations if e.event_date is not None and (start is None or e.event_date >= start) and
           (end is None or e.event_date <= end)]
    group = {}
    groups = [group.setdefault(e.device_assignment_id, len(group)) for e in evs]
    nan = float("nan")
    cells, n_invalid, n_outside = grid_select(groups, [e.event_date for e in evs], np.arange(len(evs), 0, -1),
                                              [nan if e.latitude is None else e.latitude for e in evs],
                                              [nan if e.longitude is None else e.longitude for e in evs], box, n_rows,
                                              n_cols, latest)
    return grid_response(cells, {"invalid": n_invalid, "outside": n_outside}, box)
