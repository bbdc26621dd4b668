"""Measurement series in time buckets: the host reduction.

One point per (measurement name, time bucket) instead of one per event.  ``bucket_series`` is the
reference reduction: the CPU engines' ``aggregate_store`` (the oracle of the MI355X kernels) and the
REST handler's host route (events listed through event management) both go through it, so every
route fills a cell the same way.  Cells are ``SERIES_CELL`` records (``models/columnar.py``).
"""
from __future__ import annotations

import math

import numpy as np

from ..models.columnar import SERIES_CELL, SERIES_MAX_CELLS, SERIES_MAX_NAMES


def series_buckets(n_names: int, start: int, end: int, bucket_ms: int) -> int:
    """Number of buckets of a query, or ``ValueError``: the argument checks every route shares."""
    if bucket_ms < 1:
        raise ValueError("bucket_ms must be at least 1")
    if end < start:
        raise ValueError("end is before start")
    if n_names < 1:
        raise ValueError("no measurement names")
    if n_names > SERIES_MAX_NAMES:
        raise ValueError(f"more than {SERIES_MAX_NAMES} measurement names in one query")
    n_buckets = (end - start) // bucket_ms + 1
    if n_names * n_buckets > SERIES_MAX_CELLS:
        raise ValueError(f"{n_names} names x {n_buckets} buckets exceed {SERIES_MAX_CELLS} cells")
    return n_buckets


def check_series_args(name_hashes, start: int, end: int, bucket_ms: int) -> tuple[list[int], int]:
    """``aggregate_store``'s argument checks: (name hashes as ints, n_buckets)."""
    names = [int(h) for h in name_hashes]
    n_buckets = series_buckets(len(names), int(start), int(end), int(bucket_ms))
    if len(set(names)) != len(names):
        raise ValueError("duplicate measurement names")
    return names, n_buckets


def bucket_series(name_idx, dates, ids, values, start: int, bucket_ms: int, n_names: int, n_buckets: int):
    """Reduce rows into cells.  ``name_idx`` (position of the row's name, 0 .. n_names - 1), ``dates``
    (start <= date, within the buckets), ``ids`` (the first / last tie-break at equal dates) and
    ``values`` are parallel arrays.  Rows whose value is NaN are skipped.  ``sum`` is ``math.fsum`` of
    the cell's values: correctly rounded.  Returns (cells [n_names, n_buckets], NaN rows skipped)."""
    cells = np.zeros((n_names, n_buckets), SERIES_CELL)
    values = np.asarray(values, np.float64)
    ok = ~np.isnan(values)
    n_nan = int(len(values) - ok.sum())
    values = values[ok]
    if not len(values):
        return cells, n_nan
    dates = np.asarray(dates, np.int64)[ok]
    ids = np.asarray(ids, np.int64)[ok]
    cell = np.asarray(name_idx, np.int64)[ok] * n_buckets + (dates - int(start)) // int(bucket_ms)
    order = np.lexsort((ids, dates, cell))
    cell, dates, ids, values = cell[order], dates[order], ids[order], values[order]
    lo = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
    hi = np.r_[lo[1:], len(cell)] - 1
    flat = cells.reshape(-1)
    at = cell[lo]
    flat["count"][at] = hi - lo + 1
    flat["min"][at] = np.minimum.reduceat(values, lo)
    flat["max"][at] = np.maximum.reduceat(values, lo)
    with np.errstate(invalid="ignore"):
        flat["sum"][at] = [_fsum(values[a:b + 1]) for a, b in zip(lo, hi)]
    for side, pos in (("first", lo), ("last", hi)):
        flat[side][at] = values[pos]
        flat[side + "_date"][at] = dates[pos]
        flat[side + "_id"][at] = ids[pos]
    return cells, n_nan


def _fsum(v) -> float:
    try:
        return math.fsum(v)
    except (OverflowError, ValueError):      # an intermediate overflow, or +inf and -inf together
        return float(np.sum(v))


def series_entries(row, start: int, bucket_ms: int) -> list[dict]:
    """A name's non-empty cells as the entries of a bucketed-series response, oldest bucket first."""
    out = []
    for b in np.flatnonzero(row["count"]):
        c = row[b]
        n = int(c["count"])
        out.append({"bucketStart": int(start) + int(b) * int(bucket_ms), "count": n, "min": float(c["min"]),
                    "max": float(c["max"]), "mean": float(c["sum"]) / n, "first": float(c["first"]),
                    "last": float(c["last"]), "firstDate": int(c["first_date"]), "lastDate": int(c["last_date"])})
    return out


def host_series(measurements, want, start: int, end: int, bucket_ms: int) -> list[dict]:
    """The host route: bucket listed measurement events (``name``, ``value``, ``event_date``) whose
    name is in ``want`` (None: every name listed).  Ties at an equal date go by listing order."""
    ms = [m for m in measurements if m.event_date is not None and start <= m.event_date <= end and
          (want is None or m.name in want)]
    names = sorted({m.name for m in ms})
    out = []
    for k in range(0, len(names), SERIES_MAX_NAMES):
        chunk = names[k:k + SERIES_MAX_NAMES]
        pos = {n: i for i, n in enumerate(chunk)}
        sel = [m for m in ms if m.name in pos]
        n_buckets = series_buckets(len(chunk), start, end, bucket_ms)
        cells, _ = bucket_series([pos[m.name] for m in sel], [m.event_date for m in sel], np.arange(len(sel)),
                                 [m.value for m in sel], start, bucket_ms, len(chunk), n_buckets)
        out += [{"measurementId": n, "entries": series_entries(cells[i], start, bucket_ms)} for n, i in pos.items()]
    return [s for s in out if s["entries"]]
