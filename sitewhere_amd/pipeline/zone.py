"""Locations in a zone: the host side of ``EngineBase.zone_store``.

``contains_np`` is ``core/geo.contains`` for arrays (the MI355X kernel ``k_zone_filter`` spells the
same crossing test in HIP, division form, fp64); ``zone_select`` is validity, the ``latest`` rule,
the containment and the ordering every route shares: the CPU engines' ``zone_store`` (the oracle of
the kernel) and ``host_zone`` (events listed through event management) both go through it.

The polygon is planar in (lat, lon), as the reference's JTS test and this engine's zone rules treat
it: a zone that crosses the antimeridian is not special-cased.
"""
from __future__ import annotations

import numpy as np

from .near import looked_at

ZONE_MAX_VTX = 1024                  # SW_ZONE_MAX_VTX: the kernel's vertex table is 16 B a vertex in 16 KiB of LDS
ZONE_LAT_PAD = 1e-9                  # degrees; see zone_box


def check_zone_args(polygon, start=None, end=None, max_vtx: int | None = ZONE_MAX_VTX) -> np.ndarray:
    """``zone_store``'s argument checks: the polygon as a contiguous (N, 2) float64 array of (lat, lon)
    vertices, or ``ValueError``.  ``max_vtx`` None: no upper limit (the host route has none)."""
    try:
        poly = np.ascontiguousarray(polygon, np.float64)
    except (TypeError, ValueError):
        raise ValueError("polygon must be an (N, 2) array of (lat, lon) vertices") from None
    if poly.ndim != 2 or poly.shape[1] != 2:
        raise ValueError("polygon must be an (N, 2) array of (lat, lon) vertices")
    if len(poly) < 3:
        raise ValueError("a zone needs at least 3 vertices")
    if max_vtx is not None and len(poly) > max_vtx:
        raise ValueError(f"a zone has at most {max_vtx} vertices")
    if not (np.isfinite(poly).all() and (np.abs(poly[:, 0]) <= 90.0).all() and (np.abs(poly[:, 1]) <= 180.0).all()):
        raise ValueError("zone vertices must be finite, latitude in [-90, 90], longitude in [-180, 180]")
    if start is not None and end is not None and int(start) > int(end):
        raise ValueError("end is before start")
    return poly


def contains_np(polygon, lats, lons) -> np.ndarray:
    """``core/geo.contains`` for arrays of points: the same fp64 operations in the same order, so the
    same answer for every point, on an edge or a vertex too.  The division is evaluated for edges that
    do not cross as well (a horizontal one divides by zero) and masked out."""
    poly = np.asarray(polygon, np.float64)
    lats, lons = np.asarray(lats, np.float64), np.asarray(lons, np.float64)
    inside = np.zeros(lats.shape, bool)
    j = len(poly) - 1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(len(poly)):
            xi, yi = poly[i]
            xj, yj = poly[j]
            inside ^= ((yi > lons) != (yj > lons)) & (lats < (xj - xi) * (lons - yi) / (yj - yi) + xi)
            j = i
    return inside


def zone_box(polygon) -> tuple[float, float, float, float]:
    """A box (lat_lo, lat_hi, lon_lo, lon_hi), edges included, that excludes only points the predicate
    calls outside.  Longitude: the exact min / max of the vertices -- beyond them ``(yi > lon) !=
    (yj > lon)`` is false for every edge, by comparisons alone.  Latitude: an edge that crosses in
    longitude counts when ``lat < (xj - xi) * (lon - yi) / (yj - yi) + xi``; the exact intersection
    lies between xi and xj, the computed one carries six roundings (2^-53 relative each) of a term of
    at most 180 and one of the sum, under 1e-12 degree in all.  So above ``max(lat) + 1e-9`` no edge
    counts, and below ``min(lat) - 1e-9`` every crossing edge counts, which on a closed ring is an even
    number of them: outside both ways.  1e-9 degree (0.1 mm, what ``near_box`` pads) is a thousand
    times that error and still a box as tight as the data.  Clamped to [-90, 90]."""
    poly = np.asarray(polygon, np.float64)
    return (max(float(poly[:, 0].min()) - ZONE_LAT_PAD, -90.0), min(float(poly[:, 0].max()) + ZONE_LAT_PAD, 90.0),
            float(poly[:, 1].min()), float(poly[:, 1].max()))


def in_zone_box(box, lats, lons) -> np.ndarray:
    lat_lo, lat_hi, lon_lo, lon_hi = box
    lats, lons = np.asarray(lats, np.float64), np.asarray(lons, np.float64)
    return (lats >= lat_lo) & (lats <= lat_hi) & (lons >= lon_lo) & (lons <= lon_hi)


def zone_select(groups, dates, ids, lats, lons, polygon, outside: bool, latest: bool):
    """The row test over candidate rows (parallel arrays; ``groups``: the row's assignment, any
    integer key).  Invalid positions are dropped and counted, whether or not ``outside`` is set.
    ``latest``: of each group only the valid row with the largest (date, id) stays, and it matches only
    if it satisfies the containment itself.  A valid row matches when ``inside != outside``.  Returns
    (indices of the matches in (date desc, id desc) order, invalid rows)."""
    groups, dates, ids = np.asarray(groups, np.int64), np.asarray(dates, np.int64), np.asarray(ids, np.int64)
    idx, n_invalid = looked_at(groups, dates, ids, lats, lons, latest)
    inside = contains_np(polygon, np.asarray(lats, np.float64)[idx], np.asarray(lons, np.float64)[idx])
    idx = idx[inside != bool(outside)]
    return idx[np.lexsort((-ids[idx], -dates[idx]))], n_invalid


def host_zone(locations, polygon, start=None, end=None, outside=False, latest=False, page_number=1,
              page_size=100) -> dict:
    """The host route: listed location events (``latitude``, ``longitude``, ``event_date``,
    ``device_assignment_id``) filtered by the same function as the hot route, in the same result shape
    (``hotSince`` None).  No vertex limit here.  Ties at an equal date go by listing order, newest
    listed first."""
    poly = check_zone_args(polygon, start, end, max_vtx=None)
    evs = [e for e in locations if e.event_date is not None and (start is None or e.event_date >= start) and
           (end is None or e.event_date <= end)]
    group = {}
    groups = [group.setdefault(e.device_assignment_id, len(group)) for e in evs]
    nan = float("nan")
    sel, _ = zone_select(groups, [e.event_date for e in evs], np.arange(len(evs), 0, -1),
                         [nan if e.latitude is None else e.latitude for e in evs],
                         [nan if e.longitude is None else e.longitude for e in evs], poly, outside, latest)
    from .engine_base import EngineBase
    lo, hi = EngineBase._window(page_number, page_size, len(sel))
    return {"hotSince": None, "numResults": int(len(sel)), "results": [evs[i] for i in sel[lo:hi]]}
