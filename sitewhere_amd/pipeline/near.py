"""Locations near a point: the host side of ``EngineBase.near_store``.

``IDeviceEventSearchProvider.getLocationsNear(latitude, longitude, distance, dateRange)`` of the
reference's search SPI.  ``haversine_np`` is ``core/geo.haversine_m`` for arrays (the MI355X kernel
``k_near_filter`` spells the same formula in HIP); ``near_select`` is the row test, the ``latest``
rule and the ordering every route shares: the CPU engines' ``near_store`` (the oracle of the
kernels) and ``host_near`` (events listed through event management) both go through it.
"""
from __future__ import annotations

import math

import numpy as np

EARTH_R_M = 6371000.0
NEAR_MAX_RADIUS_M = 10_000_000.0     # keeps asin(sqrt(a)) away from a = 1 (the antipode), where it is ill conditioned
NEAR_BAND_M = 1e-6                   # the contract's band around the radius and around a returned distance
ORDERS = ("date", "distance")


def check_near_args(lat, lon, radius_m, start=None, end=None, order="date") -> tuple[float, float, float]:
    """``near_store``'s argument checks: (lat, lon, radius_m) as floats, or ``ValueError``."""
    lat, lon, radius_m = float(lat), float(lon), float(radius_m)
    if not (math.isfinite(lat) and abs(lat) <= 90.0):
        raise ValueError("latitude must lie in [-90, 90]")
    if not (math.isfinite(lon) and abs(lon) <= 180.0):
        raise ValueError("longitude must lie in [-180, 180]")
    if not (math.isfinite(radius_m) and radius_m >= 0.0):
        raise ValueError("distance must be finite and not negative")
    if radius_m > NEAR_MAX_RADIUS_M:
        raise ValueError(f"distance exceeds {NEAR_MAX_RADIUS_M:.0f} m")
    if start is not None and end is not None and int(start) > int(end):
        raise ValueError("end is before start")
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}")
    return lat, lon, radius_m


def haversine_np(lat1: float, lon1: float, lat2, lon2) -> np.ndarray:
    """``core/geo.haversine_m`` from one point to arrays of points: the same operations in the same
    order, fp64.  NaN where rounding lifts ``a`` above 1 (only at the antipode, far past any radius)."""
    lat2, lon2 = np.asarray(lat2, np.float64), np.asarray(lon2, np.float64)
    with np.errstate(invalid="ignore"):
        p1, p2 = math.radians(lat1), np.radians(lat2)
        dp, dl = p2 - p1, np.radians(lon2 - lon1)
        s1, s2 = np.sin(dp / 2), np.sin(dl / 2)
        a = s1 * s1 + math.cos(p1) * np.cos(p2) * (s2 * s2)
        return (2 * EARTH_R_M) * np.arcsin(np.sqrt(a))


def valid_position(lat, lon) -> np.ndarray:
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(lat) & np.isfinite(lon) & (np.abs(lat) <= 90.0) & (np.abs(lon) <= 180.0)


def near_box(lat: float, lon: float, radius_m: float) -> tuple[float, float, float, float]:
    """A conservative box around the cap of ``radius_m`` about (lat, lon), in degrees: (lat_lo, lat_hi,
    lon_lo, lon_hi).  ``lon_lo > lon_hi`` means the interval wraps across +-180 (inside: ``lon >= lon_lo
    or lon <= lon_hi``).  A cap that touches a pole takes the whole circle of longitudes.  The box
    excludes only points farther than ``radius_m + NEAR_BAND_M``: the angular radius is widened by
    1e-9 relative plus 1e-9 rad (6 mm on the ground) and each edge by another 1e-9 degree, orders of
    magnitude more than the rounding of the few operations here and of the haversine itself."""
    delta = (radius_m + NEAR_BAND_M) / EARTH_R_M * (1.0 + 1e-9) + 1e-9
    pad = 1e-9
    ddeg = math.degrees(delta) + pad
    lat_lo, lat_hi = lat - ddeg, lat + ddeg
    if lat_lo <= -90.0 or lat_hi >= 90.0:
        return max(lat_lo, -90.0), min(lat_hi, 90.0), -180.0, 180.0
    # delta < pi / 2 here (else a pole is inside), and cos(lat) > sin(delta): the asin is defined
    s = math.sin(delta) / math.cos(math.radians(lat))
    if s >= 1.0:
        return lat_lo, lat_hi, -180.0, 180.0
    dlon = math.degrees(math.asin(s)) * (1.0 + 1e-9) + pad
    if dlon >= 180.0:
        return lat_lo, lat_hi, -180.0, 180.0
    lon_lo, lon_hi = lon - dlon, lon + dlon
    if lon_lo < -180.0:
        lon_lo += 360.0
    if lon_hi > 180.0:
        lon_hi -= 360.0
    return lat_lo, lat_hi, lon_lo, lon_hi


def in_box(box, lat, lon) -> np.ndarray:
    lat_lo, lat_hi, lon_lo, lon_hi = box
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    in_lon = (lon >= lon_lo) | (lon <= lon_hi) if lon_lo > lon_hi else (lon >= lon_lo) & (lon <= lon_hi)
    return (lat >= lat_lo) & (lat <= lat_hi) & in_lon


def looked_at(groups, dates, ids, lats, lons, latest: bool):
    """The rows a location query looks at, of candidate rows as int64 arrays (``groups``: the row's
    assignment): those with a valid position, and with ``latest`` of each group only the one with the
    largest (date, id).  Returns (their indices, invalid rows).  The near, zone and grid queries share it."""
    ok = valid_position(lats, lons)
    idx = np.flatnonzero(ok)
    n_invalid = int(len(ok) - len(idx))
    if latest and len(idx):
        o = np.lexsort((ids[idx], dates[idx], groups[idx]))
        g = groups[idx][o]
        idx = idx[o[np.r_[g[1:] != g[:-1], True]]]
    return idx, n_invalid


def near_select(groups, dates, ids, lats, lons, lat: float, lon: float, radius_m: float, latest: bool, order: str):
    """The row test over candidate rows (parallel arrays; ``groups``: the row's assignment, any
    integer key).  Invalid positions are dropped and counted.  ``latest``: of each group only the valid
    row with the largest (date, id) stays, and it matches only if it lies inside the radius itself.
    Returns (indices of the matches in result order, their distances, invalid rows)."""
    groups, dates, ids = np.asarray(groups, np.int64), np.asarray(dates, np.int64), np.asarray(ids, np.int64)
    idx, n_invalid = looked_at(groups, dates, ids, lats, lons, latest)
    dist = haversine_np(lat, lon, np.asarray(lats, np.float64)[idx], np.asarray(lons, np.float64)[idx])
    with np.errstate(invalid="ignore"):
        m = dist <= radius_m
    idx, dist = idx[m], dist[m]
    keys = (-ids[idx], -dates[idx]) + ((dist,) if order == "distance" else ())
    o = np.lexsort(keys)
    return idx[o], dist[o], n_invalid


def host_near(locations, lat, lon, radius_m, start=None, end=None, latest=False, order="date", page_number=1,
              page_size=100) -> dict:
    """The host route: listed location events (``latitude``, ``longitude``, ``event_date``,
    ``device_assignment_id``) filtered by the same function as the hot route, in the same result shape
    (``hotSince`` None).  Ties at an equal date go by listing order, newest listed first."""
    lat, lon, radius_m = check_near_args(lat, lon, radius_m, start, end, order)
    evs = [e for e in locations if e.event_date is not None and (start is None or e.event_date >= start) and
           (end is None or e.event_date <= end)]
    group = {}
    groups = [group.setdefault(e.device_assignment_id, len(group)) for e in evs]
    nan = float("nan")
    sel, dist, _ = near_select(groups, [e.event_date for e in evs], np.arange(len(evs), 0, -1),
                               [nan if e.latitude is None else e.latitude for e in evs],
                               [nan if e.longitude is None else e.longitude for e in evs], lat, lon, radius_m, latest,
                               order)
    from .engine_base import EngineBase
    lo, hi = EngineBase._window(page_number, page_size, len(sel))
    return {"hotSince": None, "numResults": int(len(sel)), "results": [evs[i] for i in sel[lo:hi]],
            "distances": [float(d) for d in dist[lo:hi]]}
