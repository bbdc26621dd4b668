"""Ranking of groups over the event ring: the host side of ``EngineBase.rank_store``.

The ring's rows of one event type are grouped by the context they were persisted with (assignment,
customer, area or asset), each group folded into count, min, max and last of ``v0``, and the groups
ordered by one of those.  ``rank_select`` is the classification, the fold and the ordering every route
shares: the CPU engines' ``rank_store`` (the oracle of the MI355X kernels ``k_rank_*``) and ``host_rank``
(events listed through event management) both go through it.

Values are ordered by ``rank_key``, an int64 whose signed order is the IEEE total order of non-NaN
doubles (-0.0 below +0.0), so min and max are integer operations that return the bits some row holds and
every engine answers with the same bytes.
"""
from __future__ import annotations

import numpy as np

from ..models.columnar import EV_ALERT, EV_LOCATION, EV_MEASUREMENT, EV_STATE_CHANGE, RANK_CELL, RANK_MAX_KEYS  # noqa: F401

RANK_GROUPS = ("assignment", "customer", "area", "asset")
RANK_STATS = ("count", "min", "max", "last")
RANK_TYPES = (EV_MEASUREMENT, EV_LOCATION, EV_ALERT, EV_STATE_CHANGE)
_I64 = np.iinfo(np.int64)


def check_rank_args(event_type, group, stat="count", k=10, start=None, end=None, name_hash=None, min_level=None):
    """``rank_store``'s argument checks: (event type, k or None, name hash or None, min level or None) as
    integers, or ``ValueError``."""
    if isinstance(event_type, bool) or not isinstance(event_type, (int, np.integer)) or int(event_type) not in RANK_TYPES:
        raise ValueError("eventType must be a measurement, location, alert or state change")
    event_type = int(event_type)
    if group not in RANK_GROUPS:
        raise ValueError(f"groupBy must be one of {', '.join(RANK_GROUPS)}")
    if stat not in RANK_STATS:
        raise ValueError(f"stat must be one of {', '.join(RANK_STATS)}")
    try:
        kk = None if k is None else int(k)
        name = None if name_hash is None else int(name_hash)
        level = None if min_level is None else int(min_level)
        same = (k is None or (kk == k and not isinstance(k, bool))) and (min_level is None or level == min_level)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("top, the name hash and minLevel must be integers") from None
    if not same:
        raise ValueError("top and minLevel must be integers")
    if kk is not None and kk < 1:
        raise ValueError("top must be at least 1")
    if name is not None and not 0 <= name < 1 << 64:
        raise ValueError("the name hash must be an unsigned 64-bit integer")
    if stat != "count" and (event_type != EV_MEASUREMENT or name is None):
        raise ValueError(f"stat {stat} needs measurements of one name")
    if level is not None and (event_type != EV_ALERT or not 0 <= level <= 3):
        raise ValueError("minLevel is for alerts and lies in 0..3")
    if start is not None and end is not None and int(start) > int(end):
        raise ValueError("end is before start")
    return event_type, kk, name, level


def rank_key(v):
    """``b ^ ((b >> 63) & INT64_MAX)`` of a double's bits ``b`` (arithmetic shift): an int64 whose signed
    order is the IEEE total order of the doubles.  Its own inverse: ``rank_key(keys.view(float64))`` of
    keys as int64 gives the doubles' bits back."""
    b = np.ascontiguousarray(v, np.float64).view(np.int64)
    return b ^ ((b >> 63) & _I64.max)


def rank_select(keys, dates, ids, values, n_keys: int, stat: str = "count", k=None, ascending: bool = False):
    """Classify, fold and order candidate rows (parallel arrays; ``keys``: the row's group key, ``ids``:
    its event id, ``values``: its ``v0``, or None for a type that has none).  A NaN value counts in
    ``nan``; then a key outside [0, n_keys) in ``ungrouped``; the rest fold into their groups.  Returns
    (``RANK_CELL`` cells of the first ``k`` groups (None: all) by ``stat`` descending (``ascending``: the
    other way), ties by key ascending, rows folded, nan, ungrouped, non-empty groups)."""
    keys, dates, ids = np.asarray(keys, np.int64), np.asarray(dates, np.int64), np.asarray(ids, np.int64)
    ok = np.ones(len(keys), bool)
    if values is not None:
        values = np.asarray(values, np.float64)
        ok = ~np.isnan(values)
    n_nan = int(len(ok) - ok.sum())
    inside = ok & (keys >= 0) & (keys < n_keys)
    n_ungrouped = int(ok.sum() - inside.sum())
    idx = np.flatnonzero(inside)
    o = idx[np.lexsort((ids[idx], dates[idx], keys[idx]))]       # by group, then (date, id): a group's last row is its last
    g = keys[o]
    first = np.flatnonzero(np.r_[True, g[1:] != g[:-1]]) if len(o) else np.zeros(0, np.int64)
    last = np.r_[first[1:], len(o)] - 1 if len(o) else first
    cells = np.zeros(len(first), RANK_CELL)
    cells["key"] = g[first]
    cells["count"] = last - first + 1
    cells["last_date"] = dates[o][last]
    cells["last_id"] = ids[o][last]
    if values is not None and len(o):
        rk = rank_key(values[o])
        cells["min"] = rank_key(np.minimum.reduceat(rk, first).view(np.float64)).view(np.float64)
        cells["max"] = rank_key(np.maximum.reduceat(rk, first).view(np.float64)).view(np.float64)
        cells["last"] = values[o][last]
    sk = cells["count"] if stat == "count" else rank_key(cells[stat])
    order = np.lexsort((cells["key"], sk if ascending else ~sk))    # ~ reverses the order and cannot overflow
    return cells[order[:k]], len(o), n_nan, n_ungrouped, len(first)


def rank_response(cells, info, ids=None, hot_since=None) -> dict:
    """The one response shape of both routes.  ``ids``: the entity id of each cell's key; a cell whose id
    is None is left out."""
    out = []
    for i, c in enumerate(cells):
        eid = int(c["key"]) if ids is None else ids[i]
        if eid is None:
            continue
        out.append({"id": eid, "count": int(c["count"]), "min": float(c["min"]), "max": float(c["max"]),
                    "last": float(c["last"]), "lastDate": int(c["last_date"])})
    return {"hotSince": hot_since, "numResults": int(info["rows"]), "nan": int(info["nan"]),
            "ungrouped": int(info["ungrouped"]), "groups": int(info["groups"]), "results": out}


_ENTITY = {"assignment": "device_assignment_id", "customer": "customer_id", "area": "area_id", "asset": "asset_id"}


def host_rank(events, event_type, group, stat="count", k=10, start=None, end=None, name=None, min_level=None,
              ascending=False) -> dict:
    """The host route: listed events of ``event_type`` (``event_date``, the entity ids, and ``name`` /
    ``value`` of a measurement, ``type`` / ``level`` of an alert) ranked by the same function as the hot
    route, in the same response shape (``hotSince`` None).  ``name``: the measurement name or alert type
    to keep.  Groups are the entity ids themselves; an event without one is ungrouped.  Ties between rows
    at an equal date go by listing order, newest listed first; ties between groups by the order in which
    the groups first appear in the listing."""
    event_type, k, _, min_level = check_rank_args(event_type, group, stat, k, start, end,
                                                  None if name is None else 0, min_level)
    field = _ENTITY[group]
    evs = [e for e in events if e.event_date is not None and (start is None or e.event_date >= start) and
           (end is None or e.event_date <= end)]
    if name is not None:
        evs = [e for e in evs if (e.name if event_type == EV_MEASUREMENT else getattr(e, "type", None)) == name]
    if min_level is not None:
        evs = [e for e in evs if _level(e) >= min_level]
    seen = {}
    keys = [-1 if getattr(e, field, None) is None else seen.setdefault(getattr(e, field), len(seen)) for e in evs]
    values = None
    if event_type == EV_MEASUREMENT:
        values = [float("nan") if e.value is None else float(e.value) for e in evs]
    cells, rows, n_nan, n_ungrouped, groups = rank_select(keys, [e.event_date for e in evs], np.arange(len(evs), 0, -1),
                                                          values, len(seen), stat, k, ascending)
    ids = list(seen)
    info = {"rows": rows, "nan": n_nan, "ungrouped": n_ungrouped, "groups": groups}
    return rank_response(cells, info, [ids[int(c["key"])] for c in cells])


def _level(e) -> int:
    from ..models.domain import ALERT_LEVEL_INDEX
    return ALERT_LEVEL_INDEX.get(getattr(e, "level", None), 0)
