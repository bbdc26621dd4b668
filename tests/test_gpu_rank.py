"""Rankings of groups on the MI355X (``sw_store_rank``, csrc/hip/swgpu.hip) against the CPU oracle engine,
under the contract of ``EngineBase.rank_store``: the cells and the info byte for byte -- every operation is
on integers or copies bits, so there is no band -- in both forms of the fold (per-workgroup LDS tables, and
the global table with run combining), and the same bytes on every call."""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X GPU")]

if gpu_available():
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

from sitewhere_amd.models.columnar import EV_ALERT, EV_LOCATION, EV_MEASUREMENT, RANK_CELL, RANK_QUERY
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine

from near_scenarios import CENTRE, RINGS
from pipeline_scenarios import NOW, canon_out, fleet_batch, setup_fleet, small_cfg
from rank_scenarios import (GROUPS, HAND_ALERT_ASG, HAND_ROWS, RING_FACTS, TEMP, assert_conserved, assert_same_rank,
                            hand_eids, hand_expected, hand_rank_batch, hand_rank_fleet, ring_queries)
from series_scenarios import ALL, NAMES, fill_ring
from state_scenarios import HOT_DEV, hot_key_batch
from zone_scenarios import POLYGONS


def lds_keys(n=-1):
    """SW_RANK_LDS_KEYS as the library was compiled (n < 0), or the limit lowered to n."""
    from sitewhere_amd._native import gpu
    return int(gpu().sw_rank_lds_keys(n))


class fold_form:
    """Run the block with the LDS limit at ``keys`` (0: the global form for every key space); the compiled
    limit is put back on the way out."""

    def __init__(self, keys):
        self.keys = keys

    def __enter__(self):
        self.compiled = lds_keys()
        assert lds_keys(self.keys) == min(self.keys, self.compiled)

    def __exit__(self, *exc):
        from sitewhere_amd._native import gpu
        gpu().sw_rank_lds_keys(1 << 40)              # clamped to the compiled limit
        assert lds_keys() == self.compiled


def ring_pair(store_cap):
    g = fill_ring(GpuInboundEngine(small_cfg(store_cap=store_cap)))
    c = fill_ring(CpuInboundEngine(small_cfg(store_cap=store_cap)))
    assert g.cursor == c.cursor == 12476
    return g, c


@pytest.fixture(scope="module")
def rings():
    return {cap: ring_pair(cap) for cap in RINGS}


_want = {}


def check(g, c, **q):
    """One query on both engines under the contract; the oracle's answer is computed once per query and ring."""
    key = (id(c), c.cursor, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in q.items())))
    if key not in _want:
        _want[key] = c.rank_store(**q)
    want = _want[key]
    got = g.rank_store(**q)
    assert_same_rank(got, want)
    assert_conserved(*got, q.get("k", 10))
    return want


# 12476 ring rows at 1024 a workgroup: 13 workgroups (4 on the wrapped ring) merge their tables.  The
# context dimensions (7, 5 and 3 keys) fold in LDS at the compiled limit and in the global table at limit 0;
# the 4096 assignment keys are past the limit and always fold in the global table, where a step's rows
# lie in runs of one assignment.
@pytest.mark.parametrize("limit", ["compiled", 0])
@pytest.mark.parametrize("cap", sorted(RINGS))
def test_ring_cases_in_both_forms(rings, cap, limit):
    g, c = rings[cap]
    assert (g.cursor > cap) == (cap == 1 << 12)
    with fold_form(lds_keys() if limit == "compiled" else 0):
        for q in ring_queries():
            cells, info = check(g, c, **q)
            assert (info["hot_since"] is None) == (cap != 1 << 12)
            if q == dict(event_type=EV_MEASUREMENT, group="assignment", stat="count", name_hash=NAMES[0], k=None):
                assert (info["rows"], info["groups"]) == RING_FACTS[cap][:2]


def edge_pair(n_asg):
    """A fleet whose assignments fill the key space: the last key of the table, n_asg - 1, is assigned."""
    out = []
    for cls in (GpuInboundEngine, CpuInboundEngine):
        e = cls(small_cfg(max_assignments=n_asg, store_cap=1 << 12))
        setup_fleet(e, n_dev=n_asg, unassigned_every=7)
        for k in range(2):
            e.step(*fleet_batch(1500, seed=40 + k, n_dev=n_asg), NOW + k, presence=False)
        out.append(e)
    assert out[0].cursor == out[1].cursor > 1 << 12              # wrapped
    return out


def test_limit_at_the_assignment_key_space_and_one_below_and_the_table_edge():
    n_asg = 300                                      # more than a workgroup's 256 threads: the merge must go round
    assert (n_asg - 1) % 7 != 6 and n_asg < lds_keys()
    g, c = edge_pair(n_asg)
    assert g.rank_key_space("assignment") == ("asg", n_asg)
    qs = [q for q in ring_queries() if q["group"] == "assignment" and "asg_idx" not in q]
    for limit in (n_asg, n_asg - 1, lds_keys(), 0):              # LDS exactly at the key space; global just below
        with fold_form(limit):
            for q in qs:
                cells, info = check(g, c, **q)
            cells, info = check(g, c, event_type=EV_MEASUREMENT, group="assignment", k=None)
            assert cells["key"].max() == n_asg - 1 and (cells["key"] >= 256).sum() > 20       # the last key has rows
            assert info["groups"] > 200


def test_hand_batch_partial_wave_nan_signed_zeros_ties_last_by_id_no_customer_and_levels():
    g, c = hand_rank_fleet(GpuInboundEngine(small_cfg())), hand_rank_fleet(CpuInboundEngine(small_cfg()))
    rg, rc = g.step(*hand_rank_batch(), NOW, presence=False), c.step(*hand_rank_batch(), NOW, presence=False)
    assert rg.n_persisted == rc.n_persisted == g.cursor == c.cursor == HAND_ROWS < 64      # less than one wave of rows
    cols, eids = c.store_rows()
    for limit in (lds_keys(), 0):
        with fold_form(limit):
            for q, want, info in hand_expected(hand_eids(cols, eids)):
                got = g.rank_store(**q)
                assert_same_rank(got, (want, dict(info, hot_since=None)))
                assert_conserved(*got, q["k"])
                check(g, c, **q)
            for lv in range(4):
                cells, info = check(g, c, event_type=EV_ALERT, group="assignment", k=None, min_level=lv)
                assert cells["key"].tolist() == sorted(a for l, a in HAND_ALERT_ASG.items() if l >= lv)
            check(g, c, event_type=EV_MEASUREMENT, group="asset", stat="last", name_hash=TEMP, asg_idx=[2, 4, 5, 7])
            check(g, c, event_type=EV_MEASUREMENT, group="customer", stat="min", name_hash=TEMP, start=NOW - 85, end=NOW - 45)


def test_hot_key_in_both_forms():
    g, c = GpuInboundEngine(small_cfg()), CpuInboundEngine(small_cfg())
    for e in (g, c):
        setup_fleet(e, n_dev=100)
        (raw, offs, now, presence), = hot_key_batch()
        e.step(raw, offs, now, presence=presence)
    # 63 full waves and a partial one of one key, and the zone alerts its 819 locations raise
    assert g.cursor == c.cursor == 4095 + 819 and g.cursor % 64
    for limit in (lds_keys(), 0):
        with fold_form(limit):
            for group in ("assignment", "customer"):
                for stat in ("count", "min", "max", "last"):
                    cells, info = check(g, c, event_type=EV_MEASUREMENT, group=group, stat=stat, k=None,
                                        name_hash=TEMP)
                    assert info["groups"] == 1 and cells["count"][0] == info["rows"] == 3276
                    assert cells["key"][0] == (HOT_DEV if group == "assignment" else HOT_DEV % 7)
                    # the last event on the newest date is not the last event
                    assert (cells["min"][0], cells["max"][0], cells["last"][0], cells["last_date"][0]) == (0.0, 4093.0, 4092.0, NOW)
                cells, info = check(g, c, event_type=EV_LOCATION, group=group, k=None)
                assert cells["count"].tolist() == [819]


def test_empty_ring_and_refused_arguments_launch_nothing():
    g = GpuInboundEngine(small_cfg())
    cells, info = g.rank_store(EV_MEASUREMENT, "assignment", "max", name_hash=NAMES[0])    # cursor == 0: no buffer, no kernel
    assert cells.dtype == RANK_CELL and len(cells) == 0 and "rank" not in g._ring_bufs
    assert info == {"candidates": 0, "rows": 0, "nan": 0, "ungrouped": 0, "groups": 0, "hot_since": None}
    fill_ring(g)
    for bad in (dict(event_type=3), dict(group="device"), dict(stat="sum"), dict(stat="max"), dict(k=0),
                dict(min_level=1), dict(event_type=EV_ALERT, min_level=4), dict(start=NOW, end=NOW - 1),
                dict(event_type=EV_LOCATION, stat="last", name_hash=NAMES[0])):
        with pytest.raises(ValueError):
            g.rank_store(**dict(dict(event_type=EV_MEASUREMENT, group="assignment"), **bad))
    assert "rank" not in g._ring_bufs                # nothing was allocated, so nothing was launched
    # a name nothing carries: counted on the device, no group
    cells, info = g.rank_store(EV_MEASUREMENT, "area", "max", name_hash=12345)
    assert len(cells) == 0 and info["candidates"] == info["groups"] == 0 and "rank" in g._ring_bufs
    assert set(g._ring_bufs["rank"]) == {"counters", "tab", "cells", "sort"}


def test_abi_size_of_the_query():
    from sitewhere_amd._native import gpu
    from sitewhere_amd.ops.engine_abi import abi_sizes
    assert abi_sizes(gpu())["rank_query"] == 8 * len(RANK_QUERY) == 160
    assert 256 < lds_keys() < 4096                   # both forms exist, and the LDS one merges past a workgroup's size
    assert lds_keys() * 28 <= 64 * 1024              # a table fits the LDS a workgroup gets without opting in


def as_bytes(r):
    return r[0].tobytes(), r[1]


def test_same_bytes_every_call(rings):
    qs = ring_queries()
    for g, _ in rings.values():
        for limit in (lds_keys(), 0):
            with fold_form(limit):
                for q in qs[2::23]:
                    a = as_bytes(g.rank_store(**q))
                    assert as_bytes(g.rank_store(**q)) == a
                    assert g.query_store(EV_LOCATION, ALL, NOW - 60000, NOW, page_size=10)[0] > 0
                    assert g.aggregate_store(ALL, NAMES, NOW - 60000, NOW, 1000)[1]["rows"] > 0
                    assert g.near_store(*CENTRE, 25000.0, latest=True)[0] > 0
                    assert g.zone_store(POLYGONS["star"], latest=True)[0] > 0
                    assert g.grid_store(31.5, 35.5, -86.5, -82.5, 8, 8)[0]["count"].sum() > 0
                    assert as_bytes(g.rank_store(**q)) == a


def test_steps_and_the_other_queries_still_match_the_oracle_after_a_query():
    from grid_scenarios import BOXES, assert_same_grid
    from grid_scenarios import case_queries as grid_queries
    from near_scenarios import assert_clear_of_band, assert_same_answer
    from near_scenarios import case_queries as near_queries
    from series_scenarios import CASES, EXACT
    from zone_scenarios import assert_same_zone_answer
    from zone_scenarios import case_queries as zone_queries
    g, c = ring_pair(1 << 12)
    q = dict(event_type=EV_MEASUREMENT, group="customer", stat="max", name_hash=NAMES[0], k=None)
    before = as_bytes(check(g, c, **q))
    raw, offs = fleet_batch(1500, seed=99, n_dev=200)
    rg, rc = g.step(raw, offs, NOW + 9, presence=False), c.step(raw, offs, NOW + 9, presence=False)
    assert rg.n_events == rc.n_events and rg.n_persisted == rc.n_persisted
    assert canon_out(rg.out, c.names) == canon_out(rc.out, c.names)
    assert g.stats_dict() == c.stats_dict()
    assert as_bytes(check(g, c, **q)) != before                  # the ring moved on, and both engines with it
    for group in GROUPS:
        check(g, c, **dict(q, group=group, stat="last", k=10))
    t, cols, eids = g.query_store(EV_LOCATION, ALL, NOW - 60000, NOW, page_size=50)
    tc, ccols, ceids = c.query_store(EV_LOCATION, ALL, NOW - 60000, NOW, page_size=50)
    assert t == tc and np.array_equal(eids, ceids) and all(np.array_equal(cols[k], ccols[k]) for k in ("asg", "date", "v0"))
    asg, names, start, end, bucket = CASES[2][:5]
    got, want = g.aggregate_store(asg, names, start, end, bucket), c.aggregate_store(asg, names, start, end, bucket)
    assert got[1] == want[1]
    assert want[1]["rows"] > 0 and all(np.array_equal(got[0][f], want[0][f]) for f in EXACT)   # all but the sum
    for gq in grid_queries(BOXES["cut"], 3, 5):
        assert_same_grid(g.grid_store(**gq), c.grid_store(**gq))
    for zq in zone_queries(POLYGONS["ell"]):
        assert_same_zone_answer(g.zone_store(**zq), c.zone_store(**zq))
    assert_clear_of_band(c.store_rows()[0], *CENTRE, 25000.0)
    for nq in near_queries(25000.0):
        assert_same_answer(g.near_store(**nq), c.near_store(**nq), nq["order"])
