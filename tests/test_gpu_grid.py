"""Location density grids on the MI355X (``sw_store_grid``, csrc/hip/swgpu.hip) against the CPU oracle
engine, under the contract of ``EngineBase.grid_store``: the cells and the info byte for byte -- counts
and dates are integers and the cell formula is correctly rounded fp64 on both sides, so there is no
band -- and the same bytes on every call."""
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X GPU")]

if gpu_available():
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

from sitewhere_amd.models.columnar import EV_LOCATION, GRID_QUERY
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine

from grid_scenarios import (AROUND, BOXES, HAND_INFO, assert_conserved, assert_same_grid, case_queries, hand_expected,
                            hand_grid_batch)
from near_scenarios import CENTRE, RINGS
from pipeline_scenarios import NOW, canon_out, fleet_batch, setup_fleet, small_cfg
from series_scenarios import ALL, NAMES, fill_ring
from zone_scenarios import POLYGONS


def lds_cells():
    """SW_GRID_LDS_CELLS as the library was compiled: the largest grid counted in LDS tables."""
    from sitewhere_amd._native import gpu
    return int(gpu().sw_grid_lds_cells(-1))


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
        _want[key] = c.grid_store(**q)
    want = _want[key]
    got = g.grid_store(**q)
    assert_same_grid(got, want)
    assert_conserved(*got, q.get("latest", False))
    return want


# 12476 ring rows at 1024 a workgroup: 13 workgroups (4 on the wrapped ring) merge into the one cell of 1 x 1,
# and into every cell of the others.  1 x limit and 1 x (limit + 1) are the two sides of the path switch,
# with the fleet in columns far past the first 256, where a flush that stopped at the workgroup's size would end.
def grids():
    n = lds_cells()
    return [("around", 1, 1), ("around", 8, 8), ("cut", 3, 5), ("around", 1, n), ("around", 1, n + 1), ("around", 256, 256)]


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("cap", sorted(RINGS))
def test_ring_cases(rings, cap, which):
    g, c = rings[cap]
    assert (g.cursor > cap) == (cap == 1 << 12)
    box, n_rows, n_cols = grids()[which]
    for b in (box, "crossing"):
        for q in case_queries(BOXES[b], n_rows, n_cols):
            cells, info = check(g, c, **q)
            if "asg_idx" not in q and "start" not in q:
                assert info["candidates"] == RINGS[cap][0] and info["invalid"] == 0
                assert (info["outside"] > 0) == (b != "around") and cells["count"].sum() > 0
                if n_rows == 1 and n_cols > 256:
                    assert cells["count"][0, 256:].sum() > 0          # cells past a workgroup's size are filled
                if q["latest"]:
                    assert cells["count"].sum() + info["outside"] == RINGS[cap][1]
            assert (info["hot_since"] is None) == (cap != 1 << 12)


def test_hand_batch_partial_wave_edges_boundaries_antimeridian_invalid_and_the_tie():
    g, c = GpuInboundEngine(small_cfg()), CpuInboundEngine(small_cfg())
    for e in (g, c):
        setup_fleet(e, n_dev=1000)
    rg, rc = g.step(*hand_grid_batch(), NOW, presence=False), c.step(*hand_grid_batch(), NOW, presence=False)
    assert rg.n_persisted == rc.n_persisted and g.cursor == c.cursor < 64          # less than one wave of rows
    for box, r, k, latest, want, outside in hand_expected():
        got = g.grid_store(*box, r, k, latest=latest)
        assert_same_grid(got, (want, dict(HAND_INFO, outside=outside, hot_since=None)))
        assert_conserved(*got, latest, 16)
        check(g, c, lat_lo=box[0], lat_hi=box[1], lon_lo=box[2], lon_hi=box[3], n_rows=r, n_cols=k, latest=latest)
    q = dict(lat_lo=33.0, lat_hi=34.0, lon_lo=-85.0, lon_hi=-84.0, n_rows=2, n_cols=2)
    check(g, c, asg_idx=[1, 2, 12], **q)
    check(g, c, start=NOW - 60, end=NOW - 41, latest=True, **q)
    # the same rows on the global path: a 300 x 200 grid of the hand box, the edges in its last row and column
    cells, info = check(g, c, **dict(q, n_rows=300, n_cols=200))
    assert cells["count"][299].sum() == 1 and cells["count"][:, 199].sum() == 1 and cells["count"].sum() == 9


def test_empty_ring_and_refused_arguments_launch_nothing():
    g = GpuInboundEngine(small_cfg())
    cells, info = g.grid_store(*AROUND, 8, 8, latest=True)                   # cursor == 0: no buffer, no kernel
    assert cells.shape == (8, 8) and not cells.tobytes().strip(b"\0") and "grid" not in g._ring_bufs
    assert info == {"candidates": 0, "invalid": 0, "outside": 0, "hot_since": None}
    fill_ring(g)
    nan = float("nan")
    for bad in ((34.0, 33.0, -85.0, -84.0, 8, 8), (33.0, 34.0, -85.0, -85.0, 8, 8), (-91.0, 34.0, -85.0, -84.0, 8, 8),
                (33.0, 34.0, -85.0, 181.0, 8, 8), (nan, 34.0, -85.0, -84.0, 8, 8), (33.0, 34.0, -85.0, -84.0, 0, 8),
                (33.0, 34.0, -85.0, -84.0, 256, 257)):
        with pytest.raises(ValueError):
            g.grid_store(*bad)
    with pytest.raises(ValueError):
        g.grid_store(*AROUND, 8, 8, start=NOW, end=NOW - 1)
    assert "grid" not in g._ring_bufs                # nothing was allocated, so nothing was launched
    # a box nothing lies in: counted on the device, every cell empty
    cells, info = g.grid_store(-34.0, -33.0, 95.0, 96.0, 4, 4)
    assert not cells.tobytes().strip(b"\0") and info["outside"] == info["candidates"] > 0 and "grid" in g._ring_bufs
    assert set(g._ring_bufs["grid"]) == {"counters", "cells"}                     # `best` comes with latest only


def test_abi_size_of_the_query():
    from sitewhere_amd._native import gpu
    from sitewhere_amd.ops.engine_abi import abi_sizes
    assert abi_sizes(gpu())["grid_query"] == 8 * len(GRID_QUERY) == 192
    assert 256 < lds_cells() < 65536                 # both paths exist, and the LDS one flushes past a workgroup's size


def as_bytes(r):
    return r[0].tobytes(), r[1]


def test_same_bytes_every_call(rings):
    n = lds_cells()
    for g, _ in rings.values():
        for q in case_queries(BOXES["cut"], 3, 5)[::5] + case_queries(AROUND, 1, n)[:1] + case_queries(AROUND, 1, n + 1)[3:4]:
            a = as_bytes(g.grid_store(**q))
            assert as_bytes(g.grid_store(**q)) == a
            assert g.query_store(EV_LOCATION, ALL, NOW - 60000, NOW, page_size=10)[0] > 0
            assert g.aggregate_store(ALL, NAMES, NOW - 60000, NOW, 1000)[1]["rows"] > 0
            assert g.near_store(*CENTRE, 25000.0, latest=True)[0] > 0
            assert g.zone_store(POLYGONS["star"], latest=True)[0] > 0
            assert as_bytes(g.grid_store(**q)) == a


def test_steps_and_the_zone_and_near_queries_still_work_after_a_query():
    from near_scenarios import assert_clear_of_band, assert_same_answer
    from near_scenarios import case_queries as near_queries
    from zone_scenarios import assert_same_zone_answer
    from zone_scenarios import case_queries as zone_queries
    g, c = ring_pair(1 << 12)
    check(g, c, **case_queries(AROUND, 8, 8)[3])
    raw, offs = fleet_batch(1500, seed=99, n_dev=200)
    rg, rc = g.step(raw, offs, NOW + 9, presence=False), c.step(raw, offs, NOW + 9, presence=False)
    assert rg.n_events == rc.n_events and rg.n_persisted == rc.n_persisted
    assert canon_out(rg.out, c.names) == canon_out(rc.out, c.names)
    assert g.stats_dict() == c.stats_dict()
    for q in case_queries(BOXES["cut"], 3, 5):
        check(g, c, **q)
    for q in zone_queries(POLYGONS["ell"]):
        assert_same_zone_answer(g.zone_store(**q), c.zone_store(**q))
    assert_clear_of_band(c.store_rows()[0], *CENTRE, 25000.0)
    for q in near_queries(25000.0):
        assert_same_answer(g.near_store(**q), c.near_store(**q), q["order"])
