"""Locations in a zone on the MI355X (``sw_store_zone``, csrc/hip/swgpu.hip) against the CPU oracle
engine, under the contract of ``EngineBase.zone_store``: total, info, event ids and every page column
byte for byte -- the predicate is correctly rounded fp64 on both sides, so there is no band -- and the
same bytes on every call."""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X GPU")]

if gpu_available():
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

from sitewhere_amd.models.columnar import EV_LOCATION, ZONE_QUERY
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine

from pipeline_scenarios import NOW, canon_out, fleet_batch, setup_fleet, small_cfg
from near_scenarios import CENTRE, RINGS, hand_near_batch
from series_scenarios import ALL, NAMES, fill_ring
from zone_scenarios import (EXPECTED, HAND_INFO, HAND_RECTS, POLYGONS, assert_same_zone_answer, case_queries,
                            expected_total, rect)


def ring_pair(store_cap):
    g = fill_ring(GpuInboundEngine(small_cfg(store_cap=store_cap)))
    c = fill_ring(CpuInboundEngine(small_cfg(store_cap=store_cap)))
    assert g.cursor == c.cursor == 12476
    return g, c


@pytest.fixture(scope="module")
def rings():
    return {cap: ring_pair(cap) for cap in RINGS}


def check(g, c, **q):
    """One query on both engines under the contract; returns the total."""
    want = c.zone_store(**q)
    assert_same_zone_answer(g.zone_store(**q), want)
    return want[0]


@pytest.mark.parametrize("name", sorted(POLYGONS))
@pytest.mark.parametrize("cap", sorted(RINGS))
def test_ring_cases(rings, cap, name):
    g, c = rings[cap]
    assert (g.cursor > cap) == (cap == 1 << 12)
    poly = POLYGONS[name]
    for q in case_queries(poly):
        total = check(g, c, **q)
        if "asg_idx" not in q and "start" not in q:
            assert total == expected_total(cap, name, q["outside"], q["latest"])
    check(g, c, polygon=poly, page_number=2, page_size=40)
    info = g.zone_store(poly)[3]
    assert info["candidates"] == RINGS[cap][0] and info["invalid"] == 0
    assert (info["hot_since"] is None) == (cap != 1 << 12)
    assert g.zone_store(poly, latest=True, page_size=1)[3] == info


def test_hand_batch_partial_wave_edges_vertices_antimeridian_pole_invalid_ties():
    g, c = GpuInboundEngine(small_cfg()), CpuInboundEngine(small_cfg())
    for e in (g, c):
        setup_fleet(e, n_dev=1000)
    rg, rc = g.step(*hand_near_batch(), NOW, presence=False), c.step(*hand_near_batch(), NOW, presence=False)
    assert rg.n_persisted == rc.n_persisted and g.cursor == c.cursor < 64          # less than one wave of rows
    for name, poly, inside, outside in HAND_RECTS:
        for out, counts in ((False, inside), (True, outside)):
            for latest in (False, True):
                total = check(g, c, polygon=poly, outside=out, latest=latest)
                if counts is not None:
                    assert total == counts[1 if latest else 0], (name, out, latest)
                assert g.zone_store(poly, outside=out, latest=latest)[3] == HAND_INFO
    small = HAND_RECTS[0][1]
    total, pc, _, _ = g.zone_store(small, latest=True)
    assert total == 1 and pc["asg"].tolist() == [1] and pc["v0"].tolist() == [33.5001]       # the tie by event id
    assert sorted(g.zone_store(small, outside=True, latest=True)[1]["asg"].tolist()) == [2, 3, 4, 5, 8, 10]
    check(g, c, polygon=small, asg_idx=[1, 2], outside=True)
    check(g, c, polygon=rect(33.4, 33.6, -84.6, -84.4), start=NOW - 60, end=NOW - 50)
    check(g, c, polygon=POLYGONS["circ"], outside=True, latest=True)


def test_empty_ring_and_refused_arguments_launch_nothing():
    g = GpuInboundEngine(small_cfg())
    tri = POLYGONS["tri"]
    total, cols, eids, info = g.zone_store(tri, latest=True)                 # cursor == 0: no buffer, no kernel
    assert total == 0 and info == {"candidates": 0, "invalid": 0, "hot_since": None} and "zone" not in g._ring_bufs
    assert len(eids) == 0 and eids.dtype == np.int64 and cols["v0"].dtype == np.float64
    assert cols["name"].dtype == np.uint64 and all(len(v) == 0 for v in cols.values())
    fill_ring(g)
    nan = float("nan")
    big = np.vstack([POLYGONS["circ"], POLYGONS["circ"][:1]])
    for bad in (tri[:2], big, np.vstack([tri, [[nan, 0.0]]]), np.vstack([tri, [[90.5, 0.0]]]),
                np.vstack([tri, [[0.0, 181.0]]])):
        with pytest.raises(ValueError):
            g.zone_store(bad)
    with pytest.raises(ValueError):
        g.zone_store(tri, start=NOW, end=NOW - 1)
    assert "zone" not in g._ring_bufs                # nothing was allocated, so nothing was launched
    # a zone nothing matches: counted on the device, an empty page
    total, cols, eids, info = g.zone_store(rect(-34.0, -33.0, 95.0, 96.0))
    assert total == 0 and len(eids) == 0 and info["candidates"] > 0 and "zone" in g._ring_bufs
    c = fill_ring(CpuInboundEngine(small_cfg()))
    check(g, c, polygon=rect(-34.0, -33.0, 95.0, 96.0), outside=True, page_size=0)


def test_match_buffer_grows_and_the_pass_repeats():
    g, c = ring_pair(1 << 14)
    g._zone_rows0 = 64                                 # fewer than the 180 latest rows: the best passes run twice
    check(g, c, polygon=POLYGONS["world"], latest=True, page_size=0)
    assert g._ring_bufs["zone"]["rows"].numel() == 180
    g._zone_rows0 = 256                                # fewer rows than the 707 and 1914 matches below
    check(g, c, polygon=POLYGONS["ell"], page_size=0)
    assert g._ring_bufs["zone"]["rows"].numel() == EXPECTED[1 << 14]["ell"][0] == 707
    check(g, c, polygon=POLYGONS["world"], latest=True, page_size=0)         # 180 rows: fits
    assert g._ring_bufs["zone"]["rows"].numel() == 707
    check(g, c, polygon=POLYGONS["ell"], outside=True, latest=True, page_size=0)
    check(g, c, polygon=POLYGONS["world"], page_size=0)
    assert g._ring_bufs["zone"]["rows"].numel() == 1914


def test_abi_size_of_the_query():
    from sitewhere_amd._native import gpu
    from sitewhere_amd.ops.engine_abi import abi_sizes
    assert abi_sizes(gpu())["zone_query"] == 8 * len(ZONE_QUERY) == 176


def as_bytes(r):
    total, cols, eids, info = r
    return (total, {k: v.tobytes() for k, v in cols.items()}, eids.tobytes(), info)


def test_same_bytes_every_call(rings):
    for g, _ in rings.values():
        for q in case_queries(POLYGONS["star"]) + [dict(polygon=POLYGONS["circ"], page_number=2, page_size=30)]:
            a = as_bytes(g.zone_store(**q))
            assert as_bytes(g.zone_store(**q)) == a
            assert g.query_store(EV_LOCATION, ALL, NOW - 60000, NOW, page_size=10)[0] > 0
            assert g.aggregate_store(ALL, NAMES, NOW - 60000, NOW, 1000)[1]["rows"] > 0
            assert g.near_store(*CENTRE, 25000.0, latest=True)[0] > 0
            assert as_bytes(g.zone_store(**q)) == a


def test_steps_and_the_near_query_still_work_after_a_query():
    from near_scenarios import assert_clear_of_band, assert_same_answer
    from near_scenarios import case_queries as near_queries
    g, c = ring_pair(1 << 12)
    check(g, c, polygon=POLYGONS["star"], latest=True)
    raw, offs = fleet_batch(1500, seed=99, n_dev=200)
    rg, rc = g.step(raw, offs, NOW + 9, presence=False), c.step(raw, offs, NOW + 9, presence=False)
    assert rg.n_events == rc.n_events and rg.n_persisted == rc.n_persisted
    assert canon_out(rg.out, c.names) == canon_out(rc.out, c.names)
    assert g.stats_dict() == c.stats_dict()
    for q in case_queries(POLYGONS["ell"]):
        check(g, c, **q)
    assert_clear_of_band(c.store_rows()[0], *CENTRE, 25000.0)
    for q in near_queries(25000.0):
        assert_same_answer(g.near_store(**q), c.near_store(**q), q["order"])
