"""Locations near a point on the MI355X (``sw_store_near``, csrc/hip/swgpu.hip) against the CPU oracle
engine, under the contract of ``EngineBase.near_store``: total, page rows, event ids and info exact,
distances within ``NEAR_BAND_M``; the same bytes on every call.  Each comparison prints the largest
|distance - oracle distance| it saw (``-s`` shows it; profiles/hot_near/README.md records it)."""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X GPU")]

if gpu_available():
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

from sitewhere_amd.models.columnar import EV_LOCATION, EV_MEASUREMENT, NEAR_QUERY, NEAR_QUERY_F64, NEAR_WORDS, RING_QUERY
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.near import NEAR_BAND_M

from pipeline_scenarios import NOW, canon_out, fleet_batch, setup_fleet, small_cfg
from near_scenarios import (CENTRE, HAND_QUERIES, RADII, RINGS, assert_clear_of_band, assert_same_answer, case_queries,
                            hand_near_batch)
from series_scenarios import ALL, NAMES, fill_ring


def ring_pair(store_cap):
    g = fill_ring(GpuInboundEngine(small_cfg(store_cap=store_cap)))
    c = fill_ring(CpuInboundEngine(small_cfg(store_cap=store_cap)))
    assert g.cursor == c.cursor == 12476
    return g, c, c.store_rows()[0]


@pytest.fixture(scope="module")
def rings():
    return {cap: ring_pair(cap) for cap in RINGS}


def check(g, c, **q):
    """One query on both engines under the contract; returns (total, largest distance deviation)."""
    got, want = g.near_store(**q), c.near_store(**q)
    err = assert_same_answer(got, want, q.get("order", "date"))
    return want[0], err


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("cap", sorted(RINGS))
def test_ring_cases(rings, cap, radius):
    g, c, cols = rings[cap]
    assert (g.cursor > cap) == (cap == 1 << 12)
    assert_clear_of_band(cols, *CENTRE, radius)
    n_match = RINGS[cap][2][RADII.index(radius)]
    worst = 0.0
    for q in case_queries(radius):
        total, err = check(g, c, **q)
        worst = max(worst, err)
        if not q["latest"] and "asg_idx" not in q and "start" not in q:
            assert total == n_match
    total, err = check(g, c, lat=CENTRE[0], lon=CENTRE[1], radius_m=radius, order="distance", page_number=2, page_size=40)
    info = g.near_store(*CENTRE, radius)[4]
    assert info["candidates"] == RINGS[cap][0] and info["invalid"] == 0
    assert (info["hot_since"] is None) == (cap != 1 << 12)
    print(f"near worst |dist - oracle| ring {cap} radius {radius:.0f}: {max(worst, err):.3e} m (band {NEAR_BAND_M:.0e})")


def test_hand_batch_partial_wave_antimeridian_pole_invalid_ties():
    g, c = GpuInboundEngine(small_cfg()), CpuInboundEngine(small_cfg())
    for e in (g, c):
        setup_fleet(e, n_dev=1000)
    rg, rc = g.step(*hand_near_batch(), NOW, presence=False), c.step(*hand_near_batch(), NOW, presence=False)
    assert rg.n_persisted == rc.n_persisted and g.cursor == c.cursor < 64          # less than one wave of rows
    cols = c.store_rows()[0]
    worst = 0.0
    for la, lo, radius, n_all, n_latest in HAND_QUERIES:
        assert_clear_of_band(cols, la, lo, radius)
        for latest, n in ((False, n_all), (True, n_latest)):
            for order in ("date", "distance"):
                total, err = check(g, c, lat=la, lon=lo, radius_m=radius, latest=latest, order=order)
                assert total == n
                worst = max(worst, err)
                assert g.near_store(la, lo, radius, latest=latest)[4] == {"candidates": 12, "invalid": 3, "hot_since": None}
    total, pc, _, dist, _ = g.near_store(33.5, -84.5, 100.0, latest=True)
    by_asg = dict(zip(pc["asg"].tolist(), pc["v0"].tolist()))
    assert by_asg == {1: 33.5001, 8: 33.5003}       # 1: the tie by event id; 2: newest row outside; 8: newest valid
    nearest = g.near_store(33.5, -84.5, 100.0, order="distance")
    assert nearest[1]["asg"].tolist() == [1, 1, 2, 8] and nearest[3][0] <= NEAR_BAND_M
    check(g, c, lat=33.5, lon=-84.5, radius_m=100.0, asg_idx=[2, 8])
    check(g, c, lat=33.5, lon=-84.5, radius_m=100.0, start=NOW - 60, end=NOW - 50)
    assert_clear_of_band(cols, 33.5, -84.5, 1.0e7)
    check(g, c, lat=33.5, lon=-84.5, radius_m=1.0e7, order="distance")           # the largest radius: the whole-circle box
    print(f"near worst |dist - oracle| hand batch: {worst:.3e} m (band {NEAR_BAND_M:.0e})")


def test_empty_ring_and_refused_arguments_launch_nothing():
    g = GpuInboundEngine(small_cfg())
    total, cols, eids, dist, info = g.near_store(*CENTRE, 1000.0, latest=True)     # cursor == 0: no buffer, no kernel
    assert total == 0 and info == {"candidates": 0, "invalid": 0, "hot_since": None} and "near" not in g._ring_bufs
    assert len(eids) == len(dist) == 0 and dist.dtype == np.float64 and cols["v0"].dtype == np.float64
    assert cols["name"].dtype == np.uint64 and all(len(v) == 0 for v in cols.values())
    fill_ring(g)
    nan = float("nan")
    for bad in ((90.5, 0.0, 1.0), (nan, 0.0, 1.0), (0.0, -180.5, 1.0), (0.0, 0.0, -1.0), (0.0, 0.0, nan),
                (0.0, 0.0, 1.0e7 + 1), (0.0, 0.0, float("inf"))):
        with pytest.raises(ValueError):
            g.near_store(*bad)
    with pytest.raises(ValueError):
        g.near_store(0.0, 0.0, 1.0, start=NOW, end=NOW - 1)
    with pytest.raises(ValueError):
        g.near_store(0.0, 0.0, 1.0, order="nearest")
    assert "near" not in g._ring_bufs                # nothing was allocated, so nothing was launched
    # a query nothing matches: counted on the device, an empty page
    total, cols, eids, dist, info = g.near_store(-33.5, 95.5, 1000.0)
    assert total == 0 and len(eids) == len(dist) == 0 and info["candidates"] > 0 and "near" in g._ring_bufs
    # a view the engine never builds, its oldest row one past the ring: the entry point itself refuses it
    # (hipErrorInvalidValue) before the counters of the query above are zeroed
    _, n, head, bits, _ = g._position_view("near", None, None, None, False)
    head[RING_QUERY.index("head")] = n
    q = np.concatenate([head, g._query_words(NEAR_WORDS, NEAR_QUERY_F64, dict(
        lat=0.0, lon=0.0, radius_m=1.0, lat_lo=-1.0, lat_hi=1.0, lon_lo=-1.0, lon_hi=1.0))])
    rows, dist, counters = (g._ring_bufs["near"][k] for k in ("rows", "dist", "counters"))
    before = counters[:3].cpu()
    assert g.lib.sw_store_near(q.ctypes.data, rows.data_ptr(), dist.data_ptr(), rows.numel(), counters.data_ptr(),
                               g._stream()) == 1
    assert counters[:3].cpu().tolist() == before.tolist() and before[1] > 0


def test_match_buffers_grow_and_the_pass_repeats():
    g, c, _ = ring_pair(1 << 14)
    g._near_rows0 = 64                                 # fewer than the 180 latest rows: the best passes run twice
    check(g, c, lat=CENTRE[0], lon=CENTRE[1], radius_m=250000.0, latest=True, page_size=0)
    assert g._ring_bufs["near"]["rows"].numel() == g._ring_bufs["near"]["dist"].numel() == 180
    g._near_rows0 = 256                                # fewer rows than the 925 and 1914 matches below
    check(g, c, lat=CENTRE[0], lon=CENTRE[1], radius_m=60000.0, order="distance", page_size=0)
    assert g._ring_bufs["near"]["rows"].numel() == g._ring_bufs["near"]["dist"].numel() == 925
    check(g, c, lat=CENTRE[0], lon=CENTRE[1], radius_m=250000.0, latest=True, page_size=0)      # 180 rows: fits
    assert g._ring_bufs["near"]["rows"].numel() == 925
    check(g, c, lat=CENTRE[0], lon=CENTRE[1], radius_m=250000.0, page_size=0)
    assert g._ring_bufs["near"]["rows"].numel() == 1914


def test_abi_size_of_the_query():
    from sitewhere_amd._native import gpu
    from sitewhere_amd.ops.engine_abi import abi_sizes
    assert abi_sizes(gpu())["near_query"] == 8 * len(NEAR_QUERY) == 176
    assert abi_sizes(gpu())["position_view"] == 120


def as_bytes(r):
    total, cols, eids, dist, info = r
    return (total, {k: v.tobytes() for k, v in cols.items()}, eids.tobytes(), dist.tobytes(), info)


def test_same_bytes_every_call(rings):
    for g, _, _ in rings.values():
        for q in case_queries(60000.0) + [dict(lat=CENTRE[0], lon=CENTRE[1], radius_m=25000.0, order="distance",
                                                page_number=2, page_size=30)]:
            a = as_bytes(g.near_store(**q))
            assert as_bytes(g.near_store(**q)) == a
            assert g.query_store(EV_LOCATION, ALL, NOW - 60000, NOW, page_size=10)[0] > 0
            assert g.aggregate_store(ALL, NAMES, NOW - 60000, NOW, 1000)[1]["rows"] > 0
            assert as_bytes(g.near_store(**q)) == a


def test_steps_still_work_after_a_query():
    g, c, _ = ring_pair(1 << 12)
    check(g, c, lat=CENTRE[0], lon=CENTRE[1], radius_m=60000.0, latest=True, order="distance")
    raw, offs = fleet_batch(1500, seed=99, n_dev=200)
    rg, rc = g.step(raw, offs, NOW + 9, presence=False), c.step(raw, offs, NOW + 9, presence=False)
    assert rg.n_events == rc.n_events and rg.n_persisted == rc.n_persisted
    assert canon_out(rg.out, c.names) == canon_out(rc.out, c.names)
    assert g.stats_dict() == c.stats_dict()
    assert g.aggregate_store(ALL, NAMES, NOW - 60000, NOW, 1000)[1] == c.aggregate_store(ALL, NAMES, NOW - 60000, NOW, 1000)[1]
    assert_clear_of_band(c.store_rows()[0], *CENTRE, 25000.0)
    for q in case_queries(25000.0):
        check(g, c, **q)
