"""Bucketed measurement series on the MI355X (``sw_store_series``, csrc/hip/swgpu.hip) against the CPU
oracle engine, under the contract of ``EngineBase.aggregate_store``: count, min, max, first, last, both
dates and both ids exact; ``|sum - fsum| <= n * 2^-52 * sum|x|`` per cell; the same bytes on every call."""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X GPU")]

if gpu_available():
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

from sitewhere_amd.models.columnar import EV_MEASUREMENT
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.fleet import hash64

from pipeline_scenarios import NOW, canon_out, fleet_batch, setup_fleet, small_cfg
from series_scenarios import ALL, CASES, NAMES, assert_cells, brute_force, fill_ring, hand_series_batch


def ring_pair(store_cap):
    g = fill_ring(GpuInboundEngine(small_cfg(store_cap=store_cap)))
    c = fill_ring(CpuInboundEngine(small_cfg(store_cap=store_cap)))
    assert g.cursor == c.cursor == 12476
    return g, c, c.store_rows()


@pytest.fixture(scope="module")
def wrapped():
    return ring_pair(1 << 12)


@pytest.fixture(scope="module")
def unwrapped():
    return ring_pair(1 << 14)


def check(g, c, rows, query, n_rows=None):
    """One query on both engines under the contract; the sum bound comes from the oracle's ring rows."""
    cols, eids = rows
    cg, ig = g.aggregate_store(*query)
    cc, ic = c.aggregate_store(*query)
    _, _, _, abs_sum = brute_force(cols, eids, *query)
    assert ig == ic and (n_rows is None or ig["rows"] == n_rows)
    assert_cells(cg, cc, abs_sum)
    return cg


@pytest.mark.parametrize("case", range(len(CASES)))
def test_wrapped_ring_cases(wrapped, case):
    g, c, rows = wrapped
    assert g.cursor > g.cfg.store_cap
    *query, n_rows, n_buckets = CASES[case]
    cells = check(g, c, rows, query, n_rows)
    assert cells.shape == (len(query[1]), n_buckets)


def test_unwrapped_ring_many_sort_tiles_and_one_long_cell(unwrapped):
    g, c, rows = unwrapped
    assert g.cursor < g.cfg.store_cap
    assert g.aggregate_store(ALL, NAMES, NOW - 60000, NOW, 1000)[1]["hot_since"] is None
    check(g, c, rows, (ALL, NAMES, NOW - 60000, NOW, 1000), 7964)            # more than one 4096-pair sort tile
    one = check(g, c, rows, (ALL, NAMES[:1], NOW - 60000, NOW, 60001), 983)  # one cell over four reduction tiles
    assert one["count"].tolist() == [[983]]
    for case in CASES:
        check(g, c, rows, case[:5])


def test_partial_wave_nan_signed_zeros_and_empty_ring():
    g, c = GpuInboundEngine(small_cfg()), CpuInboundEngine(small_cfg())
    query = ([1, 2], [hash64("temp"), hash64("hum")], NOW - 100, NOW - 71, 10)
    cells, info = g.aggregate_store(*query)                                   # cursor == 0: no kernel, zeroed cells
    assert info == {"rows": 0, "nan": 0, "hot_since": None} and "series" not in g._ring_bufs
    assert cells.shape == (2, 3) and not cells.tobytes().strip(b"\0")
    for e in (g, c):
        setup_fleet(e, n_dev=1000)
        assert e.step(*hand_series_batch(), NOW, presence=False).n_persisted == 7
    cells = check(g, c, c.store_rows(), query, 6)
    assert g.aggregate_store(*query)[1]["nan"] == 1
    assert cells["count"].tolist() == [[0, 2, 3], [1, 0, 0]]
    assert cells[0, 2]["min"] == -1e300 and cells[0, 2]["max"] == 1e300
    assert np.signbit(cells[0, 1]["first"]) != np.signbit(cells[0, 1]["last"])      # -0.0 and 0.0, by event id
    # a query nothing matches: counted on the device, nothing reduced
    none, info = g.aggregate_store([1, 2], [hash64("nope")], NOW - 100, NOW, 10)
    assert info["rows"] == 0 and not none.tobytes().strip(b"\0")


def test_same_bytes_every_call(wrapped, unwrapped):
    for g, _, _ in (wrapped, unwrapped):
        for case in CASES:
            a = g.aggregate_store(*case[:5])[0].tobytes()
            assert g.aggregate_store(*case[:5])[0].tobytes() == a
            total, _, _ = g.query_store(EV_MEASUREMENT, ALL, NOW - 60000, NOW, page_size=10)
            assert total > 0
            assert g.aggregate_store(*case[:5])[0].tobytes() == a


def test_steps_still_work_after_aggregating():
    g, c, rows = ring_pair(1 << 12)
    check(g, c, rows, CASES[1][:5])
    raw, offs = fleet_batch(1500, seed=99, n_dev=200)
    rg, rc = g.step(raw, offs, NOW + 9, presence=False), c.step(raw, offs, NOW + 9, presence=False)
    assert rg.n_events == rc.n_events and rg.n_persisted == rc.n_persisted
    assert canon_out(rg.out, c.names) == canon_out(rc.out, c.names)
    assert g.stats_dict() == c.stats_dict()
    rows = c.store_rows()
    for case in CASES[:4]:
        check(g, c, rows, case[:5])


def test_argument_errors_launch_nothing():
    g = fill_ring(GpuInboundEngine(small_cfg(store_cap=1 << 12)))
    for bad in ((ALL, NAMES, NOW - 1000, NOW, 0), (ALL, NAMES, NOW, NOW - 1, 10), (ALL, [], NOW - 1000, NOW, 10),
                (ALL, list(range(1, 66)), NOW - 1000, NOW, 10), (ALL, NAMES + NAMES[:1], NOW - 1000, NOW, 10),
                (ALL, NAMES, NOW - 8192, NOW, 1)):
        with pytest.raises(ValueError):
            g.aggregate_store(*bad)
    assert "series" not in g._ring_bufs              # nothing was allocated, so nothing was launched
    assert g.aggregate_store(ALL, NAMES, NOW - 8191, NOW, 1)[0].size == 65536
