"""Location density grids (``EngineBase.grid_store``) on the CPU engines -- the oracle of the MI355X
kernel (tests/test_gpu_grid.py) -- and through the service API, the search provider and REST."""
import math

import numpy as np
import pytest

from sitewhere_amd.models.columnar import (GRID_CELL, GRID_QUERY, GRID_QUERY_F64, NEAR_QUERY, POSITION_QUERY, RING_QUERY,
                                           ZONE_QUERY)
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.grid import (GRID_MAX_CELLS, check_grid_args, grid_cell_np, grid_select, grid_steps,
                                         host_grid)
from sitewhere_amd.pipeline.native_engine import NativeCpuEngine

from abi_header import HEADER, struct_fields
from grid_scenarios import (AROUND, BOXES, CROSSING, CUT, HAND_INFO, assert_conserved, assert_same_grid,
                            brute_force_grid, case_queries, hand_expected, hand_grid_batch)
from near_scenarios import RINGS
from pipeline_scenarios import NOW, setup_fleet, small_cfg
from series_scenarios import fill_ring
from test_near import HOME, T0, _north, site  # noqa: F401  (the instance with a hot tenant and a per-event one)

GRIDS = [("around", 1, 1), ("around", 8, 8), ("cut", 3, 5), ("crossing", 8, 8), ("crossing", 3, 5), ("around", 1, 300)]


@pytest.fixture(scope="module")
def rings():
    """Both CPU engines on both rings; they hold the same rows."""
    out = {}
    for cap in RINGS:
        engs = [fill_ring(cls(small_cfg(store_cap=cap))) for cls in (CpuInboundEngine, NativeCpuEngine)]
        cols, eids = engs[0].store_rows()
        c2, e2 = engs[1].store_rows()
        assert np.array_equal(eids, e2) and all(cols[k].tobytes() == c2[k].tobytes() for k in cols)
        out[cap] = engs, cols, eids
    return out


@pytest.mark.parametrize("box,n_rows,n_cols", GRIDS)
@pytest.mark.parametrize("cap", sorted(RINGS))
def test_oracle_matches_brute_force_and_conserves_on_every_case(rings, cap, box, n_rows, n_cols):
    engs, cols, eids = rings[cap]
    wrapped = engs[0].cursor > cap
    assert wrapped == (cap == 1 << 12)
    totals = []
    for q in case_queries(BOXES[box], n_rows, n_cols):
        want, cand, invalid, outside, n_asg = brute_force_grid(cols, eids, **q)
        answers = [eng.grid_store(**q) for eng in engs]
        assert_same_grid(answers[1], answers[0])
        cells, info = answers[0]
        assert info == {"candidates": cand, "invalid": invalid, "outside": outside,
                        "hot_since": int(cols["recv"][0]) if wrapped else None}
        assert_same_grid((cells, info), (want, info))
        assert_conserved(cells, info, q["latest"], n_asg)
        totals.append(int(cells["count"].sum()))
        if "asg_idx" not in q and "start" not in q:
            assert cand == RINGS[cap][0] and invalid == 0
            if q["latest"]:
                assert totals[-1] + outside == RINGS[cap][1]
            assert (outside == 0) == (box == "around")
    # what the cases are there to exercise: the subset and the sub-range narrow, latest drops rows
    assert 0 < totals[1] < totals[0] and 0 < totals[2] < totals[0] and 0 < totals[3] < totals[0]


def test_the_8_by_8_grid_fills_the_sixteen_inner_cells(rings):
    for cap, (lo, hi) in ((1 << 12, (10, 74)), (1 << 14, (36, 215))):
        cells, info = rings[cap][0][0].grid_store(*AROUND, 8, 8)
        inner = cells["count"][2:6, 2:6]
        assert inner.min() == lo and inner.max() == hi and cells["count"].sum() == inner.sum() == RINGS[cap][0]
        assert (cells["last_date"][2:6, 2:6] > NOW - 60000).all() and info["outside"] == 0


def _hand_engine(cls=CpuInboundEngine):
    eng = cls(small_cfg())
    setup_fleet(eng, n_dev=1000)
    res = eng.step(*hand_grid_batch(), NOW, presence=False)
    assert res.n_events == 21 and res.n_persisted == eng.cursor < 64      # less than one wave of rows
    return eng


@pytest.mark.parametrize("cls", [CpuInboundEngine, NativeCpuEngine])
def test_hand_batch_edges_boundaries_antimeridian_invalid_and_the_tie(cls):
    eng = _hand_engine(cls)
    cols, eids = eng.store_rows()
    for box, r, c, latest, want, outside in hand_expected():
        cells, info = eng.grid_store(*box, r, c, latest=latest)
        assert_same_grid((cells, info), (want, dict(HAND_INFO, outside=outside, hot_since=None)))
        assert_conserved(cells, info, latest, 16)
        assert_same_grid((brute_force_grid(cols, eids, *box, r, c, latest=latest)[0], info), (want, info))


def test_grid_cell_boundaries():
    box = (33.0, 34.0, -85.0, -84.0)
    # closed north and east edges: the quotient equals the cell count and is clamped
    inside, i, j = grid_cell_np(box, 2, 2, [34.0, 33.0, 33.5, 33.75, math.nextafter(34.0, 35.0)],
                                [-84.0, -85.0, -84.5, math.nextafter(-85.0, -86.0), -84.5])
    assert inside.tolist() == [True, True, True, False, False]
    assert (i[:3].tolist(), j[:3].tolist()) == ([1, 0, 1], [1, 0, 1])
    # a quotient that rounds up to the cell count below the edge: 3 columns of (1 - 0) / 3, the last double under 1
    d = grid_steps((0.0, 1.0, 0.0, 1.0), 3, 3)[1]
    x = math.nextafter(1.0, 0.0)
    assert int(x / d) == 3 and int(1.0 / d) == 3                     # without the clamp both name a fourth column
    inside, i, j = grid_cell_np((0.0, 1.0, 0.0, 1.0), 3, 3, [x, 1.0], [x, 1.0])
    assert inside.all() and i.tolist() == j.tolist() == [2, 2]
    # a crossing box: the western part's offset is negative until 360.0 is added
    cross = (-1.0, 1.0, 179.0, -179.0)
    assert grid_steps(cross, 1, 4) == (2.0, 0.5, True)
    inside, i, j = grid_cell_np(cross, 1, 4, [0.0] * 6, [179.0, 179.75, -179.75, -179.0, 178.9, -178.9])
    assert inside.tolist() == [True] * 4 + [False] * 2 and j[:4].tolist() == [0, 1, 2, 3] and not i.any()
    # lon -180 and 180: one meridian, not special-cased.  A crossing box holds both in one cell ...
    inside, _, j = grid_cell_np(cross, 1, 4, [0.0, 0.0], [180.0, -180.0])
    assert inside.all() and j.tolist() == [2, 2]
    # ... a box from -180 to 180 in its first and last column
    inside, _, j = grid_cell_np((-1.0, 1.0, -180.0, 180.0), 1, 4, [0.0, 0.0], [180.0, -180.0])
    assert inside.all() and j.tolist() == [3, 0]
    # grid_select: the tie by id, an invalid row, one outside
    cells, bad, out = grid_select([0, 0, 1, 2], [5, 5, 5, 7], [1, 2, 3, 4], [33.2, 33.7, 95.0, 35.0],
                                  [-84.7, -84.2, 0.0, -84.5], box, 2, 2, True)
    assert (bad, out) == (1, 1) and cells["count"].tolist() == [[0, 0], [0, 1]] and cells["last_date"][1, 1] == 5


def test_check_grid_args_refusals():
    ok = (33.0, 34.0, -85.0, -84.0, 8, 8)
    assert check_grid_args(*ok) == ((33.0, 34.0, -85.0, -84.0), 8, 8)
    assert check_grid_args(-90, 90, 180, -180, 1, GRID_MAX_CELLS)[1:] == (1, GRID_MAX_CELLS)
    nan, inf = float("nan"), float("inf")
    for bad in ((34.0, 33.0, -85.0, -84.0, 8, 8), (33.0, 33.0, -85.0, -84.0, 8, 8), (-90.5, 34.0, -85.0, -84.0, 8, 8),
                (33.0, 90.5, -85.0, -84.0, 8, 8), (33.0, 34.0, -180.5, -84.0, 8, 8), (33.0, 34.0, -85.0, 180.5, 8, 8),
                (33.0, 34.0, -85.0, -85.0, 8, 8), (33.0, 34.0, -85.0, -84.0, 0, 8), (33.0, 34.0, -85.0, -84.0, 8, 0),
                (33.0, 34.0, -85.0, -84.0, 256, 257), (33.0, 34.0, -85.0, -84.0, 1, GRID_MAX_CELLS + 1),
                (nan, 34.0, -85.0, -84.0, 8, 8), (33.0, inf, -85.0, -84.0, 8, 8), (33.0, 34.0, nan, -84.0, 8, 8),
                (33.0, 34.0, -85.0, -inf, 8, 8), (33.0, 34.0, -85.0, -84.0, 2.5, 8), (None, 34.0, -85.0, -84.0, 8, 8)):
        with pytest.raises(ValueError):
            check_grid_args(*bad)
    with pytest.raises(ValueError):
        check_grid_args(*ok, start=NOW, end=NOW - 1)
    eng = CpuInboundEngine(small_cfg())
    with pytest.raises(ValueError):
        eng.grid_store(33.0, 34.0, -85.0, -84.0, 300, 300)
    cells, info = eng.grid_store(*ok)                                # an empty ring
    assert cells.shape == (8, 8) and not cells.tobytes().strip(b"\0")
    assert info == {"candidates": 0, "invalid": 0, "outside": 0, "hot_since": None}


class _Ev:
    def __init__(self, asg, lat, lon, date):
        self.device_assignment_id, self.latitude, self.longitude, self.event_date = asg, lat, lon, date


def test_host_grid_equals_the_oracle(rings):
    engs, cols, eids = rings[1 << 14]
    loc = np.flatnonzero(cols["etype"] == 1)
    order = loc[np.lexsort((-eids[loc], -cols["date"][loc]))]          # newest first, as event management lists
    evs = [_Ev(int(cols["asg"][r]), float(cols["v0"][r]), float(cols["v1"][r]), int(cols["date"][r])) for r in order]
    evs.append(_Ev(7, None, 1.0, NOW - 10000))                         # no latitude: invalid
    for box, n_rows, n_cols in ((CUT, 3, 5), (CROSSING, 4, 4)):
        for latest in (False, True):
            for rng in ((None, None), (NOW - 45000, NOW - 5000)):
                cells, info = engs[0].grid_store(*box, n_rows, n_cols, start=rng[0], end=rng[1], latest=latest)
                got = host_grid(evs, *box, n_rows, n_cols, rng[0], rng[1], latest)
                assert got["hotSince"] is None and got["numResults"] == cells["count"].sum() > 0
                assert (got["outside"], got["invalid"]) == (info["outside"], info["invalid"] + 1)
                assert (got["rows"], got["cols"]) == (n_rows, n_cols)
                assert (got["latStep"], got["lonStep"]) == grid_steps(box, n_rows, n_cols)[:2]
                rr, cc = np.nonzero(cells["count"])
                assert [(c["row"], c["col"], c["count"], c["lastDate"]) for c in got["cells"]] == \
                    [(r, c, cells["count"][r, c], cells["last_date"][r, c]) for r, c in zip(rr, cc)]
    with pytest.raises(ValueError):
        host_grid(evs, 34.0, 33.0, -85.0, -84.0, 2, 2)


def test_grid_query_mirrors_header():
    text, fields = struct_fields("SwGridQuery")
    assert tuple(n for n, _ in fields) == GRID_QUERY and len(GRID_QUERY) == 24 and GRID_QUERY[:10] == RING_QUERY
    assert {t for _, t in fields} == {"ptr", "int64_t", "double"}                  # every field 8 bytes
    assert tuple(n for n, t in fields if t == "double") == GRID_QUERY_F64
    assert "static_assert(sizeof(SwGridQuery) == %d" % (8 * len(GRID_QUERY)) in text
    assert "#define SW_GRID_MAX_CELLS %d" % GRID_MAX_CELLS in text
    assert [n for n, _ in struct_fields("SwGridCell")[1]] == list(GRID_CELL.names) and GRID_CELL.itemsize == 16
    # the other queries' layouts mirror the header too: the three share k_near_best through one head, SwPositionView
    assert tuple(n for n, _ in struct_fields("SwNearQuery")[1]) == NEAR_QUERY
    assert tuple(n for n, _ in struct_fields("SwZoneQuery")[1]) == ZONE_QUERY
    assert NEAR_QUERY[:15] == ZONE_QUERY[:15] == GRID_QUERY[:15] == POSITION_QUERY
    assert tuple(n for n, _ in struct_fields("SwPositionView")[1]) == POSITION_QUERY
    assert "static_assert(sizeof(SwPositionView) == %d" % (8 * len(POSITION_QUERY)) in text
    # sw_abi_sizes reports the size the library was compiled with (compared on the GPU in
    # tests/test_gpu_grid.py, where the library loads): here, that the word it reports is this struct's
    assert "out[15] = sizeof(SwGridQuery);" in (HEADER.parent.parent / "hip" / "swgpu.hip").read_text()
    import inspect

    from sitewhere_amd.ops import engine_abi
    assert '"grid_query": buf[15]' in inspect.getsource(engine_abi.abi_sizes)


# ------------------------------------------------------------------------------ service API, provider and REST
GRID = "/sitewhere/api/search/%s/locations/grid"


def test_service_provider_and_rest_on_the_hot_route(site, monkeypatch):  # noqa: F811
    run, api = site["run"], site["api"]
    # tab 1 walks north from HOME 100 m a step and ends 900 m out; tab 2 rests 250 m out, then 5 km away.
    # Four rows of 250 m from 75 m south of HOME: tab 1's steps fall 2, 3, 2, 3 to a row, tab 2's rest in the second.
    box = (_north(-75), _north(925), HOME[1] - 0.01, HOME[1] + 0.01)
    hot = run(lambda: api.locations_grid_hot(box, 4, 1))
    assert hot["hotSince"] is None and (hot["rows"], hot["cols"]) == (4, 1)
    assert (hot["numResults"], hot["outside"], hot["invalid"]) == (11, 1, 0)
    assert hot["cells"] == [{"row": 0, "col": 0, "count": 2, "lastDate": T0 + 10},
                            {"row": 1, "col": 0, "count": 4, "lastDate": T0 + 40},
                            {"row": 2, "col": 0, "count": 2, "lastDate": T0 + 60},
                            {"row": 3, "col": 0, "count": 3, "lastDate": T0 + 90}]
    assert hot["latStep"] == (box[1] - box[0]) / 4 and hot["lonStep"] == box[3] - box[2]
    # latest: where the tablets are now -- tab 1 in the last row, tab 2 outside
    now = run(lambda: api.locations_grid_hot(box, 4, 1, latest=True))
    assert (now["numResults"], now["outside"]) == (1, 1)
    assert now["cells"] == [{"row": 3, "col": 0, "count": 1, "lastDate": T0 + 90}]
    # ... and where they were at T0 + 40
    then = run(lambda: api.locations_grid_hot(box, 4, 1, T0, T0 + 40, latest=True))
    assert then["cells"] == [{"row": 1, "col": 0, "count": 2, "lastDate": T0 + 40}]
    one = run(lambda: api.locations_grid_hot(box, 4, 1, None, None, "Assignment", [site["asg"][1]]))
    assert (one["numResults"], one["outside"]) == (1, 1) and one["cells"][0]["lastDate"] == T0 + 35
    with pytest.raises(ValueError):
        run(lambda: api.locations_grid_hot((box[1], box[0], box[2], box[3]), 4, 1))
    # the provider takes the hot route (the ring has not wrapped) and REST shows its answer
    calls = []
    from sitewhere_amd.services.gpu_inbound import GpuInboundApi
    real = GpuInboundApi.locations_grid_hot
    monkeypatch.setattr(GpuInboundApi, "locations_grid_hot",
                        lambda self, *a, **k: calls.append(a[1:3]) or real(self, *a, **k))
    es = site["inst"].api("EventSearch", "col")
    crit = {"latMin": box[0], "latMax": box[1], "lonMin": box[2], "lonMax": box[3], "rows": 4, "cols": 1}
    assert run(lambda: es.get_locations_grid("events", crit)) == hot and calls == [(4, 1)]
    client, h = site["client"], site["col"]
    r = client.get(GRID % "events", headers=h, params=crit)
    assert r.status_code == 200, r.text
    assert r.json() == hot
    r = client.get(GRID % "events", headers=h, params=dict(crit, latest="true", startDate=T0, endDate=T0 + 40))
    assert r.json()["cells"] == then["cells"]
    # a crossing box that holds HOME: lonMin > lonMax
    r = client.get(GRID % "events", headers=h, params=dict(crit, lonMin=170.0, lonMax=HOME[1] + 0.01, cols=2))
    assert r.status_code == 200 and r.json()["numResults"] == 11 and {c["col"] for c in r.json()["cells"]} == {1}
    # refusals: a bad box, too many cells and a range the wrong way round are a 400, an unknown provider a 404
    for bad in ({"latMin": box[1], "latMax": box[0]}, {"latMax": 91}, {"lonMin": -180.5}, {"lonMax": box[2]}, {"rows": 0},
                {"rows": 257, "cols": 256}, {"latMin": "nan"}, {"startDate": T0 + 1, "endDate": T0}):
        assert client.get(GRID % "events", headers=h, params=dict(crit, **bad)).status_code == 400, bad
    assert client.get(GRID % "nope", headers=h, params=crit).status_code == 404
    from sitewhere_amd.core.errors import NotFoundException
    with pytest.raises(NotFoundException):
        run(lambda: es.get_locations_grid("nope", crit))
    assert len(calls) == 4                                       # no refused query reached the engine


def test_host_route_on_the_per_event_tenant(site):  # noqa: F811
    client, h = site["client"], site["default"]
    from sitewhere_amd.services.inbound_processing import InboundProcessingApi
    from sitewhere_amd.services.labels_media_search import SolrSearchProvider
    assert InboundProcessingApi(None).locations_grid_hot((0.0, 1.0, 0.0, 1.0), 2, 2) is None
    for dev in ("grid-dev-1", "grid-dev-2"):
        r = client.post("/sitewhere/api/devices", headers=h, json={"token": dev, "deviceTypeToken": "raspberrypi"})
        assert r.status_code == 200, r.text
        r = client.post("/sitewhere/api/assignments", headers=h, json={
            "token": dev.replace("dev", "asg"), "deviceToken": dev, "customerToken": "acme", "areaToken": "peachtree"})
        assert r.status_code == 200, r.text
    # an empty corner of the map: the dataset's own locations are far away
    home = (-45.0, 165.0)
    north = lambda m: home[0] + math.degrees(m / 6371000.0)  # noqa: E731
    for asg, m, d in (("grid-asg-1", 0, T0 + 1), ("grid-asg-1", 300, T0 + 2), ("grid-asg-1", 2000, T0 + 9),
                      ("grid-asg-2", 150, T0 + 2)):
        r = client.post(f"/sitewhere/api/assignments/{asg}/locations", headers=h,
                        json={"latitude": north(m), "longitude": home[1], "elevation": 0.0, "eventDate": d})
        assert r.status_code == 200, r.text
    # two rows of 250 m from 50 m south: 0 and 150 m in the first, 300 m in the second, 2 km outside ...
    crit = {"latMin": north(-50), "latMax": north(450), "lonMin": home[1] - 0.01, "lonMax": home[1] + 0.01, "rows": 2,
            "cols": 1}
    solr = SolrSearchProvider("solr", "http://localhost:1").get_locations_grid(crit)
    assert solr["cells"] == [] and solr["numResults"] == 0 and (solr["rows"], solr["cols"]) == (2, 1)
    got = client.get(GRID % "events", headers=h, params=crit)
    assert got.status_code == 200, got.text
    body = got.json()
    assert body["hotSince"] is None and body["numResults"] == 3 and body["invalid"] == 0
    assert body["cells"] == [{"row": 0, "col": 0, "count": 2, "lastDate": T0 + 2},
                             {"row": 1, "col": 0, "count": 1, "lastDate": T0 + 2}]
    assert body["latStep"] == (crit["latMax"] - crit["latMin"]) / 2 and set(body) == set(solr)
    # ... where the dataset's own locations are too: the box keeps them out of the cells, not out of `outside`
    assert body["outside"] >= 1
    latest = client.get(GRID % "events", headers=h, params=dict(crit, latest="true")).json()
    assert latest["cells"] == [{"row": 0, "col": 0, "count": 1, "lastDate": T0 + 2}]       # asg 1 ended 2 km out
    then = client.get(GRID % "events", headers=h, params=dict(crit, latest="true", endDate=T0 + 5)).json()
    assert then["cells"] == [{"row": 0, "col": 0, "count": 1, "lastDate": T0 + 2},
                             {"row": 1, "col": 0, "count": 1, "lastDate": T0 + 2}]
    assert client.get(GRID % "events", headers=h, params=dict(crit, latMax=crit["latMin"])).status_code == 400
    assert client.get(GRID % "events", headers=h, params=dict(crit, rows=70000)).status_code == 400
    assert client.get(GRID % "nope", headers=h, params=crit).status_code == 404
    from sitewhere_amd.client import SiteWhereClient
    assert callable(SiteWhereClient.locations_grid)
