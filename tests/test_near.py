"""Locations near a point (``EngineBase.near_store``) on the CPU engines -- the oracle of the MI355X
kernels (tests/test_gpu_near.py) -- and through the service API, the search provider and REST."""
import math

import numpy as np
import pytest

from sitewhere_amd.core.geo import haversine_m
from sitewhere_amd.models.columnar import NEAR_QUERY, NEAR_QUERY_F64
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.native_engine import NativeCpuEngine
from sitewhere_amd.pipeline.near import (NEAR_BAND_M, NEAR_MAX_RADIUS_M, check_near_args, haversine_np, host_near,
                                         in_box, near_box)

from abi_header import HEADER, struct_fields
from pipeline_scenarios import NOW, setup_fleet, small_cfg
from near_scenarios import (CENTRE, HAND_QUERIES, RADII, RINGS, assert_clear_of_band, brute_force_near, case_queries,
                            hand_near_batch)
from series_scenarios import fill_ring


@pytest.fixture(scope="module", params=sorted(RINGS))
def ring(request):
    eng = fill_ring(CpuInboundEngine(small_cfg(store_cap=request.param)))
    return eng, eng.store_rows(), RINGS[request.param]


def test_oracle_matches_brute_force_on_every_case(ring):
    eng, (cols, eids), (n_loc, n_asg, matches) = ring
    loc = cols["etype"] == 1
    assert int(loc.sum()) == n_loc and len(set(cols["asg"][loc].tolist())) == n_asg
    wrapped = eng.cursor > eng.cfg.store_cap
    for radius, n_match in zip(RADII, matches):
        assert_clear_of_band(cols, *CENTRE, radius)
        assert eng.near_store(*CENTRE, radius, page_size=0)[0] == n_match
        for q in case_queries(radius):
            total, pc, pe, dist, info = eng.near_store(**q)
            ids, want, cand, invalid = brute_force_near(cols, eids, **q)
            assert total == len(ids) == len(pe) and pe.tolist() == ids
            assert info == {"candidates": cand, "invalid": invalid, "hot_since": int(cols["recv"][0]) if wrapped else None}
            assert np.allclose(dist, want, rtol=0, atol=NEAR_BAND_M / 100) and dist.dtype == np.float64
            assert (pc["etype"] == 1).all() and (dist <= radius).all()
            if q["latest"]:
                assert len(set(pc["asg"].tolist())) == total              # one row per assignment at most
            if q["order"] == "distance":
                assert (np.diff(dist) >= 0).all()
            else:
                assert (np.diff(pc["date"]) <= 0).all()
    # what the cases are there to exercise: latest drops rows, the subset and the sub-range narrow
    full = eng.near_store(*CENTRE, 60000.0, page_size=0)[0]
    assert eng.near_store(*CENTRE, 60000.0, latest=True, page_size=0)[0] < full
    by_q = [eng.near_store(**q)[0] for q in case_queries(60000.0)[:3]]
    assert by_q[0] == full and 0 < by_q[1] < full and 0 < by_q[2] < full


def test_paging_cuts_the_whole_answer(ring):
    eng = ring[0]
    total, cols, eids, dist, info = eng.near_store(*CENTRE, 60000.0, order="distance", page_size=0)
    t2, c2, e2, d2, i2 = eng.near_store(*CENTRE, 60000.0, order="distance", page_number=3, page_size=50)
    assert (t2, i2) == (total, info) and np.array_equal(e2, eids[100:150]) and np.array_equal(d2, dist[100:150])
    assert c2["v0"].tobytes() == cols["v0"][100:150].tobytes()
    assert len(eng.near_store(*CENTRE, 60000.0, page_number=99, page_size=50)[2]) == 0
    assert len(eng.near_store(*CENTRE, 60000.0)[2]) == 100                 # the default page


def test_haversine_is_geo_haversine():
    rng = np.random.default_rng(3)
    lat, lon = rng.uniform(-90, 90, 500), rng.uniform(-180, 180, 500)
    for la, lo in ((33.5, -84.5), (0.0, 180.0), (90.0, 0.0), (-47.25, 13.0)):
        d = haversine_np(la, lo, lat, lon)
        want = np.array([haversine_m(la, lo, a, b) for a, b in zip(lat, lon)])
        # the same operations; numpy's sin / cos / arcsin are not libm's to the last bit, which inside the
        # radius cap stays a hundred times under the band (the cap is there for that)
        capped = want <= NEAR_MAX_RADIUS_M
        assert capped.sum() > 100 and (np.abs(d - want)[capped] <= NEAR_BAND_M / 100).all()
        assert np.allclose(d, want, rtol=1e-12, atol=0)
    assert haversine_np(33.5, -84.5, [33.5], [-84.5])[0] == 0.0


def test_box_excludes_only_rows_past_the_radius():
    rng = np.random.default_rng(4)
    centres = [(33.5, -84.5), (0.0, 180.0), (0.0, -180.0), (89.9, 10.0), (90.0, 0.0), (-90.0, 0.0), (-89.99, 179.0),
               (60.0, 179.9), (10.0, -179.99), (85.0, 0.0)]
    for la, lo in centres:
        for radius in (0.0, 1.0, 100.0, 25000.0, 2.5e5, 1.2e6, 5e6, NEAR_MAX_RADIUS_M):
            box = near_box(la, lo, radius)
            assert -90 <= box[0] <= box[1] <= 90 and -180 <= box[2] <= 180 and -180 <= box[3] <= 180
            # points spread over the globe and points crowded around the cap's rim
            delta = math.degrees(radius / 6371000.0)
            lat = np.r_[rng.uniform(-90, 90, 2000), np.clip(la + rng.uniform(-1.5, 1.5, 2000) * delta, -90, 90)]
            lon = np.r_[rng.uniform(-180, 180, 2000), rng.uniform(-180, 180, 2000)]
            dist = haversine_np(la, lo, lat, lon)
            outside = ~in_box(box, lat, lon)
            assert (dist[outside] > radius + NEAR_BAND_M).all(), (la, lo, radius)
            rim = np.abs(dist - radius) < 1e-3 * max(radius, 1.0)
            assert in_box(box, lat, lon)[rim & (dist <= radius)].all()
    # a small cap is a small box, a wrapped one across the antimeridian, a polar one the whole circle
    assert near_box(33.5, -84.5, 1000.0)[1] - near_box(33.5, -84.5, 1000.0)[0] < 0.02
    lo_, hi_ = near_box(0.0, 180.0, 100.0)[2:]
    assert lo_ > hi_ and lo_ > 179.99 and hi_ < -179.99
    assert near_box(89.9999, 0.0, 100.0)[2:] == (-180.0, 180.0)


def test_check_near_args_refusals():
    assert check_near_args(33, -84, 10) == (33.0, -84.0, 10.0)
    assert check_near_args(90, 180, 0, 5, 5, "distance") == (90.0, 180.0, 0.0)
    assert check_near_args(-90, -180, NEAR_MAX_RADIUS_M)[2] == NEAR_MAX_RADIUS_M
    nan, inf = float("nan"), float("inf")
    for bad in ((90.0001, 0, 1), (-91, 0, 1), (nan, 0, 1), (0, 180.5, 1), (0, -inf, 1), (0, nan, 1), (0, 0, -1e-9),
                (0, 0, nan), (0, 0, inf), (0, 0, NEAR_MAX_RADIUS_M + 1), (0, 0, 1, 10, 9), (0, 0, 1, None, None, "nearest")):
        with pytest.raises(ValueError):
            check_near_args(*bad)
    for cls in (CpuInboundEngine, NativeCpuEngine):
        eng = cls(small_cfg())
        with pytest.raises(ValueError):
            eng.near_store(91, 0, 1)
        total, cols, eids, dist, info = eng.near_store(0, 0, 1)                 # an empty ring
        assert total == 0 and len(eids) == len(dist) == len(cols["v0"]) == 0
        assert info == {"candidates": 0, "invalid": 0, "hot_since": None}


@pytest.mark.parametrize("cls", [CpuInboundEngine, NativeCpuEngine])
def test_hand_batch(cls):
    eng = cls(small_cfg())
    setup_fleet(eng, n_dev=1000)
    assert eng.step(*hand_near_batch(), NOW, presence=False).n_persisted >= 12
    cols, eids = eng.store_rows()
    for la, lo, radius, n_all, n_latest in HAND_QUERIES:
        assert_clear_of_band(cols, la, lo, radius)
        for latest, n in ((False, n_all), (True, n_latest)):
            for order in ("date", "distance"):
                total, pc, pe, dist, info = eng.near_store(la, lo, radius, latest=latest, order=order)
                ids, want, cand, invalid = brute_force_near(cols, eids, la, lo, radius, latest=latest, order=order)
                assert total == n and pe.tolist() == ids and np.allclose(dist, want, rtol=0, atol=1e-8)
                assert info == {"candidates": 12, "invalid": 3, "hot_since": None} == {
                    "candidates": cand, "invalid": invalid, "hot_since": None}
    by_asg = lambda r: dict(zip(r[1]["asg"].tolist(), zip(r[1]["v0"].tolist(), r[3].tolist())))  # noqa: E731
    a = by_asg(eng.near_store(33.5, -84.5, 100.0, latest=True))
    assert set(a) == {1, 8}                       # device 2's newest row is outside: absent
    assert a[1][0] == 33.5001                     # device 1: two rows at one date, the later event id wins
    assert a[8][0] == 33.5003                     # device 8: its newer row is invalid, the valid one is its newest
    allrows = eng.near_store(33.5, -84.5, 100.0, order="distance")
    assert allrows[3][0] == 0.0 and allrows[1]["asg"].tolist() == [1, 1, 2, 8]
    assert eng.near_store(33.5, -84.5, 100.0, asg_idx=[2, 8])[1]["asg"].tolist() == [8, 2]      # date order
    assert eng.near_store(33.5, -84.5, 100.0, start=NOW - 60, end=NOW - 50)[0] == 3
    am = eng.near_store(0.0, 180.0, 100.0)
    assert sorted(am[1]["v1"].tolist()) == [-179.9995, 179.9995] and np.allclose(am[3], 55.5974633, atol=1e-6)
    assert eng.near_store(90.0, 0.0, 100.0)[1]["v0"].tolist() == [89.9999]


def test_host_near_matches_the_oracle():
    from sitewhere_amd.models.domain import DeviceLocation
    eng = CpuInboundEngine(small_cfg())
    setup_fleet(eng, n_dev=1000)
    eng.step(*hand_near_batch(), NOW, presence=False)
    big = fill_ring(CpuInboundEngine(small_cfg(store_cap=1 << 14)))
    for e in (eng, big):
        # event management lists newest first; equal dates then go by listing order
        _, cols, eids = e.query_store(1, range(1000), page_size=0)
        evs = [DeviceLocation(id=str(int(i)), device_assignment_id=str(int(a)), event_date=int(d), latitude=float(la),
                              longitude=float(lo)) for i, a, d, la, lo in
               zip(eids, cols["asg"], cols["date"], cols["v0"], cols["v1"])]
        queries = [dict(lat=la, lon=lo, radius_m=r) for la, lo, r, _, _ in HAND_QUERIES] if e is eng else \
            [dict(lat=CENTRE[0], lon=CENTRE[1], radius_m=r) for r in RADII]
        for q in queries:
            for extra in (dict(), dict(latest=True), dict(order="distance"), dict(latest=True, order="distance"),
                          dict(start=NOW - 45000, end=NOW - 33), dict(page_number=2, page_size=7)):
                total, _, pe, dist, _ = e.near_store(**q, **extra)
                got = host_near(evs, q["lat"], q["lon"], q["radius_m"], **extra)
                assert got["hotSince"] is None and got["numResults"] == total
                assert [int(ev.id) for ev in got["results"]] == pe.tolist()
                assert got["distances"] == dist.tolist()
    with pytest.raises(ValueError):
        host_near([], 0, 0, -1)
    assert host_near([], 0, 0, 1) == {"hotSince": None, "numResults": 0, "results": [], "distances": []}


def test_near_query_mirrors_header():
    text, fields = struct_fields("SwNearQuery")
    assert tuple(n for n, _ in fields) == NEAR_QUERY
    assert {t for _, t in fields} == {"ptr", "int64_t", "double"}                  # every field 8 bytes
    assert tuple(n for n, t in fields if t == "double") == NEAR_QUERY_F64
    assert "static_assert(sizeof(SwNearQuery) == %d" % (8 * len(NEAR_QUERY)) in text
    # sw_abi_sizes reports the size the library was compiled with (compared on the GPU in
    # tests/test_gpu_near.py, where the library loads): here, that the word it reports is this struct's
    assert "out[11] = sizeof(SwNearQuery);" in (HEADER.parent.parent / "hip" / "swgpu.hip").read_text()
    import inspect

    from sitewhere_amd.ops import engine_abi
    assert '"near_query": buf[11]' in inspect.getsource(engine_abi.abi_sizes)


# ------------------------------------------------------------------------------ service API, provider and REST
T0 = 1_700_000_000_000
HOME = (33.75, -84.39)


def _north(metres):
    """A latitude ``metres`` north of HOME's."""
    return HOME[0] + math.degrees(metres / 6371000.0)


@pytest.fixture(scope="module")
def site():
    """An instance with a ``gpu-columnar`` tenant (hot store) next to the per-event ``default`` tenant."""
    import base64
    import time

    from fastapi.testclient import TestClient

    from conftest import engine_knows
    from sitewhere_amd.assembly import SiteWhereInstance
    from sitewhere_amd.models import wire
    inst = SiteWhereInstance().start()
    try:
        inst.wait_for_tenant("default", 60)
        tm = inst.api("TenantManagement")
        inst.instance.system_user.run(lambda: tm.create_tenant({
            "token": "col", "name": "Columnar", "authenticationToken": "col-auth",
            "configurationTemplateId": "gpu-columnar", "datasetTemplateId": "construction"}))
        inst.wait_for_tenant("col", 60)
        run = lambda f: inst.instance.system_user.run(f, "col")  # noqa: E731
        dm = inst.api("DeviceManagement", "col")
        devs = [run(lambda t=t: dm.get_device_by_token(t)) for t in ("galaxytab-001", "galaxytab-002")]
        ib = inst.tenant_engine("inbound-processing", "col")
        end = time.time() + 10
        while not all(engine_knows(ib, d) for d in devs) and time.time() < end:
            time.sleep(0.02)
        api = inst.api("InboundProcessing", "col")
        # tab 1 walks north from HOME, 100 m a step, and ends 900 m out; tab 2 rests 250 m out, then 5 km away
        msgs = [wire.location("galaxytab-001", _north(100 * i), HOME[1], event_date=T0 + 10 * i) for i in range(10)]
        msgs += [wire.location("galaxytab-002", _north(250), HOME[1], event_date=T0 + 35),
                 wire.location("galaxytab-002", _north(5000), HOME[1], event_date=T0 + 200)]
        assert run(lambda: api.process_payloads(msgs))["persisted"] >= 12
        client = TestClient(inst.rest_app)
        r = client.get("/sitewhere/authapi/jwt",
                       headers={"Authorization": "Basic " + base64.b64encode(b"admin:password").decode()})
        h = {"Authorization": f"Bearer {r.headers['X-Sitewhere-JWT']}"}
        yield {"run": run, "api": api, "client": client, "inst": inst,
               "asg": [d.device_assignment_id for d in devs],
               "col": dict(h, **{"X-SiteWhere-Tenant-Id": "col", "X-SiteWhere-Tenant-Auth": "col-auth"}),
               "default": dict(h, **{"X-SiteWhere-Tenant-Id": "default",
                                     "X-SiteWhere-Tenant-Auth": "sitewhere1234567890"})}
    finally:
        inst.stop()


NEAR = "/sitewhere/api/search/%s/locations/near"


def test_service_provider_and_rest_on_the_hot_route(site):
    run, api = site["run"], site["api"]
    hot = run(lambda: api.locations_near_hot(HOME[0], HOME[1], 450.0, None, None))
    assert hot["hotSince"] is None and hot["numResults"] == 6 == len(hot["results"]) == len(hot["distances"])
    # date order: tab 1 at 400 m, tab 2's rest between tab 1's 300 m and 400 m rows, then tab 1 down to 0
    assert [ev.event_date for ev in hot["results"]] == [T0 + 40, T0 + 35, T0 + 30, T0 + 20, T0 + 10, T0]
    assert np.allclose(hot["distances"], [400, 250, 300, 200, 100, 0], atol=1e-6) and hot["distances"][-1] == 0.0
    assert hot["results"][1].device_assignment_id == site["asg"][1] and hot["results"][0].latitude == _north(400)
    near = run(lambda: api.locations_near_hot(HOME[0], HOME[1], 450.0, None, None, order="distance"))
    assert np.allclose(near["distances"], [0, 100, 200, 250, 300, 400], atol=1e-6)
    # latest: tab 1's newest row is 900 m out, tab 2's 5 km out
    assert run(lambda: api.locations_near_hot(HOME[0], HOME[1], 450.0, None, None, latest=True))["numResults"] == 0
    last = run(lambda: api.locations_near_hot(HOME[0], HOME[1], 1000.0, None, None, latest=True))
    assert [ev.event_date for ev in last["results"]] == [T0 + 90] and abs(last["distances"][0] - 900) < 1e-6
    # ... but within a period that ends at T0 + 50 each tablet's last known position was near
    then = run(lambda: api.locations_near_hot(HOME[0], HOME[1], 1000.0, T0, T0 + 50, latest=True, order="distance"))
    assert [ev.event_date for ev in then["results"]] == [T0 + 35, T0 + 50]
    one = run(lambda: api.locations_near_hot(HOME[0], HOME[1], 450.0, None, None, "Assignment", [site["asg"][1]]))
    assert one["numResults"] == 1 and one["results"][0].device_assignment_id == site["asg"][1]
    with pytest.raises(ValueError):
        run(lambda: api.locations_near_hot(95.0, 0.0, 1.0, None, None))
    # the provider takes the hot route (the ring has not wrapped) and REST shows its answer
    es = site["inst"].api("EventSearch", "col")
    got = run(lambda: es.get_locations_near("events", HOME[0], HOME[1], 450.0, {"pageSize": 4, "order": "distance"}))
    assert got["numResults"] == 6 and np.allclose(got["distances"], [0, 100, 200, 250], atol=1e-6)
    client, h = site["client"], site["col"]
    r = client.get(NEAR % "events", headers=h, params={"latitude": HOME[0], "longitude": HOME[1], "distance": 450,
                                                       "order": "distance", "page": 2, "pageSize": 4})
    assert r.status_code == 200, r.text
    body = r.json()
    assert body["numResults"] == 6 and [round(x["distance"]) for x in body["results"]] == [300, 400]
    assert body["results"][0]["latitude"] == _north(300) and body["results"][0]["eventType"] == "Location"
    r = client.get(NEAR % "events", headers=h, params={"latitude": HOME[0], "longitude": HOME[1], "distance": 1000,
                                                       "latest": "true", "startDate": T0, "endDate": T0 + 50})
    assert [x["eventDate"] for x in r.json()["results"]] == [T0 + 50, T0 + 35]
    for bad in ({"latitude": 91}, {"longitude": -180.5}, {"distance": -1}, {"distance": 2e7}, {"order": "nearest"},
                {"startDate": T0 + 1, "endDate": T0}, {"latitude": "nan"}):
        params = dict({"latitude": HOME[0], "longitude": HOME[1], "distance": 450}, **bad)
        assert client.get(NEAR % "events", headers=h, params=params).status_code == 400, bad
    assert client.get(NEAR % "nope", headers=h, params={"latitude": 0, "longitude": 0, "distance": 1}).status_code == 404


def test_host_route_on_the_per_event_tenant(site):
    client, h = site["client"], site["default"]
    from sitewhere_amd.services.inbound_processing import InboundProcessingApi
    from sitewhere_amd.services.labels_media_search import SolrSearchProvider
    assert InboundProcessingApi(None).locations_near_hot(0.0, 0.0, 1.0, None, None) is None
    assert SolrSearchProvider("solr", "http://localhost:1")\
        .get_locations_near(0.0, 0.0, 1.0)["results"] == []
    for dev in ("near-dev-1", "near-dev-2"):
        r = client.post("/sitewhere/api/devices", headers=h, json={"token": dev, "deviceTypeToken": "raspberrypi"})
        assert r.status_code == 200, r.text
        r = client.post("/sitewhere/api/assignments", headers=h, json={
            "token": dev.replace("dev", "asg"), "deviceToken": dev, "customerToken": "acme", "areaToken": "peachtree"})
        assert r.status_code == 200, r.text
    # an empty corner of the map: the dataset's own locations are far away
    home = (-45.0, 170.0)
    north = lambda m: home[0] + math.degrees(m / 6371000.0)  # noqa: E731
    for asg, m, d in (("near-asg-1", 0, T0 + 1), ("near-asg-1", 300, T0 + 2), ("near-asg-1", 2000, T0 + 9),
                      ("near-asg-2", 150, T0 + 2)):
        r = client.post(f"/sitewhere/api/assignments/{asg}/locations", headers=h,
                        json={"latitude": north(m), "longitude": home[1], "elevation": 0.0, "eventDate": d})
        assert r.status_code == 200, r.text
    args = {"latitude": home[0], "longitude": home[1], "distance": 500}
    got = client.get(NEAR % "events", headers=h, params=args)
    assert got.status_code == 200, got.text
    body = got.json()
    assert body["numResults"] == 3 and [x["eventDate"] for x in body["results"]] == [T0 + 2, T0 + 2, T0 + 1]
    assert sorted(round(x["distance"]) for x in body["results"][:2]) == [150, 300] and body["results"][2]["distance"] == 0.0
    by_dist = client.get(NEAR % "events", headers=h, params=dict(args, order="distance")).json()
    assert [round(x["distance"]) for x in by_dist["results"]] == [0, 150, 300]
    assert by_dist["results"][1]["latitude"] == north(150)
    latest = client.get(NEAR % "events", headers=h, params=dict(args, latest="true")).json()
    assert latest["numResults"] == 1 and round(latest["results"][0]["distance"]) == 150      # asg 1 ended 2 km out
    then = client.get(NEAR % "events", headers=h, params=dict(args, latest="true", endDate=T0 + 5, order="distance")).json()
    assert [round(x["distance"]) for x in then["results"]] == [150, 300]
    assert client.get(NEAR % "events", headers=h, params=dict(args, distance=-5)).status_code == 400
    assert client.get(NEAR % "events", headers=h, params=dict(args, latitude=-90.5)).status_code == 400
    from sitewhere_amd.client import SiteWhereClient
    assert callable(SiteWhereClient.locations_near)
