"""Locations in a zone (``EngineBase.zone_store``) on the CPU engines -- the oracle of the MI355X
kernel (tests/test_gpu_zone.py) -- and through the service API, the search provider and REST."""
import math

import numpy as np
import pytest

from sitewhere_amd.core.geo import contains, polygon_of
from sitewhere_amd.models.columnar import GRID_QUERY, NEAR_QUERY, POSITION_QUERY, ZONE_QUERY, ZONE_QUERY_F64
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.native_engine import NativeCpuEngine
from sitewhere_amd.pipeline.zone import (ZONE_MAX_VTX, check_zone_args, contains_np, host_zone, in_zone_box, zone_box,
                                         zone_select)

from abi_header import HEADER, struct_fields
from pipeline_scenarios import NOW, setup_fleet, small_cfg
from near_scenarios import RINGS, SUB_RANGE, SUBSET, hand_near_batch
from series_scenarios import fill_ring
from test_near import HOME, T0, _north, site  # noqa: F401  (the instance with a hot tenant and a per-event one)
from zone_scenarios import (EXPECTED, HAND_INFO, HAND_RECTS, POLYGONS, assert_same_zone_answer, brute_force_zone,
                            case_queries, expected_total, inside_flags, rect)


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


@pytest.mark.parametrize("name", sorted(POLYGONS))
@pytest.mark.parametrize("cap", sorted(RINGS))
def test_oracle_matches_brute_force_on_every_case(rings, cap, name):
    engs, cols, eids = rings[cap]
    poly = POLYGONS[name]
    flags = inside_flags(cols, poly, key=(cap, name))
    wrapped = engs[0].cursor > cap
    assert wrapped == (cap == 1 << 12)
    for q in case_queries(poly):
        ids, cand, invalid = brute_force_zone(cols, eids, flags, **q)
        plain = "asg_idx" not in q and "start" not in q
        if plain:
            assert len(ids) == expected_total(cap, name, q["outside"], q["latest"])
        answers = [eng.zone_store(**q) for eng in engs]
        assert_same_zone_answer(answers[1], answers[0])
        total, pc, pe, info = answers[0]
        assert total == len(ids) == len(pe) and pe.tolist() == ids
        assert info == {"candidates": cand, "invalid": invalid, "hot_since": int(cols["recv"][0]) if wrapped else None}
        assert (pc["etype"] == 1).all() and (np.diff(pc["date"]) <= 0).all()
        if q["latest"]:
            assert len(set(pc["asg"].tolist())) == total              # one row per assignment at most
        if plain and not q["latest"] and not q["outside"]:
            assert info["candidates"] == RINGS[cap][0] and invalid == 0
    # what the cases are there to exercise: the subset and the sub-range narrow, latest drops rows
    if name != "world":
        by_q = [engs[0].zone_store(**q)[0] for q in case_queries(poly)[:6]]
        assert 0 < by_q[1] < by_q[0] and 0 < by_q[2] < by_q[0] and 0 < by_q[3] < by_q[0]


def test_paging_cuts_the_whole_answer(rings):
    eng = rings[1 << 14][0][0]
    poly = POLYGONS["ell"]
    total, cols, eids, info = eng.zone_store(poly, page_size=0)
    t2, c2, e2, i2 = eng.zone_store(poly, page_number=3, page_size=50)
    assert (t2, i2) == (total, info) and np.array_equal(e2, eids[100:150])
    assert all(c2[k].tobytes() == cols[k][100:150].tobytes() for k in cols)
    assert len(eng.zone_store(poly, page_number=99, page_size=50)[2]) == 0
    assert len(eng.zone_store(poly)[2]) == 100                     # the default page


def _hand_engine(cls=CpuInboundEngine):
    eng = cls(small_cfg())
    setup_fleet(eng, n_dev=1000)
    assert eng.step(*hand_near_batch(), NOW, presence=False).n_persisted >= 12
    return eng


def _points(rings):
    """Valid positions to try a predicate on: the big ring's locations, the hand batch's, and points on the
    polygons' own vertices and edge midpoints."""
    cols = rings[1 << 14][1]
    loc = cols["etype"] == 1
    hand = _hand_engine().store_rows()[0]
    ok = (hand["etype"] == 1) & (np.abs(hand["v0"]) <= 90) & (np.abs(hand["v1"]) <= 180)
    lat, lon = [cols["v0"][loc], hand["v0"][ok]], [cols["v1"][loc], hand["v1"][ok]]
    for p in list(POLYGONS.values()) + [r for _, r, _, _ in HAND_RECTS]:
        p = p[:64]
        mid = (p + np.roll(p, 1, axis=0)) / 2
        lat += [p[:, 0], mid[:, 0]]
        lon += [p[:, 1], mid[:, 1]]
    return np.concatenate(lat), np.concatenate(lon)


def test_contains_np_is_geo_contains_and_the_box_excludes_nothing_inside(rings):
    lat, lon = _points(rings)
    assert len(lat) > 2000
    for name, poly in list(POLYGONS.items()) + [(n, r) for n, r, _, _ in HAND_RECTS]:
        got = contains_np(poly, lat, lon)
        pts = range(len(lat)) if len(poly) < 100 else range(0, len(lat), 7)          # circ: every seventh point
        assert all(bool(got[i]) == contains(poly, float(lat[i]), float(lon[i])) for i in pts), name
        box = zone_box(poly)
        assert -90 <= box[0] <= box[1] <= 90 and -180 <= box[2] <= box[3] <= 180
        assert box[2] == poly[:, 1].min() and box[3] == poly[:, 1].max()
        assert 0 <= poly[:, 0].min() - box[0] <= 1.01e-9 and 0 <= box[1] - poly[:, 0].max() <= 1.01e-9      # the pad, rounded
        assert not (got & ~in_zone_box(box, lat, lon)).any(), name
        if name != "world":
            assert got.any() or name in ("east edge", "north edge", "north-east vertex")
            assert (~in_zone_box(box, lat, lon)).any()
    # the box is inclusive: the vertices themselves are in it
    for poly in POLYGONS.values():
        assert in_zone_box(zone_box(poly), poly[:, 0], poly[:, 1]).all()


def test_check_zone_args_refusals():
    tri = POLYGONS["tri"]
    assert check_zone_args(tri.tolist()).dtype == np.float64 and check_zone_args(tri, 5, 5).shape == (3, 2)
    assert len(check_zone_args(POLYGONS["circ"])) == ZONE_MAX_VTX == 1024
    big = np.vstack([POLYGONS["circ"], POLYGONS["circ"][:1]])
    assert len(check_zone_args(big, max_vtx=None)) == 1025
    nan = float("nan")
    for bad in (tri[:2], big, np.vstack([tri, [[nan, 0.0]]]), np.vstack([tri, [[90.5, 0.0]]]),
                np.vstack([tri, [[0.0, -180.5]]]), np.vstack([tri, [[0.0, float("inf")]]]), tri.reshape(-1), "zone"):
        with pytest.raises(ValueError):
            check_zone_args(bad)
    with pytest.raises(ValueError):
        check_zone_args(tri, 10, 9)
    for cls in (CpuInboundEngine, NativeCpuEngine):
        eng = cls(small_cfg())
        with pytest.raises(ValueError):
            eng.zone_store(tri[:2])
        with pytest.raises(ValueError):
            eng.zone_store(tri, start=NOW, end=NOW - 1)
        total, cols, eids, info = eng.zone_store(tri)                             # an empty ring
        assert total == 0 and len(eids) == len(cols["v0"]) == 0
        assert info == {"candidates": 0, "invalid": 0, "hot_since": None}


@pytest.mark.parametrize("cls", [CpuInboundEngine, NativeCpuEngine])
def test_hand_batch(cls):
    eng = _hand_engine(cls)
    cols, eids = eng.store_rows()
    for name, poly, inside, outside in HAND_RECTS:
        flags = inside_flags(cols, poly)
        for out, counts in ((False, inside), (True, outside)):
            if counts is None:
                continue
            for latest, n in ((False, counts[0]), (True, counts[1])):
                total, pc, pe, info = eng.zone_store(poly, outside=out, latest=latest)
                ids, cand, invalid = brute_force_zone(cols, eids, flags, outside=out, latest=latest)
                assert total == n == len(ids) and pe.tolist() == ids, (name, out, latest)
                assert info == HAND_INFO == {"candidates": cand, "invalid": invalid, "hot_since": None}
    small = HAND_RECTS[0][1]
    a = eng.zone_store(small)
    assert a[1]["asg"].tolist() == [1, 1] and a[1]["v0"].tolist() == [33.5001, 33.5]       # the later event id first
    assert eng.zone_store(small, latest=True)[1]["v0"].tolist() == [33.5001]
    # device 2's newest row is outside `small`, device 8's newest valid row is its older one
    latest_out = eng.zone_store(small, outside=True, latest=True)
    assert sorted(latest_out[1]["asg"].tolist()) == [2, 3, 4, 5, 8, 10]
    assert eng.zone_store(small, asg_idx=[1, 2], outside=True)[1]["asg"].tolist() == [2, 2]
    assert eng.zone_store(rect(33.4, 33.6, -84.6, -84.4), start=NOW - 60, end=NOW - 50)[0] == 3


def test_host_zone_matches_the_oracle(rings):
    from sitewhere_amd.models.domain import DeviceLocation
    big = rings[1 << 14][0][0]
    for e, polys in ((_hand_engine(), [r for _, r, _, _ in HAND_RECTS]), (big, list(POLYGONS.values()))):
        # event management lists newest first; equal dates then go by listing order
        _, cols, eids = e.query_store(1, range(1000), page_size=0)
        evs = [DeviceLocation(id=str(int(i)), device_assignment_id=str(int(a)), event_date=int(d), latitude=float(la),
                              longitude=float(lo)) for i, a, d, la, lo in
               zip(eids, cols["asg"], cols["date"], cols["v0"], cols["v1"])]
        for poly in polys:
            for extra in (dict(), dict(latest=True), dict(outside=True), dict(outside=True, latest=True),
                          dict(start=NOW - 45000, end=NOW - 33), dict(page_number=2, page_size=7)):
                total, _, pe, _ = e.zone_store(poly, **extra)
                got = host_zone(evs, poly, **extra)
                assert got["hotSince"] is None and got["numResults"] == total
                assert [int(ev.id) for ev in got["results"]] == pe.tolist()
    with pytest.raises(ValueError):
        host_zone([], POLYGONS["tri"][:2])
    assert host_zone([], POLYGONS["tri"]) == {"hotSince": None, "numResults": 0, "results": []}
    # no vertex limit on the host: the 1024-gon with one vertex doubled answers as the 1024-gon
    more = np.vstack([POLYGONS["circ"][:1], POLYGONS["circ"]])
    assert host_zone(evs, more, page_size=0)["numResults"] == EXPECTED[1 << 14]["circ"][0]
    sel, bad = zone_select([0, 0, 1], [5, 6, 5], [1, 2, 3], [33.5, 95.0, 33.5], [-84.5, 0.0, -84.5], POLYGONS["tri"],
                           False, True)
    assert sel.tolist() == [2, 0] and bad == 1


def test_zone_query_mirrors_header():
    text, fields = struct_fields("SwZoneQuery")
    assert tuple(n for n, _ in fields) == ZONE_QUERY and len(ZONE_QUERY) == 22
    assert {t for _, t in fields} == {"ptr", "int64_t", "double"}                  # every field 8 bytes
    assert tuple(n for n, t in fields if t == "double") == ZONE_QUERY_F64
    assert "static_assert(sizeof(SwZoneQuery) == %d" % (8 * len(ZONE_QUERY)) in text
    assert "#define SW_ZONE_MAX_VTX %d" % ZONE_MAX_VTX in text
    # the near query's layout mirrors the header too: the queries share k_near_best through one head, SwPositionView
    assert tuple(n for n, _ in struct_fields("SwNearQuery")[1]) == NEAR_QUERY
    assert NEAR_QUERY[:15] == ZONE_QUERY[:15] == GRID_QUERY[:15] == POSITION_QUERY
    # sw_abi_sizes reports the size the library was compiled with (compared on the GPU in
    # tests/test_gpu_zone.py, where the library loads): here, that the word it reports is this struct's
    assert "out[14] = sizeof(SwZoneQuery);" in (HEADER.parent.parent / "hip" / "swgpu.hip").read_text()
    import inspect

    from sitewhere_amd.ops import engine_abi
    assert '"zone_query": buf[14]' in inspect.getsource(engine_abi.abi_sizes)


# ------------------------------------------------------------------------------ service API, provider and REST
ZONE = "/sitewhere/api/search/%s/locations/zone/%s"


def _bounds(poly):
    return [{"latitude": float(la), "longitude": float(lo)} for la, lo in poly]


def _make_zone(site, tenant, token, poly):  # noqa: F811
    inst = site["inst"]
    dm = inst.api("DeviceManagement", tenant)
    z = inst.instance.system_user.run(lambda: dm.create_zone({
        "token": token, "name": token, "areaToken": "peachtree", "bounds": _bounds(poly)}), tenant)
    assert np.array_equal(polygon_of(z.bounds), np.asarray(poly, np.float64))
    return z


def test_service_provider_and_rest_on_the_hot_route(site, monkeypatch):  # noqa: F811
    run, api = site["run"], site["api"]
    # tab 1 walks north from HOME 100 m a step and ends 900 m out; tab 2 rests 250 m out, then 5 km away
    band = rect(_north(150), _north(450), HOME[1] - 0.01, HOME[1] + 0.01)
    hot = run(lambda: api.locations_in_zone_hot(band, None, None))
    assert hot["hotSince"] is None and hot["numResults"] == 4 == len(hot["results"])
    assert [ev.event_date for ev in hot["results"]] == [T0 + 40, T0 + 35, T0 + 30, T0 + 20]
    assert hot["results"][1].device_assignment_id == site["asg"][1] and hot["results"][0].latitude == _north(400)
    assert run(lambda: api.locations_in_zone_hot(band, None, None, outside=True))["numResults"] == 8
    # latest: both tablets have left the band since ...
    assert run(lambda: api.locations_in_zone_hot(band, None, None, latest=True))["numResults"] == 0
    assert run(lambda: api.locations_in_zone_hot(band, None, None, outside=True, latest=True))["numResults"] == 2
    # ... but within a period that ends at T0 + 40 each tablet's last known position was inside
    then = run(lambda: api.locations_in_zone_hot(band, T0, T0 + 40, latest=True))
    assert [ev.event_date for ev in then["results"]] == [T0 + 40, T0 + 35]
    one = run(lambda: api.locations_in_zone_hot(band, None, None, "Assignment", [site["asg"][1]]))
    assert one["numResults"] == 1 and one["results"][0].device_assignment_id == site["asg"][1]
    with pytest.raises(ValueError):
        run(lambda: api.locations_in_zone_hot(band[:2], None, None))
    # the provider loads the zone, takes the hot route (the ring has not wrapped) and REST shows its answer
    _make_zone(site, "col", "band", band)
    calls = []
    from sitewhere_amd.services.gpu_inbound import GpuInboundApi
    real = GpuInboundApi.locations_in_zone_hot
    monkeypatch.setattr(GpuInboundApi, "locations_in_zone_hot",
                        lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    es = site["inst"].api("EventSearch", "col")
    got = run(lambda: es.get_locations_in_zone("events", "band", {"pageSize": 3}))
    assert got["numResults"] == 4 and [ev.event_date for ev in got["results"]] == [T0 + 40, T0 + 35, T0 + 30]
    assert calls == [4]
    client, h = site["client"], site["col"]
    r = client.get(ZONE % ("events", "band"), headers=h, params={"page": 2, "pageSize": 3})
    assert r.status_code == 200, r.text
    body = r.json()
    assert body["numResults"] == 4 and [x["eventDate"] for x in body["results"]] == [T0 + 20]
    assert body["results"][0]["latitude"] == _north(200) and body["results"][0]["eventType"] == "Location"
    r = client.get(ZONE % ("events", "band"), headers=h, params={"latest": "true", "startDate": T0, "endDate": T0 + 40})
    assert [x["eventDate"] for x in r.json()["results"]] == [T0 + 40, T0 + 35]
    assert client.get(ZONE % ("events", "band"), headers=h, params={"outside": "true"}).json()["numResults"] == 8
    # refusals: a range the wrong way round and a zone of 2 bounds are a 400, an unknown zone or provider a 404
    assert client.get(ZONE % ("events", "band"), headers=h,
                      params={"startDate": T0 + 1, "endDate": T0}).status_code == 400
    _make_zone(site, "col", "line", band[:2])
    assert client.get(ZONE % ("events", "line"), headers=h).status_code == 400
    assert client.get(ZONE % ("events", "no-such-zone"), headers=h).status_code == 404
    assert client.get(ZONE % ("nope", "band"), headers=h).status_code == 404
    from sitewhere_amd.core.errors import NotFoundException
    with pytest.raises(NotFoundException):
        run(lambda: es.get_locations_in_zone("events", "no-such-zone"))
    # a zone past the vertex limit never reaches the engine
    n_calls = len(calls)
    ring = [[_north(300) + 0.002 * math.cos(2 * math.pi * k / 1025), HOME[1] + 0.002 * math.sin(2 * math.pi * k / 1025)]
            for k in range(1025)]
    _make_zone(site, "col", "ring-1025", ring)
    r = client.get(ZONE % ("events", "ring-1025"), headers=h)
    assert r.status_code == 200 and len(calls) == n_calls


def test_host_route_on_the_per_event_tenant(site):  # noqa: F811
    client, h = site["client"], site["default"]
    from sitewhere_amd.services.inbound_processing import InboundProcessingApi
    from sitewhere_amd.services.labels_media_search import SolrSearchProvider
    assert InboundProcessingApi(None).locations_in_zone_hot(POLYGONS["tri"], None, None) is None
    assert SolrSearchProvider("solr", "http://localhost:1").get_locations_in_zone("z")["results"] == []
    for dev in ("zone-dev-1", "zone-dev-2"):
        r = client.post("/sitewhere/api/devices", headers=h, json={"token": dev, "deviceTypeToken": "raspberrypi"})
        assert r.status_code == 200, r.text
        r = client.post("/sitewhere/api/assignments", headers=h, json={
            "token": dev.replace("dev", "asg"), "deviceToken": dev, "customerToken": "acme", "areaToken": "peachtree"})
        assert r.status_code == 200, r.text
    # an empty corner of the map: the dataset's own locations are far away
    home = (-45.0, 175.0)
    north = lambda m: home[0] + math.degrees(m / 6371000.0)  # noqa: E731
    for asg, m, d in (("zone-asg-1", 0, T0 + 1), ("zone-asg-1", 300, T0 + 2), ("zone-asg-1", 2000, T0 + 9),
                      ("zone-asg-2", 150, T0 + 2)):
        r = client.post(f"/sitewhere/api/assignments/{asg}/locations", headers=h,
                        json={"latitude": north(m), "longitude": home[1], "elevation": 0.0, "eventDate": d})
        assert r.status_code == 200, r.text
    _make_zone(site, "default", "corner", rect(north(-50), north(500), home[1] - 0.01, home[1] + 0.01))
    got = client.get(ZONE % ("events", "corner"), headers=h)
    assert got.status_code == 200, got.text
    body = got.json()
    assert body["numResults"] == 3 and [x["eventDate"] for x in body["results"]] == [T0 + 2, T0 + 2, T0 + 1]
    assert sorted(x["latitude"] for x in body["results"]) == [north(0), north(150), north(300)]
    latest = client.get(ZONE % ("events", "corner"), headers=h, params={"latest": "true"}).json()
    assert latest["numResults"] == 1 and latest["results"][0]["latitude"] == north(150)       # asg 1 ended 2 km out
    then = client.get(ZONE % ("events", "corner"), headers=h, params={"latest": "true", "endDate": T0 + 5}).json()
    assert sorted(x["latitude"] for x in then["results"]) == [north(150), north(300)]
    # a zone of 1025 bounds is answered here too (the host route has no vertex limit)
    ring = [[north(150) + 0.002 * math.cos(2 * math.pi * k / 1025), home[1] + 0.002 * math.sin(2 * math.pi * k / 1025)]
            for k in range(1025)]
    _make_zone(site, "default", "corner-1025", ring)
    body = client.get(ZONE % ("events", "corner-1025"), headers=h).json()
    assert body["numResults"] == 3                                  # 0.002 degree is 222 m: 0, 150 and 300 m are inside
    _make_zone(site, "default", "corner-line", ring[:2])
    assert client.get(ZONE % ("events", "corner-line"), headers=h).status_code == 400
    assert client.get(ZONE % ("events", "no-such-zone"), headers=h).status_code == 404
    from sitewhere_amd.client import SiteWhereClient
    assert callable(SiteWhereClient.locations_in_zone)
