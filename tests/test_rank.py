"""Rankings of groups over the event ring (``EngineBase.rank_store``) on the CPU engines -- the oracle of
the MI355X kernels (tests/test_gpu_rank.py) -- and through the service API, the search provider and REST."""
import math

import numpy as np
import pytest

from sitewhere_amd.models.columnar import (EV_ALERT, EV_COMMAND_INVOCATION, EV_LOCATION, EV_MEASUREMENT, RANK_CELL,
                                           RANK_MAX_KEYS, RANK_QUERY, RING_QUERY)
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.native_engine import NativeCpuEngine
from sitewhere_amd.pipeline.rank import check_rank_args, host_rank, rank_key, rank_select

from abi_header import HEADER, struct_fields
from near_scenarios import RINGS
from pipeline_scenarios import NOW, small_cfg
from rank_scenarios import (COLUMN, GROUPS, HAND_ALERT_ASG, HAND_ROWS, KEY_SETS, RING_FACTS, TEMP, assert_conserved,
                            assert_same_rank, bits, brute_force_rank, hand_eids, hand_expected, hand_rank_batch,
                            hand_rank_fleet, ring_queries, total_order_key)
from series_scenarios import NAMES, fill_ring
from test_near import T0, site  # noqa: F401  (the instance with a hot tenant and a per-event one)


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


@pytest.mark.parametrize("cap", sorted(RINGS))
def test_oracle_matches_brute_force_and_conserves_on_every_query(rings, cap):
    engs, cols, eids = rings[cap]
    wrapped = engs[0].cursor > cap
    assert wrapped == (cap == 1 << 12)
    hot_since = int(cols["recv"][0]) if wrapped else None
    for q in ring_queries():
        n_keys = engs[0].rank_key_space(q["group"])[1]
        cells, info = brute_force_rank(cols, eids, n_keys, **q)
        want = cells, dict(info, hot_since=hot_since)
        answers = [eng.rank_store(**q) for eng in engs]
        assert_same_rank(answers[1], answers[0])
        assert_same_rank(answers[0], want)
        assert_conserved(*answers[0], q["k"])


@pytest.mark.parametrize("cap", sorted(RINGS))
def test_the_rings_leave_no_case_empty(rings, cap):
    eng = rings[cap][0][0]
    rows, groups, counts = RING_FACTS[cap]
    cells, info = eng.rank_store(EV_MEASUREMENT, "assignment", k=None, name_hash=NAMES[0])
    assert (info["rows"], info["groups"], info["nan"], info["ungrouped"]) == (rows, groups, 0, 0)
    if counts is not None:
        assert len(set(cells["count"].tolist())) == counts           # ties abound: the key decides most places
    assert eng.rank_key_space("assignment") == ("asg", 4096)
    for group, n in KEY_SETS.items():
        cells, info = eng.rank_store(EV_MEASUREMENT, group, "max", None, name_hash=NAMES[0])
        assert info["groups"] == n == eng.rank_key_space(group)[1] and cells["key"].tolist() != sorted(cells["key"])
    alerts = rings[cap][1]["etype"] == EV_ALERT
    assert set(rings[cap][1]["level"][alerts].tolist()) == {0, 1, 2}
    assert len(set(rings[cap][1]["name"][alerts].tolist())) == 6
    by_level = [eng.rank_store(EV_ALERT, "customer", k=None, min_level=lv)[1]["rows"] for lv in range(4)]
    assert by_level[0] > by_level[1] > by_level[2] > by_level[3] == 0
    # the subset and the sub-range narrow
    full = eng.rank_store(EV_MEASUREMENT, "area", k=None, name_hash=NAMES[0])[1]["rows"]
    for q in ring_queries():
        if "asg_idx" in q or "start" in q:
            assert 0 < eng.rank_store(**q)[1]["rows"] < full


def _hand_engine(cls=CpuInboundEngine):
    eng = hand_rank_fleet(cls(small_cfg()))
    res = eng.step(*hand_rank_batch(), NOW, presence=False)
    assert res.n_events == 15 and res.n_persisted == eng.cursor == HAND_ROWS < 64      # less than one wave of rows
    return eng


@pytest.mark.parametrize("cls", [CpuInboundEngine, NativeCpuEngine])
def test_hand_batch_nan_signed_zeros_ties_last_by_id_no_customer_and_levels(cls):
    eng = _hand_engine(cls)
    cols, eids = eng.store_rows()
    for q, want, info in hand_expected(hand_eids(cols, eids)):
        got = eng.rank_store(**q)
        assert_same_rank(got, (want, dict(info, hot_since=None)))
        assert_conserved(*got, q["k"])
        n_keys = eng.rank_key_space(q["group"])[1]
        assert_same_rank((brute_force_rank(cols, eids, n_keys, **q)[0], got[1]), (want, got[1]))
    zero = eng.rank_store(EV_MEASUREMENT, "assignment", "min", 2, name_hash=TEMP, ascending=True)[0]
    assert [bits(v) for v in zero["min"]] == [bits(-0.0), bits(0.0)] and zero["key"].tolist() == [2, 3]
    for lv in range(4):                                               # an alert at each level, each of another assignment
        cells, info = eng.rank_store(EV_ALERT, "assignment", k=None, min_level=lv)
        assert cells["key"].tolist() == sorted(a for l, a in HAND_ALERT_ASG.items() if l >= lv)
        assert info["candidates"] == info["rows"] == 4 - lv and (cells["count"] == 1).all()
        assert (cells["last_date"] == NOW).all() and not cells["max"].any()


def test_rank_key_is_the_total_order_and_its_own_inverse():
    vals = np.array([-math.inf, -1e300, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.5, 1e300, math.inf])
    keys = rank_key(vals)
    assert keys.dtype == np.int64 and (np.diff(keys) > 0).all() and (keys[4], keys[5]) == (-1, 0)
    assert rank_key(keys.view(np.float64)).tobytes() == vals.tobytes()
    assert [total_order_key(v) for v in vals] == sorted(total_order_key(v) for v in vals)
    # without the sign fold the negatives would rank in reverse and above the positives' smallest
    assert vals.view(np.int64)[0] > vals.view(np.int64)[1] and (np.argsort(keys) == np.arange(len(vals))).all()


def test_rank_select_classifies_in_order_and_breaks_ties_by_key():
    nan = float("nan")
    #        keys                  dates               ids                     values
    args = ([5, 5, 1, 9, -1, 1, 3], [7, 7, 7, 1, 1, 2, 7], [10, 11, 12, 13, 14, 15, 16], [2.0, 1.0, 2.0, 4.0, 1.0, nan, -0.0])
    cells, rows, n_nan, ungrouped, groups = rank_select(*args, n_keys=9, stat="max")
    assert (rows, n_nan, ungrouped, groups) == (4, 1, 2, 3)            # the NaN counts as one even with a good key
    assert cells["key"].tolist() == [1, 5, 3] and cells["last"].tolist() == [2.0, 1.0, -0.0]
    assert cells[1].tolist() == (5, 2, 1.0, 2.0, 1.0, 7, 11)           # a date tie: the larger id is last
    assert bits(cells["min"][2]) == bits(-0.0)
    asc = rank_select(*args, n_keys=9, stat="count", ascending=True)[0]
    assert asc["key"].tolist() == [1, 3, 5] and rank_select(*args, n_keys=9, stat="count", k=1)[0]["key"].tolist() == [5]
    # no values: every row is grouped or ungrouped, min / max / last stay 0.0
    cells, rows, n_nan, ungrouped, groups = rank_select(args[0], args[1], args[2], None, 10)
    assert (rows, n_nan, ungrouped, groups) == (6, 0, 1, 4) and not cells["min"].any() and not cells["last"].any()
    empty = rank_select([], [], [], [], 4, "last", 3)
    assert empty[0].dtype == RANK_CELL and len(empty[0]) == 0 and empty[1:] == (0, 0, 0, 0)
    assert rank_select([0, 1], [1, 1], [1, 2], None, 0)[1:] == (0, 0, 2, 0)           # an empty key space


def test_check_rank_args_refusals():
    ok = check_rank_args(EV_MEASUREMENT, "customer", "max", 5, NOW - 1, NOW, NAMES[0], None)
    assert ok == (EV_MEASUREMENT, 5, NAMES[0], None)
    assert check_rank_args(EV_ALERT, "area", k=None, min_level=3) == (EV_ALERT, None, None, 3)
    for bad in (dict(event_type=EV_COMMAND_INVOCATION), dict(event_type=255), dict(event_type="Alert"),
                dict(event_type=True), dict(group="device"), dict(group=None), dict(stat="sum"), dict(stat="mean"),
                dict(k=0), dict(k=-1), dict(k=2.5), dict(k="ten"), dict(k=True), dict(stat="max"),
                dict(stat="min", name_hash=NAMES[0], event_type=EV_LOCATION), dict(stat="last", event_type=EV_ALERT),
                dict(min_level=1), dict(event_type=EV_ALERT, min_level=4), dict(event_type=EV_ALERT, min_level=-1),
                dict(event_type=EV_ALERT, min_level=1.5), dict(event_type=EV_LOCATION, min_level=0),
                dict(name_hash=-1), dict(name_hash=1 << 64), dict(name_hash="temp"), dict(start=NOW, end=NOW - 1)):
        with pytest.raises(ValueError):
            check_rank_args(**dict(dict(event_type=EV_MEASUREMENT, group="assignment"), **bad))
    eng = CpuInboundEngine(small_cfg())
    with pytest.raises(ValueError):
        eng.rank_store(EV_MEASUREMENT, "assignment", "max")
    cells, info = eng.rank_store(EV_MEASUREMENT, "customer", k=None)       # an empty ring, and no customer anywhere
    assert cells.dtype == RANK_CELL and len(cells) == 0 and eng.rank_key_space("customer") == ("cust", 0)
    assert info == {"candidates": 0, "rows": 0, "nan": 0, "ungrouped": 0, "groups": 0, "hot_since": None}
    # a key space past the limit is refused; at the limit it is not
    eng.asg_customer[0] = RANK_MAX_KEYS - 1
    assert eng.rank_key_space("customer")[1] == RANK_MAX_KEYS
    eng.asg_customer[0] = RANK_MAX_KEYS
    with pytest.raises(ValueError):
        eng.rank_store(EV_MEASUREMENT, "customer")


def test_an_id_no_assignment_carries_any_more_is_ungrouped():
    eng = _hand_engine()
    before = eng.rank_store(EV_MEASUREMENT, "customer", k=None, name_hash=TEMP)
    assert before[1]["ungrouped"] == 1 and 6 in before[0]["key"].tolist()
    # customers 5 and 6 leave the fleet: the key space shrinks to 5 and their rows fall out of it
    moved = np.flatnonzero(eng.asg_customer >= 5)
    eng.set_assignments(moved, eng.asg_device[moved], customer=0, area=eng.asg_area[moved], asset=eng.asg_asset[moved],
                        active=eng.asg_active[moved])
    cells, info = eng.rank_store(EV_MEASUREMENT, "customer", k=None, name_hash=TEMP)
    assert eng.rank_key_space("customer")[1] == 5 and info["ungrouped"] == 4 and cells["key"].max() == 4
    assert_conserved(cells, info, None)


class _Ev:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_host_rank_equals_the_oracle(rings):
    from sitewhere_amd.models.domain import AlertLevel
    engs, cols, eids = rings[1 << 14]
    eng = engs[0]
    levels = [AlertLevel.Info, AlertLevel.Warning, AlertLevel.Error, AlertLevel.Critical]
    ent = lambda kind, i: None if i < 0 else f"{kind}-{i:04d}"  # noqa: E731  (ids that sort like the keys)
    for et in (EV_MEASUREMENT, EV_ALERT):
        sel = np.flatnonzero(cols["etype"] == et)
        order = sel[np.lexsort((-eids[sel], -cols["date"][sel]))]        # newest first, as event management lists
        evs = [_Ev(device_assignment_id=ent("asg", int(cols["asg"][r])), customer_id=ent("cust", int(cols["cust"][r])),
                   area_id=ent("area", int(cols["area"][r])), asset_id=ent("asset", int(cols["asset"][r])),
                   event_date=int(cols["date"][r]), name=eng.names.get(int(cols["name"][r])),
                   type=eng.names.get(int(cols["name"][r])), value=float(cols["v0"][r]),
                   level=levels[int(cols["level"][r])]) for r in order]
        name = eng.names[NAMES[0]] if et == EV_MEASUREMENT else "zone.exit"
        for group in GROUPS:
            cases = ((("max", 5, False, None), ("min", None, True, None), ("last", 3, False, None), ("count", 4, True, None))
                     if et == EV_MEASUREMENT else (("count", None, False, None), ("count", 4, True, 1)))
            for stat, k, asc, lv in cases:
                # rule alerts are dated by their step: only the measurements have a range to cut
                rng = (NOW - 45000, NOW - 5000) if (et, stat) == (EV_MEASUREMENT, "count") else (None, None)
                h = NAMES[0] if et == EV_MEASUREMENT else [h for h, n in eng.names.items() if n == name][0]
                cells, info = eng.rank_store(et, group, stat, None, None, rng[0], rng[1], h, lv, asc)
                got = host_rank(evs, et, group, stat, k, rng[0], rng[1], name, lv, asc)
                assert got["hotSince"] is None and got["numResults"] == info["rows"] > 0
                assert (got["nan"], got["ungrouped"], got["groups"]) == (info["nan"], info["ungrouped"], info["groups"])
                # the same groups with the same figures; the host breaks ties between groups by listing order, so
                # the two orders are compared on the statistic alone
                by_id = {ent(COLUMN[group], int(c["key"])): c for c in cells}
                assert len(got["results"]) == (len(cells) if k is None else min(k, len(cells)))
                for res in got["results"]:
                    c = by_id[res["id"]]
                    assert (res["count"], res["lastDate"]) == (c["count"], c["last_date"])
                    assert [bits(res[f]) for f in ("min", "max", "last")] == [bits(c[f]) for f in ("min", "max", "last")]
                want = cells[stat][:len(got["results"])].tolist()
                assert [r[stat] for r in got["results"]] == want
    with pytest.raises(ValueError):
        host_rank([], EV_MEASUREMENT, "assignment", "max")


def test_rank_query_and_cell_mirror_the_header():
    text, fields = struct_fields("SwRankQuery")
    assert tuple(n for n, _ in fields) == RANK_QUERY and len(RANK_QUERY) == 20 and RANK_QUERY[:10] == RING_QUERY
    assert {t for _, t in fields} == {"ptr", "int64_t"}                            # every field 8 bytes
    assert "static_assert(sizeof(SwRankQuery) == %d" % (8 * len(RANK_QUERY)) in text
    assert "#define SW_RANK_MAX_KEYS (1 << 22)" in text and RANK_MAX_KEYS == 1 << 22
    cell = struct_fields("SwRankCell")[1]
    assert [n for n, _ in cell] == list(RANK_CELL.names) and RANK_CELL.itemsize == 56 == 8 * len(cell)
    assert [t == "double" for _, t in cell] == [RANK_CELL[n].kind == "f" for n in RANK_CELL.names]
    assert "out[16] = sizeof(SwRankQuery);" in (HEADER.parent.parent / "hip" / "swgpu.hip").read_text()
    import inspect

    from sitewhere_amd.ops import engine_abi
    assert '"rank_query": buf[16]' in inspect.getsource(engine_abi.abi_sizes)


# ------------------------------------------------------------------------------ service API, provider and REST
RANKING = "/sitewhere/api/search/%s/events/ranking"


def test_service_provider_and_rest_on_the_hot_route(site, monkeypatch):  # noqa: F811
    from sitewhere_amd.models import wire
    run, api = site["run"], site["api"]
    tab1, tab2 = site["asg"]
    # tab 1 reports 20.5, 31.0 and then 25.0 degrees, tab 2 -0.0 and a NaN; tab 2 raises two alerts
    msgs = [wire.measurements("galaxytab-001", {"temp": v}, event_date=T0 + 300 + i) for i, v in enumerate((20.5, 31.0, 25.0))]
    msgs += [wire.measurements("galaxytab-002", {"temp": -0.0, "hum": 40.0}, event_date=T0 + 310),
             wire.measurements("galaxytab-002", {"temp": float("nan")}, event_date=T0 + 311),
             wire.alert("galaxytab-002", "overheat", "m", event_date=T0 + 320),
             wire.alert("galaxytab-002", "overheat", "m", event_date=T0 + 321)]
    assert run(lambda: api.process_payloads(msgs))["persisted"] >= 8
    hot = run(lambda: api.event_ranking_hot("Measurement", "Assignment", "max", 10, "temp"))
    assert hot["hotSince"] is None and (hot["numResults"], hot["nan"], hot["ungrouped"], hot["groups"]) == (4, 1, 0, 2)
    assert hot["results"] == [{"id": tab1, "count": 3, "min": 20.5, "max": 31.0, "last": 25.0, "lastDate": T0 + 302},
                              {"id": tab2, "count": 1, "min": -0.0, "max": -0.0, "last": -0.0, "lastDate": T0 + 310}]
    assert math.copysign(1.0, hot["results"][1]["min"]) == -1.0
    low = run(lambda: api.event_ranking_hot("Measurement", "Assignment", "min", 1, "temp", ascending=True))
    assert [r["id"] for r in low["results"]] == [tab2] and low["groups"] == 2
    # the twelve locations of the fixture, by assignment: tab 1 walked ten steps
    loc = run(lambda: api.event_ranking_hot("Location", "Assignment"))
    assert [(r["id"], r["count"]) for r in loc["results"]] == [(tab1, 10), (tab2, 2)] and loc["results"][0]["max"] == 0.0
    alerts = run(lambda: api.event_ranking_hot("Alert", "Assignment", alert_type="overheat", min_level=0))
    assert [(r["id"], r["count"], r["lastDate"]) for r in alerts["results"]] == [(tab2, 2, T0 + 321)]
    # by customer, area and asset the ids are the entities' own
    dm = site["inst"].api("DeviceManagement", "col")
    a1 = run(lambda: dm.get_device_assignment(tab1))
    for group, want in (("Customer", a1.customer_id), ("Area", a1.area_id), ("Asset", a1.asset_id)):
        got = run(lambda g=group: api.event_ranking_hot("Measurement", g, "count", None, "temp"))
        assert got["numResults"] + got["ungrouped"] == 4 and (want is None or want in [r["id"] for r in got["results"]])
    for bad in (("Measurement", "Assignment", "max"), ("Command", "Assignment"), ("Alert", "Device"),
                ("Location", "Area", "count", 0), ("Location", "Area", "count", 5, "temp")):
        with pytest.raises(ValueError):
            run(lambda b=bad: api.event_ranking_hot(*b))
    # the provider takes the hot route (the ring has not wrapped) and REST shows its answer
    calls = []
    from sitewhere_amd.services.gpu_inbound import GpuInboundApi
    real = GpuInboundApi.event_ranking_hot
    monkeypatch.setattr(GpuInboundApi, "event_ranking_hot",
                        lambda self, *a, **k: calls.append(k.get("stat")) or real(self, *a, **k))
    es = site["inst"].api("EventSearch", "col")
    crit = {"eventType": "Measurement", "groupBy": "Assignment", "stat": "max", "measurementId": "temp"}
    assert run(lambda: es.get_event_ranking("events", crit)) == hot and calls == ["max"]
    client, h = site["client"], site["col"]
    r = client.get(RANKING % "events", headers=h, params=crit)
    assert r.status_code == 200, r.text
    assert r.json() == hot and math.copysign(1.0, r.json()["results"][1]["max"]) == -1.0
    r = client.get(RANKING % "events", headers=h, params=dict(crit, stat="min", ascending="true", top=1))
    assert r.json()["results"] == low["results"]
    r = client.get(RANKING % "events", headers=h, params=dict(crit, startDate=T0 + 301, endDate=T0 + 310))
    assert [(x["id"], x["count"]) for x in r.json()["results"]] == [(tab1, 2), (tab2, 1)]
    # refusals are a 400, an unknown provider a 404
    for bad in ({"stat": "sum"}, {"top": 0}, {"groupBy": "Device"}, {"eventType": "Command"}, {"minLevel": 1},
                {"measurementId": None}, {"startDate": T0 + 1, "endDate": T0}, {"alertType": "overheat"}):
        params = {k: v for k, v in dict(crit, **bad).items() if v is not None}
        assert client.get(RANKING % "events", headers=h, params=params).status_code == 400, bad
    assert client.get(RANKING % "nope", headers=h, params=crit).status_code == 404
    assert len(calls) == 4                                       # no refused query reached the engine


def test_host_route_on_the_per_event_tenant(site):  # noqa: F811
    client, h = site["client"], site["default"]
    from sitewhere_amd.services.inbound_processing import InboundProcessingApi
    from sitewhere_amd.services.labels_media_search import SolrSearchProvider
    assert InboundProcessingApi(None).event_ranking_hot("Measurement", "Assignment") is None
    for dev in ("rank-dev-1", "rank-dev-2"):
        r = client.post("/sitewhere/api/devices", headers=h, json={"token": dev, "deviceTypeToken": "raspberrypi"})
        assert r.status_code == 200, r.text
        r = client.post("/sitewhere/api/assignments", headers=h, json={
            "token": dev.replace("dev", "asg"), "deviceToken": dev, "customerToken": "acme", "areaToken": "peachtree"})
        assert r.status_code == 200, r.text
    # a measurement name of its own: the dataset's events do not carry it
    for asg, v, d in (("rank-asg-1", 4.0, T0 + 1), ("rank-asg-1", 9.0, T0 + 2), ("rank-asg-1", 6.0, T0 + 3),
                      ("rank-asg-2", 9.0, T0 + 2), ("rank-asg-2", -0.0, T0 + 5)):
        r = client.post(f"/sitewhere/api/assignments/{asg}/measurements", headers=h,
                        json={"name": "rank.probe", "value": v, "eventDate": d})
        assert r.status_code == 200, r.text
    ids = {a: client.get(f"/sitewhere/api/assignments/{a}", headers=h).json()["id"] for a in ("rank-asg-1", "rank-asg-2")}
    crit = {"eventType": "Measurement", "groupBy": "Assignment", "stat": "last", "measurementId": "rank.probe"}
    solr = SolrSearchProvider("solr", "http://localhost:1").get_event_ranking(crit)
    assert solr["results"] == [] and solr["numResults"] == 0
    with pytest.raises(ValueError):
        SolrSearchProvider("solr", "http://localhost:1").get_event_ranking(dict(crit, stat="sum"))
    got = client.get(RANKING % "events", headers=h, params=crit)
    assert got.status_code == 200, got.text
    body = got.json()
    assert body["hotSince"] is None and set(body) == set(solr)
    assert (body["numResults"], body["nan"], body["ungrouped"], body["groups"]) == (5, 0, 0, 2)
    assert body["results"] == [
        {"id": ids["rank-asg-1"], "count": 3, "min": 4.0, "max": 9.0, "last": 6.0, "lastDate": T0 + 3},
        {"id": ids["rank-asg-2"], "count": 2, "min": -0.0, "max": 9.0, "last": -0.0, "lastDate": T0 + 5}]
    low = client.get(RANKING % "events", headers=h, params=dict(crit, stat="min", ascending="true", top=1)).json()
    assert [x["id"] for x in low["results"]] == [ids["rank-asg-2"]] and low["groups"] == 2
    then = client.get(RANKING % "events", headers=h, params=dict(crit, stat="count", endDate=T0 + 2)).json()
    assert [(x["id"], x["count"]) for x in then["results"]] == [(ids["rank-asg-1"], 2), (ids["rank-asg-2"], 1)]
    by_cust = client.get(RANKING % "events", headers=h, params=dict(crit, groupBy="Customer", stat="max")).json()
    assert by_cust["groups"] == 1 and by_cust["results"][0]["count"] == 5 and by_cust["results"][0]["max"] == 9.0
    assert client.get(RANKING % "events", headers=h, params=dict(crit, stat="sum")).status_code == 400
    assert client.get(RANKING % "events", headers=h, params=dict(crit, top=0)).status_code == 400
    assert client.get(RANKING % "nope", headers=h, params=crit).status_code == 404
    from sitewhere_amd.client import SiteWhereClient
    assert callable(SiteWhereClient.event_ranking)
