"""Measurement series in time buckets (``EngineBase.aggregate_store``) on the CPU engines -- the oracle
of the MI355X kernels (tests/test_gpu_series.py) -- and through the service API and REST."""
import numpy as np
import pytest

from sitewhere_amd.models.columnar import SERIES_CELL, SERIES_QUERY
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.fleet import hash64
from sitewhere_amd.pipeline.native_engine import NativeCpuEngine

from abi_header import struct_fields
from pipeline_scenarios import NOW, setup_fleet, small_cfg
from series_scenarios import CASES, NAMES, assert_cells, brute_force, fill_ring, hand_series_batch


@pytest.mark.parametrize("cls", [CpuInboundEngine, NativeCpuEngine])
def test_oracle_matches_brute_force_on_wrapped_ring(cls):
    eng = fill_ring(cls(small_cfg(store_cap=1 << 12)))
    assert eng.cursor == 12476 > eng.cfg.store_cap
    cols, eids = eng.store_rows()
    for asg, names, lo, hi, bucket, n_rows, n_buckets in CASES:
        cells, info = eng.aggregate_store(asg, names, lo, hi, bucket)
        want, rows, nan, abs_sum = brute_force(cols, eids, asg, names, lo, hi, bucket)
        assert cells.shape == (len(names), n_buckets)
        assert info == {"rows": rows, "nan": nan, "hot_since": int(cols["recv"][0])}
        assert rows == n_rows == int(cells["count"].sum())
        assert_cells(cells, want, abs_sum, exact_sum=True)        # both sums are math.fsum
    # what the cases are there to exercise
    c1 = eng.aggregate_store(*CASES[0][:5])[0]
    assert (c1["count"][3] == 0).all() and int((c1["count"] == 0).sum()) == 39
    c2 = eng.aggregate_store(*CASES[1][:5])[0]
    full = c2["count"] > 0
    assert int(full.sum()) == 475
    # cells whose first (28) or last (32) date is shared by rows of differing values: the event id decides
    asg, names, lo, hi, bucket = CASES[1][:5]
    sel = ((cols["etype"] == 0) & (cols["date"] >= lo) & (cols["date"] <= hi) & np.isin(cols["asg"], asg) &
           np.isin(cols["name"], np.asarray(names, np.uint64)))
    ties = 0
    for i, b in zip(*np.nonzero(full)):
        in_cell = sel & (cols["name"] == np.uint64(names[i])) & ((cols["date"] - lo) // bucket == b)
        for side in ("first_date", "last_date"):
            ties += len(set(cols["v0"][in_cell & (cols["date"] == c2[side][i, b])])) > 1
    assert ties == 60
    assert int((eng.aggregate_store(*CASES[2][:5])[0]["count"] == 0).sum()) == 75
    assert eng.aggregate_store(*CASES[3][:5])[0]["count"].tolist() == [[315]]
    assert eng.aggregate_store(*CASES[4][:5])[0].size == 32008


def test_series_cell_mirrors_header():
    text, fields = struct_fields("SwSeriesCell")
    kinds = {"int64_t": np.dtype("<i8"), "double": np.dtype("<f8")}
    assert [(n, kinds[t]) for n, t in fields] == [(n, SERIES_CELL.fields[n][0]) for n in SERIES_CELL.names]
    assert [SERIES_CELL.fields[n][1] for n in SERIES_CELL.names] == list(range(0, 80, 8))
    assert SERIES_CELL.itemsize == 80 and "static_assert(sizeof(SwSeriesCell) == 80" in text
    # the query block the host builds as int64 words: same names, same order, every field 8 bytes
    _, qf = struct_fields("SwSeriesQuery")
    assert tuple(n for n, _ in qf) == SERIES_QUERY
    assert {t for _, t in qf} == {"ptr", "int64_t"}


@pytest.mark.parametrize("cls", [CpuInboundEngine, NativeCpuEngine])
def test_argument_errors(cls):
    eng = cls(small_cfg())
    ok = ([1], NAMES[:2], NOW - 1000, NOW, 10)
    assert eng.aggregate_store(*ok)[0].shape == (2, 101)           # an empty ring: zeroed cells
    assert not eng.aggregate_store(*ok)[0].tobytes().strip(b"\0")
    for bad in (([1], NAMES[:2], NOW - 1000, NOW, 0), ([1], NAMES[:2], NOW, NOW - 1, 10), ([1], [], NOW - 1000, NOW, 10),
                ([1], list(range(1, 66)), NOW - 1000, NOW, 10), ([1], [NAMES[0], NAMES[1], NAMES[0]], NOW - 1000, NOW, 10),
                ([1], NAMES[:2], NOW - 32768, NOW, 1)):
        with pytest.raises(ValueError):
            eng.aggregate_store(*bad)
    assert eng.aggregate_store([1], NAMES[:2], NOW - 32767, NOW, 1)[0].size == 65536     # the limit itself


@pytest.mark.parametrize("cls", [CpuInboundEngine, NativeCpuEngine])
def test_hand_values(cls):
    eng = cls(small_cfg())
    setup_fleet(eng, n_dev=1000)
    r = eng.step(*hand_series_batch(), NOW, presence=False)
    assert r.n_persisted == 7
    temp, hum = hash64("temp"), hash64("hum")
    cells, info = eng.aggregate_store([1, 2], [temp, hum], NOW - 100, NOW - 71, 10)
    assert info == {"rows": 6, "nan": 1, "hot_since": None}
    assert cells.shape == (2, 3) and cells["count"].tolist() == [[0, 2, 3], [1, 0, 0]]     # the NaN is in no cell
    cols, eids = eng.store_rows()
    rows = [(int(d), int(e), float(v)) for d, e, v, h in zip(cols["date"], eids, cols["v0"], cols["name"])
            if int(h) == temp and v == v]
    zeros = cells[0, 1]                  # -0.0 (device 1) and 0.0 (device 2) at one date: by event id
    assert zeros["min"] == zeros["max"] == zeros["sum"] == 0.0
    ids = sorted(e for d, e, _ in rows if d == NOW - 90)
    assert [int(zeros["first_id"]), int(zeros["last_id"])] == ids and ids[0] != ids[1]
    assert np.signbit(zeros["first"]) != np.signbit(zeros["last"])
    big = cells[0, 2]                    # 1e300, -1e300, 1.0 at one date: the sum is 1.0 exactly (fsum)
    assert (big["sum"], big["min"], big["max"]) == (1.0, -1e300, 1e300)
    assert int(big["first_date"]) == int(big["last_date"]) == NOW - 80
    by_id = sorted((e, v) for d, e, v in rows if d == NOW - 80)
    assert (big["first"], int(big["first_id"])) == (by_id[0][1], by_id[0][0])
    assert (big["last"], int(big["last_id"])) == (by_id[-1][1], by_id[-1][0])
    assert cells[1, 0]["first"] == cells[1, 0]["sum"] == 40.0     # hum rode the NaN payload and persists


# ------------------------------------------------------------------------------ service API and REST
T0 = 1_700_000_000_000


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
        dev = run(lambda: dm.get_device_by_token("galaxytab-001"))
        ib = inst.tenant_engine("inbound-processing", "col")
        end = time.time() + 10
        while not engine_knows(ib, dev) and time.time() < end:
            time.sleep(0.02)
        api = inst.api("InboundProcessing", "col")
        msgs = [wire.measurements("galaxytab-001", {"temp": 20.0 + i}, event_date=T0 + i) for i in range(50)]
        msgs += [wire.measurements("galaxytab-001", {"hum": 40.0 + i}, event_date=T0 + 25 + i) for i in range(3)]
        assert run(lambda: api.process_payloads(msgs))["persisted"] == 53
        client = TestClient(inst.rest_app)
        r = client.get("/sitewhere/authapi/jwt",
                       headers={"Authorization": "Basic " + base64.b64encode(b"admin:password").decode()})
        h = {"Authorization": f"Bearer {r.headers['X-Sitewhere-JWT']}"}
        token = run(lambda: dm.get_device_assignment(dev.device_assignment_id)).token
        yield {"run": run, "api": api, "client": client, "asg_id": dev.device_assignment_id, "asg_token": token,
               "col": dict(h, **{"X-SiteWhere-Tenant-Id": "col", "X-SiteWhere-Tenant-Auth": "col-auth"}),
               "default": dict(h, **{"X-SiteWhere-Tenant-Id": "default",
                                     "X-SiteWhere-Tenant-Auth": "sitewhere1234567890"})}
    finally:
        inst.stop()


SERIES = "/sitewhere/api/assignments/%s/measurements/series"
ENTRY_KEYS = {"bucketStart", "count", "min", "max", "mean", "first", "last", "firstDate", "lastDate"}


def test_service_and_rest_return_the_same_buckets(site):
    hot = site["run"](lambda: site["api"].measurement_series_hot("Assignment", [site["asg_id"]], None, T0, T0 + 49, 10))
    assert hot["hotSince"] is None and hot["rows"] == 53
    assert [s["measurementId"] for s in hot["series"]] == ["hum", "temp"]
    hum, temp = (s["entries"] for s in hot["series"])
    assert [e["bucketStart"] for e in temp] == [T0 + 10 * k for k in range(5)] and set(temp[0]) == ENTRY_KEYS
    # two buckets by hand: temp's rows i = 10 .. 19 are 30.0 .. 39.0; hum's three rows at T0 + 25 .. 27
    assert temp[1] == {"bucketStart": T0 + 10, "count": 10, "min": 30.0, "max": 39.0, "mean": 34.5, "first": 30.0,
                       "last": 39.0, "firstDate": T0 + 10, "lastDate": T0 + 19}
    assert hum == [{"bucketStart": T0 + 20, "count": 3, "min": 40.0, "max": 42.0, "mean": 41.0, "first": 40.0,
                    "last": 42.0, "firstDate": T0 + 25, "lastDate": T0 + 27}]
    r = site["client"].get(SERIES % site["asg_token"], headers=site["col"],
                           params={"bucketMs": 10, "startDate": T0, "endDate": T0 + 49})
    assert r.status_code == 200, r.text
    assert r.json() == hot["series"]
    one = site["client"].get(SERIES % site["asg_token"], headers=site["col"],
                             params={"bucketMs": 10, "startDate": T0 + 20, "endDate": T0 + 49, "measurementIds": "hum"})
    assert one.json() == [{"measurementId": "hum", "entries": hum}]


def test_rest_host_route_on_per_event_tenant(site):
    client, h = site["client"], site["default"]
    from sitewhere_amd.services.inbound_processing import InboundProcessingApi
    assert InboundProcessingApi(None).measurement_series_hot("Assignment", [], None, 0, 1, 1) is None
    r = client.post("/sitewhere/api/devices", headers=h, json={"token": "series-dev", "deviceTypeToken": "raspberrypi"})
    assert r.status_code == 200, r.text
    r = client.post("/sitewhere/api/assignments", headers=h, json={"token": "series-asg", "deviceToken": "series-dev",
                                                                  "customerToken": "acme", "areaToken": "peachtree"})
    assert r.status_code == 200, r.text
    for d, v in ((T0 + 1, 1.0), (T0 + 4, 3.0), (T0 + 12, 5.0)):
        r = client.post("/sitewhere/api/assignments/series-asg/measurements", headers=h,
                        json={"name": "temp", "value": v, "eventDate": d})
        assert r.status_code == 200, r.text
    args = {"bucketMs": 10, "startDate": T0, "endDate": T0 + 19}
    got = client.get(SERIES % "series-asg", headers=h, params=args)
    assert got.status_code == 200, got.text
    assert got.json() == [{"measurementId": "temp", "entries": [
        {"bucketStart": T0, "count": 2, "min": 1.0, "max": 3.0, "mean": 2.0, "first": 1.0, "last": 3.0,
         "firstDate": T0 + 1, "lastDate": T0 + 4},
        {"bucketStart": T0 + 10, "count": 1, "min": 5.0, "max": 5.0, "mean": 5.0, "first": 5.0, "last": 5.0,
         "firstDate": T0 + 12, "lastDate": T0 + 12}]}]
    assert client.get(SERIES % "series-asg", headers=h, params={"bucketMs": 10, "endDate": T0 + 19}).status_code == 400
    assert client.get(SERIES % "series-asg", headers=h, params={"bucketMs": 10, "startDate": T0}).status_code == 400
    assert client.get(SERIES % "series-asg", headers=h, params=dict(args, bucketMs=0)).status_code == 400
    assert client.get(SERIES % "series-asg", headers=h, params={"bucketMs": 1, "startDate": T0, "endDate": T0 + 40000,
                                                                "measurementIds": "a,b"}).status_code == 400
    raw = client.get(SERIES % "series-asg", headers=h, params={"startDate": T0, "endDate": T0 + 19}).json()
    assert raw == [{"measurementId": "temp", "entries": [{"value": 1.0, "measurementDate": T0 + 1},
                                                         {"value": 3.0, "measurementDate": T0 + 4},
                                                         {"value": 5.0, "measurementDate": T0 + 12}]}]
