"""Measurement (threshold) rules inside the engine step: the Python oracle, the native C++ engine,
checkpoints, the inbound tenant and a two-rank run.  (The MI355X engine: test_gpu_measurement_rules.py.)

A measurement test fires on a persisted measurement row whose name matches and whose value lies
strictly outside [min, max]; its alert is generated, persisted and indexed exactly like a zone
alert, in row-major, test-ascending order (zone tests first in the test-index space).
"""
import copy
import os
import time

import numpy as np
import pytest

from sitewhere_amd.models.columnar import EV_ALERT, EV_LOCATION
from sitewhere_amd.pipeline.config import EngineConfig
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.engine_base import MeasurementTest, Zone, ZoneTest
from sitewhere_amd.pipeline.fleet import fingerprints, gen_tokens, hash64
from sitewhere_amd.pipeline.native_engine import NativeCpuEngine

from measurement_scenarios import (BOUNDARY_ALERTS, FLEET_RULES, HAND_RULES, alerts_of, boundary_batch, count_hits,
                                   many_rules, rows)
from pipeline_scenarios import NOW, SQUARE, fleet_batch, setup_fleet, small_cfg

ENGINES = [("oracle", lambda **kw: CpuInboundEngine(small_cfg(**kw))),
           ("native1", lambda **kw: NativeCpuEngine(small_cfg(**kw), threads=1)),
           ("native3", lambda **kw: NativeCpuEngine(small_cfg(**kw), threads=3))]


def same_result(ra, rb):
    assert ra.n_events == rb.n_events and ra.n_persisted == rb.n_persisted
    assert ra.first_seq == rb.first_seq
    assert ra.out.tobytes() == rb.out.tobytes()
    assert ra.prec.tobytes() == rb.prec.tobytes()
    assert ra.rejects.tobytes() == rb.rejects.tobytes()


def same_engine(a, b):
    assert a.stats_dict() == b.stats_dict()
    assert a.cursor == b.cursor
    ca, ea = a.store_rows()
    cb, eb = b.store_rows()
    assert np.array_equal(ea, eb)
    for k in ca:
        assert np.array_equal(ca[k], cb[k], equal_nan=ca[k].dtype.kind == "f"), k


# ------------------------------------------------------------------ semantics, written out by hand
@pytest.mark.parametrize("kind,make", ENGINES, ids=[k for k, _ in ENGINES])
def test_boundary_batch_fires_exactly_the_expected_alerts(kind, make):
    e = make()
    setup_fleet(e, n_dev=20)
    e.set_measurement_rules(HAND_RULES)
    raw, offs = boundary_batch()
    res = e.step(raw, offs, NOW, presence=False)
    n_gen = len(BOUNDARY_ALERTS)
    assert res.n_persisted == 10 + n_gen                    # 9 messages, one with two measurements
    assert e.stats_dict()["rule_alerts"] == n_gen
    assert alerts_of(e, res, n_gen) == [(a, t, lv) for a, t, lv, _ in BOUNDARY_ALERTS]
    gen = res.prec[len(res.prec) - n_gen:]
    assert gen["aux_off"].tolist() == [k for *_, k in BOUNDARY_ALERTS]       # the combined test index
    assert (gen["etype"] == EV_ALERT).all() and (gen["event_date"] == NOW).all()
    assert gen["name_hash"].tolist() == [hash64(t) for _, t, _, _ in BOUNDARY_ALERTS]
    for k in ("v0", "v1", "v2", "alt_hash", "fp_lo", "fp_hi", "aux_len"):
        assert not gen[k].any(), k
    # the alerts are persisted rows like any other: in the event store, after the device rows
    cols, _ = e.store_rows()
    assert cols["etype"][-n_gen:].tolist() == [EV_ALERT] * n_gen
    assert cols["asg"][-n_gen:].tolist() == [a for a, *_ in BOUNDARY_ALERTS]


def test_defaults_of_a_measurement_test():
    t = MeasurementTest("temp", max=20.0)
    assert t.alert_type == "temp.threshold" and t.alert_level == 1
    assert t.alert_message == "temp outside [None, 20.0]"
    e = CpuInboundEngine(small_cfg())
    setup_fleet(e, n_dev=10)
    e.set_measurement_rules([t, MeasurementTest("hum", min=1.0, max=2.0, alert_type="h", alert_level=3)])
    assert e.names[hash64("temp.threshold")] == "temp.threshold" and e.names[hash64("h")] == "h"
    assert [type(x).__name__ for x in e.rule_tests] == ["ZoneTest", "ZoneTest", "MeasurementTest", "MeasurementTest"]
    tab, levels, hashes = e.measurement_arrays()
    assert tab.dtype.itemsize == 24
    assert tab["name_hash"].tolist() == [hash64("temp"), hash64("hum")]
    assert tab["lo"].tolist() == [-np.inf, 1.0] and tab["hi"].tolist() == [20.0, 2.0]
    assert levels.tolist() == [1, 3] and hashes.tolist() == [hash64("temp.threshold"), hash64("h")]


# ------------------------------------------------------------------ oracle vs native
@pytest.mark.parametrize("threads", [1, 4])
def test_fleet_parity_oracle_native(threads):
    o = CpuInboundEngine(small_cfg())
    n = NativeCpuEngine(small_cfg(), threads=threads)
    for e in (o, n):
        setup_fleet(e)
        e.set_measurement_rules(FLEET_RULES)
    zone_hits = mx_hits = 0
    for k in range(4):
        raw, offs = fleet_batch(3000, seed=100 + k)
        ro = o.step(raw, offs, NOW + k * 1000, presence=False)
        rn = n.step(raw, offs, NOW + k * 1000, presence=False)
        same_result(ro, rn)
        n_gen = int(((ro.prec["fp_lo"] == 0) & (ro.prec["fp_hi"] == 0)).sum())     # generated: no token
        dev = ro.prec[:len(ro.prec) - n_gen]
        hits = count_hits(dev, FLEET_RULES)
        assert 100 < hits < 300                             # ~180 per step
        mx_hits += hits
        zone_hits += int((dev["etype"] == EV_LOCATION).sum())     # inside / outside of one zone: one each
        assert n_gen == int((dev["etype"] == EV_LOCATION).sum()) + hits
    same_engine(o, n)
    assert o.stats_dict()["rule_alerts"] == zone_hits + mx_hits


def test_gen_cap_cuts_both_engines_at_the_same_alert():
    o = CpuInboundEngine(small_cfg(gen_cap=64))
    n = NativeCpuEngine(small_cfg(gen_cap=64), threads=4)
    for e in (o, n):
        setup_fleet(e)
        e.set_measurement_rules(many_rules(20))
    raw, offs = fleet_batch(3000, seed=100)
    same_result(o.step(raw, offs, NOW, presence=False), n.step(raw, offs, NOW, presence=False))
    same_engine(o, n)
    assert o.stats_dict()["rule_alerts"] == 64


# ------------------------------------------------------------------ validation
def test_validation():
    with pytest.raises(ValueError):
        MeasurementTest("t")                                # neither bound
    with pytest.raises(ValueError):
        MeasurementTest("t", min=float("nan"))
    with pytest.raises(ValueError):
        MeasurementTest("t", max=float("nan"))
    with pytest.raises(ValueError):
        MeasurementTest("t", min=2.0, max=1.0)
    MeasurementTest("t", min=1.0, max=1.0)                  # a point interval is fine
    e = CpuInboundEngine(small_cfg())
    setup_fleet(e, n_dev=10)                                # 2 zone tests
    with pytest.raises(ValueError):                         # a bound edited into a NaN after construction
        bad = MeasurementTest("t", min=1.0)
        bad.min = float("nan")
        e.set_measurement_rules([bad])
    e.set_measurement_rules(many_rules(62))                 # 2 + 62 = 64: every bit of the mask
    assert len(e.rule_tests) == 64
    with pytest.raises(ValueError):
        e.set_measurement_rules(many_rules(63))
    assert len(e.mtests) == 62                              # a refused list changes nothing
    with pytest.raises(ValueError):                         # the sum is checked from the zone side too
        e.set_zone_rules([Zone("z1", SQUARE)], [ZoneTest("z1", "inside", f"z{i}") for i in range(3)])
    assert len(e.tests) == 2


# ------------------------------------------------------------------ checkpoint
@pytest.mark.parametrize("kind,make", ENGINES[:2], ids=["oracle", "native"])
def test_checkpoint_round_trip_keeps_the_rules(kind, make, tmp_path):
    live, stopped = make(), make()
    for e in (live, stopped):
        setup_fleet(e)
        e.set_measurement_rules(FLEET_RULES)
        e.step(*fleet_batch(1500, seed=100), NOW, presence=False)
    path = str(tmp_path / "shard.safetensors")
    stopped.save_checkpoint(path, include_store=True)
    back = make()
    setup_fleet(back)
    back.load_checkpoint(path)
    assert back.mtests == FLEET_RULES and len(back.tests) == 2
    raw, offs = fleet_batch(1500, seed=101)
    rl, rb = live.step(raw, offs, NOW + 1000, presence=False), back.step(raw, offs, NOW + 1000, presence=False)
    same_result(rl, rb)
    same_engine(live, back)
    assert count_hits(rb.prec, FLEET_RULES) > 0             # the restored rules fired in that step


def test_checkpoint_without_the_key_restores_no_rules(tmp_path):
    import json
    from safetensors import safe_open
    from safetensors.numpy import load_file, save_file
    e = CpuInboundEngine(small_cfg())
    setup_fleet(e, n_dev=50)
    e.set_measurement_rules(FLEET_RULES)
    path = str(tmp_path / "old.safetensors")
    e.save_checkpoint(path)
    with safe_open(path, "np") as f:
        meta = json.loads(f.metadata()["meta"])
    assert len(meta.pop("mtests")) == 3                     # rewrite it as an older writer would have
    save_file(load_file(path), path, metadata={"meta": json.dumps(meta)})
    back = CpuInboundEngine(small_cfg())
    back.set_measurement_rules(FLEET_RULES)
    back.load_checkpoint(path)
    assert back.mtests == [] and len(back.tests) == 2


# ------------------------------------------------------------------ replacement between steps
@pytest.mark.parametrize("kind,make", ENGINES[:2], ids=["oracle", "native"])
def test_replaced_then_cleared_rules(kind, make):
    plain, e = make(), make()
    setup_fleet(plain)
    setup_fleet(e)
    e.set_measurement_rules(FLEET_RULES)
    batches = [fleet_batch(1500, seed=100 + k) for k in range(3)]
    r0 = e.step(*batches[0], NOW, presence=False)
    p0 = plain.step(*batches[0], NOW, presence=False)
    assert r0.n_persisted - p0.n_persisted == count_hits(r0.prec, FLEET_RULES) > 0
    e.set_measurement_rules(FLEET_RULES[:1])
    r1 = e.step(*batches[1], NOW + 1000, presence=False)
    p1 = plain.step(*batches[1], NOW + 1000, presence=False)
    assert r1.n_persisted - p1.n_persisted == count_hits(r1.prec, FLEET_RULES[:1]) > 0
    e.set_measurement_rules([])
    r2 = e.step(*batches[2], NOW + 2000, presence=False)
    p2 = plain.step(*batches[2], NOW + 2000, presence=False)
    # the cleared step is the step of an engine that never had rules (its rows sit further along
    # the store: the earlier alerts took sequence numbers)
    # (names compared by their hashes: the alert types took interned ids on the engine that had rules)
    assert rows(e, r2) == rows(plain, p2) and r2.prec.tobytes() == p2.prec.tobytes()
    assert r2.rejects.tobytes() == p2.rejects.tobytes()
    assert r2.first_seq - p2.first_seq == e.stats_dict()["rule_alerts"] - plain.stats_dict()["rule_alerts"] > 0


# ------------------------------------------------------------------ inbound tenant
def wait_until(cond, timeout=20.0, step=0.02):
    end = time.time() + timeout
    while time.time() < end:
        if cond():
            return True
        time.sleep(step)
    return bool(cond())


MX_CONF = [{"measurement": "engine.temp", "max": 90.0, "alertType": "engine.overheat", "alertLevel": 3,
            "alertMessage": "engine too hot"},
           {"measurement": "fuel.level", "min": 10.0}]


def test_tenant_raises_system_alerts_from_configured_measurement_tests():
    import struct
    from conftest import engine_knows
    from sitewhere_amd.assembly import SiteWhereInstance
    from sitewhere_amd.models import wire
    from sitewhere_amd.models.domain import AlertLevel, AlertSource
    from sitewhere_amd.services.event_sources import RAW_PAYLOADS
    from sitewhere_amd.services.tenant_management import TENANT_TEMPLATES

    tpl = copy.deepcopy(TENANT_TEMPLATES["gpu"])
    tpl["services"]["inbound-processing"].update(device="cpu", measurementTests=MX_CONF)
    TENANT_TEMPLATES["mx-rules"] = tpl
    inst = SiteWhereInstance().start()
    try:
        inst.wait_for_tenant("default", 60)
        tm = inst.api("TenantManagement")
        inst.instance.system_user.run(lambda: tm.create_tenant({"token": "mxr", "name": "mxr",
                                                                "configurationTemplateId": "mx-rules",
                                                                "datasetTemplateId": "construction"}))
        inst.wait_for_tenant("mxr", 60)
        ib = inst.tenant_engine("inbound-processing", "mxr")
        run = lambda f: inst.instance.system_user.run(f, "mxr")  # noqa: E731
        dev = run(lambda: inst.api("DeviceManagement", "mxr").get_device_by_token("galaxytab-001"))
        assert wait_until(lambda: engine_knows(ib, dev))
        assert ib.engine_kind == "cpu"
        assert [(t.measurement, t.min, t.max) for t in ib.engine.mtests] == [("engine.temp", None, 90.0),
                                                                             ("fuel.level", 10.0, None)]
        msgs = [wire.measurements("galaxytab-001", {"engine.temp": 95.5, "fuel.level": 50.0}, event_date=NOW,
                                  alternate_id="mx-1"),
                wire.measurements("galaxytab-001", {"engine.temp": 90.0, "fuel.level": 9.5}, event_date=NOW + 1,
                                  alternate_id="mx-2")]
        topic = inst.instance.naming.tenant_prefix("mxr") + RAW_PAYLOADS
        inst.instance.bus.append(topic, 0, [(None, struct.pack(f"<I{len(msgs)}I", len(msgs), *map(len, msgs))
                                             + b"".join(msgs))], ts=NOW + 5)
        em = inst.api("DeviceEventManagement", "mxr")
        alerts = lambda: run(lambda: em.list_alerts_for_index(  # noqa: E731
            "Assignment", [dev.device_assignment_id], {"pageSize": 0})).results
        assert wait_until(lambda: len(alerts()) == 2), alerts()
        got = {a.type: a for a in alerts()}
        hot, low = got["engine.overheat"], got["fuel.level.threshold"]
        assert hot.source == AlertSource.System and low.source == AlertSource.System
        assert hot.message == "engine too hot" and low.message == "fuel.level outside [10.0, None]"
        assert AlertLevel(hot.level) == AlertLevel.Critical and AlertLevel(low.level) == AlertLevel.Warning
        assert ib.engine.stats_dict()["rule_alerts"] == 2
    finally:
        inst.stop()
        del TENANT_TEMPLATES["mx-rules"]


def test_configuration_model_knows_measurement_tests():
    from sitewhere_amd.configuration import model_for
    m = model_for("inbound-processing")
    assert m.validate({"engine": "gpu", "measurementTests": MX_CONF}) == []
    errs = m.validate({"engine": "gpu", "measurementTests": [{"measurement": "t", "max": 1.0, "hysteresis": 2}]})
    assert any("unknown attribute 'hysteresis'" in str(x) for x in errs), errs
    errs = m.validate({"engine": "gpu", "measurementTests": [{"max": 1.0}]})
    assert errs, "a measurement test without its measurement must not validate"


# ------------------------------------------------------------------ two ranks over gloo
N_DEV = 900
RANK_RULE = [MeasurementTest("mx.metric2", min=200.0, max=800.0)]


def _shard(e, world, rank):
    heap, offs = gen_tokens("dev-", 0, N_DEV)
    lo, hi = fingerprints(heap, offs)
    dev = e.register_devices(lo, hi)
    e.set_assignments(dev, dev, customer=dev % 7, area=dev % 5, asset=dev % 3)
    e.set_measurement_rules(RANK_RULE)
    return ((hi >> np.uint64(32)) % np.uint64(world)) == rank


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    e = CpuInboundEngine(EngineConfig.small(world=world, rank=rank))
    mine = _shard(e, world, rank)
    raw, offs = fleet_batch(1000, seed=500 + rank, n_dev=N_DEV)
    r = e.step(raw, offs, NOW, presence=False)
    al = r.out[r.out["etype"] == EV_ALERT]
    typ = e.intern.get(hash64("mx.metric2.threshold"), -2)
    gen = al[al["name_id"] == typ]                            # device alerts carry other types
    q.put((rank, e.stats_dict()["rule_alerts"], len(gen), bool(mine[gen["assignment"]].all()),
           count_hits(r.prec, RANK_RULE), bool(mine[r.out["assignment"]].all())))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_two_ranks_alert_on_the_owner_only():
    import multiprocessing as mp
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    single = CpuInboundEngine(EngineConfig.small())
    _shard(single, 1, 0)
    for r in range(2):
        single.step(*fleet_batch(1000, seed=500 + r, n_dev=N_DEV), NOW, presence=False)
    total = single.stats_dict()["rule_alerts"]
    assert total > 50
    for rank, n_rule, n_rows, on_owner, hits, rows_owned in outs:
        assert n_rule == n_rows == hits > 0, outs             # a rank alerts on the rows it persisted...
        assert on_owner and rows_owned, outs                  # ...which are its own devices' rows
    assert sum(o[1] for o in outs) == total
