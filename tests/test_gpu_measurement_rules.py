"""Measurement (threshold) rules on the MI355X engine (k_mx_mask + k_zone_emit) against the host
engines: the same alerts in the same order (row-major, test index ascending, zone tests first), the
same stats, store rows and durable block.  Presence is off, so every generated row is a rule alert
and the outbound rows are compared in order, names by their hashes (each engine interns its own ids).
"""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X GPU")]

if gpu_available():
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

from sitewhere_amd.models.columnar import EV_ALERT
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.fleet import fingerprints, gen_tokens
from sitewhere_amd.pipeline.native_engine import NativeCpuEngine

from measurement_scenarios import (BOUNDARY_ALERTS, FLEET_RULES, HAND_RULES, alerts_of, boundary_batch, count_hits,
                                   many_rules, rows)
from pipeline_scenarios import NOW, fleet_batch, setup_fleet, small_cfg
from state_scenarios import full_state, state_diff

EMPTY = (np.zeros(64, np.uint8), np.zeros(1, np.uint32))


def pair(rules, host=CpuInboundEngine, zones=True, **kw):
    g = GpuInboundEngine(small_cfg(**kw))
    c = host(small_cfg(**kw))
    for e in (g, c):
        if zones:
            setup_fleet(e, n_dev=1000)
        else:
            register_only(e)
        e.set_measurement_rules(rules)
    return g, c


def register_only(e, n_dev=1000):
    """setup_fleet without its zone rules."""
    heap, offs = gen_tokens("dev-", 0, n_dev)
    lo, hi = fingerprints(heap, offs)
    e.register_devices(lo, hi)
    dev = np.arange(n_dev, dtype=np.int32)
    e.set_assignments(dev, dev, customer=dev % 7, area=dev % 5, asset=dev % 3, active=(dev % 10 != 9).astype(np.uint8))


def same_step(g, c, rg, rc):
    assert rg.n_events == rc.n_events and rg.n_persisted == rc.n_persisted
    assert rg.first_seq == rc.first_seq
    a, b = rows(g, rg), rows(c, rc)
    assert len(a) == len(b)
    assert a == b, next((i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y)


def same_store(g, c):
    cg, eg = g.store_rows()
    cc, ec = c.store_rows()
    assert np.array_equal(eg, ec)
    for k in ("etype", "level", "dev", "asg", "cust", "area", "asset", "date", "recv", "name"):
        assert np.array_equal(cg[k], cc[k]), k
    assert np.array_equal(cg["v0"].view(np.uint64), cc["v0"].view(np.uint64))


def test_boundary_batch():
    g, c = pair(HAND_RULES)
    raw, offs = boundary_batch()
    rg = g.step(raw, offs, NOW, presence=False)
    rc = c.step(raw, offs, NOW, presence=False)
    n_gen = len(BOUNDARY_ALERTS)
    assert rg.n_persisted == 10 + n_gen
    assert alerts_of(g, rg, n_gen) == [(a, t, lv) for a, t, lv, _ in BOUNDARY_ALERTS]
    same_step(g, c, rg, rc)
    assert g.stats_dict() == c.stats_dict() and g.stats_dict()["rule_alerts"] == n_gen
    cols, _ = g.store_rows()
    assert (cols["aux"][-n_gen:] & np.uint64(0xFFFFFFFF)).tolist() == [k for *_, k in BOUNDARY_ALERTS]
    same_store(g, c)


def test_fleet_several_tiles_with_zone_tests():
    g, c = pair(FLEET_RULES)
    for k in range(4):
        raw, offs = fleet_batch(3000, seed=100 + k)
        rg = g.step(raw, offs, NOW + k * 1000, presence=False)
        rc = c.step(raw, offs, NOW + k * 1000, presence=False)
        same_step(g, c, rg, rc)
        n_dev_rows = int((rc.prec["fp_lo"] != 0).sum())
        assert n_dev_rows > 4 * 1024 and n_dev_rows % 1024          # 5 tiles, the last one partial
        assert count_hits(rc.prec, FLEET_RULES) > 100
    assert g.stats_dict() == c.stats_dict()
    same_store(g, c)
    sg, sc = full_state(g), full_state(c)
    assert sg == sc, state_diff(sg, sc)


def test_measurement_tests_without_zone_tests():
    """The launch branch without k_zone_mask: k_mx_mask writes zmask and ztile itself, the tiles past
    the step's rows included (a large step, then none, a few rows, a large step again)."""
    g, c = pair(FLEET_RULES + HAND_RULES, zones=False)
    steps = [fleet_batch(3000, seed=100), EMPTY, boundary_batch(), fleet_batch(3000, seed=101), EMPTY]
    for k, (raw, offs) in enumerate(steps):
        rg = g.step(raw, offs, NOW + k * 1000, presence=False)
        rc = c.step(raw, offs, NOW + k * 1000, presence=False)
        same_step(g, c, rg, rc)
        assert g.stats_dict() == c.stats_dict(), k
        if len(offs) == 1:
            assert rg.n_persisted == 0
    assert alerts_of(c, c.step(*boundary_batch(), NOW + 9000, presence=False), 7) == \
        alerts_of(g, g.step(*boundary_batch(), NOW + 9000, presence=False), 7) == \
        [(a, t, lv) for a, t, lv, _ in BOUNDARY_ALERTS[1:]]
    same_store(g, c)


def test_sixty_four_tests_use_every_bit():
    rules = many_rules(62)
    g, c = pair(rules, host=NativeCpuEngine, gen_cap=16384)      # ~9,000 alerts per step, none cut
    for k in range(2):
        raw, offs = fleet_batch(3000, seed=100 + k)
        rg = g.step(raw, offs, NOW + k * 1000, presence=False)
        rc = c.step(raw, offs, NOW + k * 1000, presence=False)
        same_step(g, c, rg, rc)
        gen = rc.prec[rc.prec["fp_lo"] == 0]
        assert int(gen["aux_off"].max()) == 63 and int(gen["aux_off"].min()) == 0
        # some row fires several tests: more measurement alerts than measurement rows
        assert int((gen["aux_off"] >= 2).sum()) == count_hits(rc.prec, rules) > int((rc.prec["etype"] == 0).sum())
    assert g.stats_dict() == c.stats_dict()
    same_store(g, c)


def test_gen_cap_keeps_the_first_alerts_in_emission_order():
    g, c = pair(FLEET_RULES, gen_cap=256)
    full = CpuInboundEngine(small_cfg())
    setup_fleet(full, n_dev=1000)
    full.set_measurement_rules(FLEET_RULES)
    raw, offs = fleet_batch(3000, seed=100)
    rg = g.step(raw, offs, NOW, presence=False)
    rc = c.step(raw, offs, NOW, presence=False)
    rf = full.step(raw, offs, NOW, presence=False)
    same_step(g, c, rg, rc)
    assert g.stats_dict() == c.stats_dict() and g.stats_dict()["rule_alerts"] == 256
    assert full.stats_dict()["rule_alerts"] > 256                    # the rules fire more than the cap
    n_dev_rows = rg.n_persisted - 256
    assert rows(g, rg)[n_dev_rows:] == rows(full, rf)[n_dev_rows:n_dev_rows + 256]
    # the step after a clamped one starts clean
    raw, offs = fleet_batch(3000, seed=101)
    same_step(g, c, g.step(raw, offs, NOW + 1000, presence=False), c.step(raw, offs, NOW + 1000, presence=False))
    assert g.stats_dict() == c.stats_dict()


def test_durable_block_and_trailer_match_the_host_builders():
    from sitewhere_amd.persistence import segments as sg
    from tests.test_block_index import check_trailer
    from tests.test_gpu_index import _strip_trailer
    g, c = pair(FLEET_RULES)
    raw, offs = fleet_batch(3000, seed=100)
    rg = g.step(raw, offs, NOW, presence=False)
    rc = c.step(raw, offs, NOW, presence=False)
    same_step(g, c, rg, rc)
    bg = g.encode_block(NOW, rg, boot=0xabc)
    assert sg.verify(bg) == 0
    # the C++ encoder and index builder over the GPU's rows (its own name ids) and the oracle's
    # persisted records and string refs: the same block, pages and trailer, byte for byte
    ref = sg.encode_block(rg.out, rc.prec, rc.pspans, rc.raw, index=True, ctx=c.ctx_table())
    sg.seal(ref, rc.first_seq, NOW, 0xabc, 0, 1)
    assert len(ref) == len(bg), (len(ref), len(bg))
    assert np.array_equal(ref, bg), f"first differing byte at {np.nonzero(ref != bg)[0][:1]}"
    assert np.array_equal(sg.index_block(_strip_trailer(bg), g.ctx_table()), bg)
    check_trailer(bg, g.ctx_table())
    cols = sg.decode_block(bg)
    n_gen = g.stats_dict()["rule_alerts"]
    assert (cols["etype"][-n_gen:] == EV_ALERT).all() and n_gen > 100


def test_rules_replaced_then_cleared_between_steps():
    g, c = pair(FLEET_RULES)
    plain = GpuInboundEngine(small_cfg())
    setup_fleet(plain, n_dev=1000)
    batches = [fleet_batch(3000, seed=100 + k) for k in range(3)]
    for k, rules in enumerate((FLEET_RULES, many_rules(9), [])):
        for e in (g, c):
            e.set_measurement_rules(rules)
        raw, offs = batches[k]
        rg = g.step(raw, offs, NOW + k * 1000, presence=False)
        rc = c.step(raw, offs, NOW + k * 1000, presence=False)
        rp = plain.step(raw, offs, NOW + k * 1000, presence=False)
        same_step(g, c, rg, rc)
        assert g.stats_dict() == c.stats_dict()
        if rules:
            assert rg.n_persisted - rp.n_persisted == count_hits(rc.prec, rules) > 0
        else:
            assert rows(g, rg) == rows(plain, rp)        # as an engine that never had measurement rules
