"""The MI355X engine's whole device state (k_persist's pass 1, k_state_p2, both run twice a step)
against the CPU oracle after every step of the ``state_scenarios`` scripts: ties on the winning date
inside a batch and across steps, stale dates, one hot key, dates at and below zero, presence, a full
state map.  The state is read back from the engine's two tables whole; ``k_state_lookup`` is checked
against that dump on its own.  Everything is compared exactly."""
import functools

import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X GPU")]

if gpu_available():
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

from sitewhere_amd.models.columnar import MS_SLOT
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine

from state_scenarios import (D_NEG, N_DEV, OVERFLOW_DEV, SCRIPTS, STATE_SLOTS, batch_events, full_state,
                             implied_device_state, make_engine, run_script, state_diff)

CASES = [("tie", True), ("tie", False), ("stale", True), ("stale", False), ("hot", True), ("hot", False),
         ("epoch", True), ("presence", True)]


@functools.lru_cache(maxsize=None)
def oracle_run(name, cluster=True):
    e = make_engine(CpuInboundEngine, name, cluster=cluster)
    return e, run_script(e, name)


@functools.lru_cache(maxsize=None)
def gpu_run(name, cluster=True):
    e = make_engine(GpuInboundEngine, name, cluster=cluster)
    return e, run_script(e, name)


@pytest.mark.parametrize("name,cluster", CASES, ids=[f"{n}-{'clustered' if c else 'arrival'}" for n, c in CASES])
def test_whole_state_and_stats_match_oracle_after_every_step(name, cluster):
    _, got = gpu_run(name, cluster)
    _, want = oracle_run(name, cluster)
    assert len(got) == len(want) > 0
    for k, ((_, sg, tg), (_, sc, tc)) in enumerate(zip(got, want)):
        assert sg == sc, (k, state_diff(sg, sc))
        assert tg == tc, k


@pytest.mark.parametrize("name", ["tie", "epoch"])
def test_lookup_kernel_returns_the_dump_for_every_assignment(name):
    g, _ = gpu_run(name)
    c, _ = oracle_run(name)
    full = full_state(g)
    silent = 0
    for a in range(N_DEV):
        got = g.device_state(a)
        assert got == implied_device_state(full, g.names, a), a
        assert got == c.device_state(a), a
        silent += got["last_interaction"] == 0 and not got["measurements"] and not got["alerts"]
    assert silent > 0                                                    # an assignment without any state
    if name == "epoch":
        s = g.device_state(D_NEG)
        assert s["last_location"] is None and s["measurements"] == {} and set(s["alerts"]) == {"zone.enter"}


def test_lookup_kernel_before_any_name_is_known():
    g = make_engine(GpuInboundEngine, "tie")
    c = make_engine(CpuInboundEngine, "tie")
    assert int(g.t["nm_counter"].item()) == 0
    assert g.device_state(0) == c.device_state(0) == implied_device_state(full_state(g), g.names, 0)
    assert full_state(g) == full_state(c)


def test_same_bytes_from_two_runs():
    """Fresh engines, the tie script twice: the same assignment table byte for byte and the same
    occupied entries (slot positions may differ; name ids are claim-ordered, so raw keys are compared
    where the two runs interned alike, and by name hash always)."""
    a, ra = gpu_run("tie")
    b = make_engine(GpuInboundEngine, "tie")
    rb = run_script(b, "tie")
    assert a is not b
    assert a.t["st"].cpu().numpy().tobytes() == b.t["st"].cpu().numpy().tobytes()
    assert [s for _, s, _ in ra] == [s for _, s, _ in rb]
    if a.intern_table() == b.intern_table():
        def occupied(e):
            ms = e.t["ms"].cpu().numpy().view(MS_SLOT)
            return sorted((int(s["key"]), int(s["date"]), int(s["eid1"])) for s in ms[ms["key"] != 0])
        assert occupied(a) == occupied(b)


def test_full_state_map_merges_every_event_of_the_keys_it_holds():
    """64 slots, fewer than the probe bound: every probe visits every slot, so a key that holds a slot has
    had each of its events merged, and every row of a key without one is counted as an overflow."""
    g, got = gpu_run("overflow")
    c, want = oracle_run("overflow")
    rows = []
    for k, ((_, sg, tg), (rc, sc, tc)) in enumerate(zip(got, want)):
        rows += [key for key, _, _, _ in batch_events(rc)]
        assert len(sg["ms"]) == STATE_SLOTS < len(sc["ms"]), k
        assert all(sc["ms"].get(key) == v for key, v in sg["ms"].items()), k
        assert tg["state_overflow"] == sum(1 for key in rows if key not in sg["ms"]) > 0, k
        assert dict(tg, state_overflow=0) == tc and tc["state_overflow"] == 0, k
        assert sg["asg"] == sc["asg"], k
    assert got[0][1]["ms"].keys() == got[1][1]["ms"].keys()                  # a full table keeps its keys
    full = full_state(g)
    held = {key[0] for key in full["ms"]}
    for a in sorted(held)[:8] + [a for a in range(OVERFLOW_DEV) if a not in held][:8]:
        assert g.device_state(a) == implied_device_state(full, g.names, a), a
