"""Shared scenarios of the alternate-id dedup tests (CPU oracle, native engine and GPU engine): ids
crafted so that probes chain.  ``chain_ids`` all share the LAST bucket of the store-backed filter as
their home, so a generation that takes them fills buckets last / 0 / 1 (the wrap of ff_has, k_ff_probe,
k_ff_add_rows and ff_add in csrc/hip/swgpu.hip); ``control_ids`` live in the same buckets with other
fingerprints and must never be found; ``slot_ids`` share the last slot of the dedup window as their
home, so their chain wraps the table end (dd_find, dedup_claim, dedup_verdict).  All are found by brute
force over ``chain-<i>`` strings, once per run.

The scripts return plain observations (statuses, hashes, rows, stats) of one engine; the CPU test
compares the Python oracle with the native engine, the GPU test the MI355X engine with the oracle, and
both assert the facts a script is for (bucket fills, recheck and duplicate counts, one rotation)."""
import functools

import numpy as np

from sitewhere_amd.models import wire
from sitewhere_amd.models.columnar import ST_DUPLICATE, ST_RECHECK
from sitewhere_amd.pipeline.config import EngineConfig
from sitewhere_amd.pipeline.dedup_filter import SLOTS, FingerprintFilter, ff_key
from sitewhere_amd.pipeline.fleet import fingerprints, gen_tokens, hash64_strs, pack_messages

NOW = 1_700_000_000_000
N_DEV = 50
N_CAND = 20000                    # candidate strings chain-0 .. chain-19999
N_CHAIN, N_CONTROL, N_SLOT = 40, 40, 12
GENS = (2, 3, 5, 8)               # 3: idle lanes in k_ff_probe's groups; 5, 8: its second load round
BLK, WAVE = 256, 64               # workgroup and wave size of the dedup kernels (csrc/hip/swgpu.hip)
N_COPIES, N_REPEATED = 48, 8      # the first-occurrence batch: 8 ids, 48 copies each

BASE = dict(max_msgs=512, rec_cap=512, gen_cap=256, max_devices=64, max_assignments=64, store_cap=1 << 12,
            dedup_slots=1 << 10, name_slots=1 << 8, names_cap=64)


def cfg(gens, **kw):
    """The test configuration with ``gens`` filter generations (0: filter off)."""
    d = dict(BASE)
    if gens:
        d.update(dedup_filter_ids=192, dedup_filter_gens=gens)
    d.update(kw)
    return EngineConfig.small(**d)


def small_window_cfg(gens):
    """Batches of 128 in the same 1024-slot window: a generation takes three batches before it rotates
    (the 512-record configuration rotates after every step that claims an id)."""
    return cfg(gens, max_msgs=128, rec_cap=128)


def make_engine(cls, c, **kw):
    e = cls(c, **kw)
    heap, offs = gen_tokens("dev-", 0, N_DEV)
    d = e.register_devices(*fingerprints(heap, offs))
    e.set_assignments(d, d)
    return e


# ------------------------------------------------------------------ crafted ids
@functools.lru_cache(maxsize=None)
def candidates():
    strs = [f"chain-{i}" for i in range(N_CAND)]
    return strs, [int(h) for h in hash64_strs(strs)]


@functools.lru_cache(maxsize=None)
def chain_ids(bmask):
    """40 (string, hash) homed in the filter's last bucket, fingerprints pairwise distinct."""
    out, fps = [], set()
    for s, h in zip(*candidates()):
        b, fp = ff_key(h, bmask)
        if b == bmask and fp not in fps and len(out) < N_CHAIN:
            out.append((s, h))
            fps.add(fp)
    assert len(out) == N_CHAIN and len({ff_key(h, bmask)[1] for _, h in out}) == N_CHAIN
    return tuple(out)


@functools.lru_cache(maxsize=None)
def control_ids(bmask):
    """About 40 (string, hash) homed in the three buckets the chain fills (last, 0, 1), none of them a
    chain id and none with a chain id's fingerprint."""
    chain = {h for _, h in chain_ids(bmask)}
    fps = {ff_key(h, bmask)[1] for h in chain}
    per = {bmask: [], 0: [], 1: []}
    for s, h in zip(*candidates()):
        b, fp = ff_key(h, bmask)
        if b in per and h not in chain and fp not in fps and len(per[b]) < (N_CONTROL + 2) // 3:
            per[b].append((s, h))
    out = tuple(x for b in (bmask, 0, 1) for x in per[b])[:N_CONTROL]
    assert len(out) >= N_CONTROL - 4 and all(len(v) >= 10 for v in per.values()), {b: len(v) for b, v in per.items()}
    return out


@functools.lru_cache(maxsize=None)
def window_ids(dd_mask):
    """Every candidate whose home slot in the dedup window is the last one, in candidate order."""
    return tuple((s, h) for s, h in zip(*candidates()) if h & dd_mask == dd_mask)


def slot_ids(dd_mask):
    """12 (string, hash) homed in the window's last slot: their chain takes slots last, 0 .. 10."""
    out = window_ids(dd_mask)[:N_SLOT]
    assert len(out) == N_SLOT
    return out


def spare_slot_ids(dd_mask):
    """Further ids homed in the window's last slot (fresh ids that have to walk the whole chain)."""
    return window_ids(dd_mask)[N_SLOT:]


CLUSTER_SPAN = 20                 # home slots last, 0 .. 18 of the window: about 400 of the candidates


@functools.lru_cache(maxsize=None)
def cluster_ids(dd_mask):
    """The candidates homed in the window's last slot or the ``CLUSTER_SPAN - 1`` slots after the wrap,
    without the spare ones: persisted together they form one run of claimed slots from the last slot
    on, which a fresh id homed in the last slot has to walk to its end (``cluster_walk``)."""
    spare = {h for _, h in spare_slot_ids(dd_mask)}
    return tuple((s, h) for s, h in zip(*candidates())
                 if ((h & dd_mask) + 1) & dd_mask < CLUSTER_SPAN and h not in spare)


def cluster_walk(dd_mask):
    """Probes a fresh id homed in the last slot makes through a table that holds ``cluster_ids``
    (linear probing, any insertion order: the set of claimed slots does not depend on it)."""
    taken = set()
    for _, h in cluster_ids(dd_mask):
        slot = h & dd_mask
        while slot in taken:
            slot = (slot + 1) & dd_mask
        taken.add(slot)
    slot, n = dd_mask, 0
    while slot in taken:
        slot, n = (slot + 1) & dd_mask, n + 1
    return n


def fresh_ids(tag, n):
    """Filler ids no crafted set contains."""
    return [f"fill-{tag}-{i}" for i in range(n)]


def quiet_ids(tag, n, dd_mask):
    """``n`` fresh ids homed in the third quarter of the window, far from ``cluster_ids``' run."""
    strs = fresh_ids(tag, 8 * n + 64)
    out = [s for s, h in zip(strs, hash64_strs(strs).tolist())
           if (dd_mask + 1) // 2 <= h & dd_mask < 3 * (dd_mask + 1) // 4]
    assert len(out) >= n
    return out[:n]


# ------------------------------------------------------------------ messages and observations
def tok(d):
    return f"dev-{d % N_DEV:010d}"


def msg(alt, value, d=None):
    """One measurement of device ``d`` with alternate id ``alt``; ``value`` names the copy."""
    value = int(value)
    return wire.measurements(tok(value if d is None else d), {"t": float(value)}, event_date=NOW + value,
                             alternate_id=alt)


def msgs_for(ids, first_value=0):
    return [msg(s, first_value + k) for k, s in enumerate(ids)]


class Stepper:
    """Steps one engine with lists of messages, one batch sequence after the other."""

    def __init__(self, engine):
        self.e, self.k = engine, 0

    def __call__(self, msgs):
        raw, offs = pack_messages(msgs)
        self.k += 1
        return observe(self.e.step(raw, offs, NOW + 1_000_000 + self.k, presence=False))


def observe(res):
    """What a step did, in an engine-independent form: rejects event for event, persisted rows in order."""
    st = np.asarray(res.reject_status).astype(np.int64)
    o = res.out
    return {
        "n_persisted": int(res.n_persisted),
        "status": st.tolist(),
        "alt_hash": [int(x) for x in res.rejects["alt_hash"]],
        "reject_v0": np.asarray(res.rejects["v0"], np.float64).view(np.uint64).tolist(),
        "rechecks": sorted(int(x) for x in res.rejects["alt_hash"][st == ST_RECHECK]),
        "duplicates": sorted(int(x) for x in res.rejects["alt_hash"][st == ST_DUPLICATE]),
        "etype": [int(x) for x in o["etype"]],
        "assignment": [int(x) for x in o["assignment"]],
        "event_date": [int(x) for x in o["event_date"]],
        "v0": np.ascontiguousarray(o["v0"], np.float64).view(np.uint64).tolist(),        # bitwise
    }


def values(obs):
    """The persisted rows' values (each copy of an id carries its own)."""
    return np.array(obs["v0"], np.uint64).view(np.float64).tolist()


def filter_table(engine):
    """The engine's whole filter as [buckets, gens, 16] fingerprints, through its checkpoint."""
    c = engine.cfg
    ck = engine.checkpoint_state()
    f = FingerprintFilter(c.ff_buckets, c.dedup_filter_gens, c.dedup_filter_ids)
    f.load(ck["dd_ff_idx"], ck["dd_ff_rows"])
    return f, f.tab.reshape(c.ff_buckets, c.dedup_filter_gens, SLOTS).copy()


# ------------------------------------------------------------------ scripts
def walk_to_generation(step, engine, target, tag="walk"):
    """Steps of fresh ids until the filter's live generation is ``target`` (real rotations: k_state_p2
    clears, k_step_end flips).  Returns the number of steps."""
    c = engine.cfg
    n = 0
    while engine.filter_state()["live"] != target:
        assert n < 2 * c.dedup_filter_gens * (c.dedup_filter_ids // c.max_msgs + 1), "the filter never got there"
        step(msgs_for(fresh_ids(f"{tag}-{n}", c.max_msgs), 1000 * n))
        n += 1
    return n


def seed_chain(engine):
    """The chain into the LAST generation through the warm start (ff_add, the seeding path): ids come
    newest first, so a live generation's worth of fresh ids fills generation 0 and the chain ids after
    them land in the generation before it, gens - 1."""
    c = engine.cfg
    assert engine.filter_state()["live"] == 0
    newer = hash64_strs(fresh_ids("seed", c.dedup_filter_ids))
    chain = np.array([h for _, h in chain_ids(c.ff_buckets - 1)], np.uint64)
    engine.filter_seed_begin()
    assert engine.filter_seed(newer) + engine.filter_seed(chain) == len(newer) + len(chain)


def chain_story(engine):
    """Scenarios 1 and 2 on one engine: reach the last generation, persist the chain in one step,
    forget the window, then send chain and control ids once each."""
    c = engine.cfg
    bmask, G = c.ff_buckets - 1, c.dedup_filter_gens
    step = Stepper(engine)
    walk_to_generation(step, engine, G - 1)
    live_before = engine.filter_state()["live"]
    chain = [s for s, _ in chain_ids(bmask)]
    control = [s for s, _ in control_ids(bmask)]
    add = step(msgs_for(chain, 100))
    out = {"live_before": live_before, "add": add, "filter_after_add": engine.filter_state(),
           "table_after_add": filter_table(engine)[1], "stats_after_add": engine.stats_dict()}
    engine.reset_dedup()
    out["probe"] = step(msgs_for(chain + control, 200))
    out["filter_after_probe"] = engine.filter_state()
    out["stats_after_probe"] = engine.stats_dict()
    return out


def repeat_story(engine):
    """Scenario 3 on one engine: the chain seeded into the last generation, then chain and control ids
    twice in one batch (``msgs + msgs[::-1]``, every copy its own value)."""
    c = engine.cfg
    bmask = c.ff_buckets - 1
    step = Stepper(engine)
    seed_chain(engine)
    out = {"table_seeded": filter_table(engine)[1], "filter_seeded": engine.filter_state()}
    ids = [s for s, _ in chain_ids(bmask)] + [s for s, _ in control_ids(bmask)]
    out["repeat"] = step(msgs_for(ids, 200) + msgs_for(ids[::-1], 200 + len(ids)))
    out["filter"] = engine.filter_state()
    out["stats"] = engine.stats_dict()
    return out


def first_occurrence_layout():
    """Batch index -> repeated id (0..7) or -1 (a fresh id), 512 entries, 48 copies of each id:
    ids 0-1 neighbours (stride 1: lanes 22..45 of one wave and 0..23 of the next, in workgroup 0 and 1);
    ids 2-4 six lanes of all eight waves (stride 64: the waves of a workgroup, and both workgroups);
    ids 5-7 the same lanes of a wave of both workgroups (stride BLK).  No id's lowest index is at lane 0:
    it sits at lane 22, 46, 52, 58 or 10 of its lowest wave, with fresh ids in the lanes below."""
    lay = np.full(2 * BLK, -1, np.int64)
    lanes = np.arange(22, 46)

    def put(k, idx):
        idx = np.asarray(idx).ravel()
        assert len(idx) == N_COPIES and (lay[idx] == -1).all()
        lay[idx] = k

    for k, blk in ((0, 0), (1, 1)):                                          # stride 1
        put(k, np.concatenate([blk * BLK + lanes, blk * BLK + WAVE + np.arange(24)]))
    for k, lane0 in ((2, 46), (3, 52), (4, 58)):                             # stride 64
        put(k, [lane0 + j + WAVE * w for w in range(2 * BLK // WAVE) for j in range(6)])
    for k, wave in ((5, 2), (6, 3)):                                         # stride BLK
        put(k, [b * BLK + wave * WAVE + lanes for b in range(2)])
    put(7, [b * BLK + w * WAVE + np.arange(10, 22) for b in range(2) for w in (2, 3)])
    assert np.bincount(lay[lay >= 0]).tolist() == [N_COPIES] * N_REPEATED
    assert all(int(np.nonzero(lay == k)[0][0]) % WAVE >= 10 for k in range(N_REPEATED))
    return lay


@functools.lru_cache(maxsize=None)
def first_occurrence_batch(dd_mask):
    """(messages, layout, hashes of the repeated ids).  Message i carries value i.  The test is sharp only
    when a first copy does NOT win its id's CAS, so that it wins by the lowest-index rule alone.  With the
    window's retired generation holding ``cluster_ids`` (the step before), the first lanes of wave 0 of
    workgroup 0 -- the wave with most ids' first copies -- carry spare ids homed in the last slot: each
    walks the cluster's whole run in dd_find, hundreds of dependent loads, before its wave reaches the
    claim's CAS, and every other id of the batch is homed far from the run, so the later waves claim
    first (filter off; with the filter on a fresh id skips the retired generation and the race is open --
    on an MI355X the first copy lost the CAS of all eight ids in every run looked at, either way)."""
    lay = first_occurrence_layout()
    quiet = quiet_ids("first", N_REPEATED + len(lay), dd_mask)
    rep, fresh = quiet[:N_REPEATED], iter(quiet[N_REPEATED:])
    spare = [s for s, _ in spare_slot_ids(dd_mask)]
    ids = []
    for i, k in enumerate(lay.tolist()):
        if k >= 0:
            ids.append(rep[k])
        elif i < WAVE and spare:
            ids.append(spare.pop(0))
        else:
            ids.append(next(fresh))
    assert len(set(ids)) == N_REPEATED + int((lay < 0).sum())
    return tuple(msg(s, i) for i, s in enumerate(ids)), lay, tuple(int(h) for h in hash64_strs(rep))


def first_occurrence_story(engine):
    """Scenario 4 on one engine."""
    c = engine.cfg
    step = Stepper(engine)
    msgs, lay, _ = first_occurrence_batch(c.dedup_slots - 1)
    msgs = list(msgs)
    out = {"prime": step(msgs_for([s for s, _ in cluster_ids(c.dedup_slots - 1)], 5000))}
    if hasattr(engine, "t"):           # the GPU engine: the batch's first sequence, both window tables after it
        out["seq_base"] = int(engine.t["seq_base"].item())
    out["batch"] = step(msgs)
    if hasattr(engine, "t"):
        out["window"] = engine.t["dd_tab"].cpu().numpy().copy()
    out["stats_batch"] = engine.stats_dict()
    out["again"] = step(msgs)
    out["stats_again"] = engine.stats_dict()
    return out


def window_wrap_story(engine):
    """Scenario 5 on one engine (a ``small_window_cfg`` one): persist ``slot_ids``, replay them in the
    same generation, push fresh ids until the window rotates exactly once, replay them again."""
    c = engine.cfg
    step = Stepper(engine)
    ids = [s for s, _ in slot_ids(c.dedup_slots - 1)]
    out = {"stats0": engine.stats_dict(), "a": step(msgs_for(ids, 0))}
    if hasattr(engine, "t"):
        g = int(engine.t["dd_meta"][0].item())
        out["window_keys"] = engine.t["dd_tab"][g * c.dedup_slots:(g + 1) * c.dedup_slots, 0].cpu().numpy().copy()
    out["stats_a"] = engine.stats_dict()
    out["b"] = step(msgs_for(ids, 20))
    out["stats_b"] = engine.stats_dict()
    out["fill"] = []
    # a rotation shows in the stats of the step after the one that filled the generation
    while engine.stats_dict()["dedup_rotations"] == out["stats_b"]["dedup_rotations"]:
        assert len(out["fill"]) < 8, "the window never rotated"
        out["fill"].append(step(msgs_for(fresh_ids(f"rot-{len(out['fill'])}", c.max_msgs - N_SLOT), 1000)))
    out["stats_fill"] = engine.stats_dict()
    out["c"] = step(msgs_for(ids, 40))
    out["stats_c"] = engine.stats_dict()
    return out


# ------------------------------------------------------------------ checks of the scripts
def check_config(c):
    """The sizes the scenarios rely on, read from the configuration."""
    assert c.rec_cap == c.max_msgs == 2 * BLK
    assert c.dedup_slots == 2 * c.rec_cap            # every step that claims an id rotates the window
    if c.dedup_filter_ids:
        assert c.dedup_filter_ids == c.dedup_slots       # ids per generation: clamped up to the window
        assert c.ff_buckets > 3                          # the chain's three buckets are not the whole table


def check_id_sets(c):
    bmask, dd_mask = c.ff_buckets - 1, c.dedup_slots - 1
    chain, control, slot = chain_ids(bmask), control_ids(bmask), slot_ids(dd_mask)
    fps = [ff_key(h, bmask)[1] for _, h in chain]
    assert len(chain) == N_CHAIN and len(set(fps)) == N_CHAIN                  # distinct fingerprints
    assert all(ff_key(h, bmask)[0] == bmask for _, h in chain)
    assert N_CONTROL - 4 <= len(control) <= N_CONTROL
    assert {ff_key(h, bmask)[0] for _, h in control} == {bmask, 0, 1}
    assert not {ff_key(h, bmask)[1] for _, h in control} & set(fps)
    assert not {h for _, h in control} & {h for _, h in chain}
    assert len(slot) == N_SLOT and all(h & dd_mask == dd_mask for _, h in slot)
    assert len({h for _, h in slot}) == N_SLOT and len(spare_slot_ids(dd_mask)) >= 4
    assert N_SLOT < len(cluster_ids(dd_mask)) <= c.max_msgs and cluster_walk(dd_mask) >= c.rec_cap // 2


def oracle_filter(c, g, hashes, base=None):
    """A filter table [buckets, gens, 16] with ``hashes`` added to generation ``g`` of ``base``."""
    f = FingerprintFilter(c.ff_buckets, c.dedup_filter_gens, c.dedup_filter_ids)
    if base is not None:
        f.tab[:] = base.reshape(-1)
    for h in hashes:
        assert f.add(int(h), g)
    return f


def check_chain_in_table(c, tab, g, other):
    """Generation ``g`` of ``tab`` holds the chain in buckets last / 0 / 1 as 16 / 16 / 8 fingerprints,
    the oracle's as a set; every other bucket of every generation holds exactly ``other``'s fingerprints
    (bucket by bucket: which slot of its bucket an id takes is the add order's, a race on the GPU); the
    oracle's ``has`` over this table finds every chain id and no control."""
    bmask = c.ff_buckets - 1
    three = [bmask, 0, 1]
    chain = [h for _, h in chain_ids(bmask)]
    assert (tab[three, g] != 0).sum(axis=1).tolist() == [16, 16, 8]
    want = oracle_filter(c, g, chain).tab.reshape(tab.shape)
    assert (want[three, g] != 0).sum(axis=1).tolist() == [16, 16, 8]
    assert sorted(tab[three, g].ravel().tolist()) == sorted(want[three, g].ravel().tolist())
    assert sorted(x for x in tab[three, g].ravel().tolist() if x) == sorted(ff_key(h, bmask)[1] for h in chain)
    rest_got, rest_want = tab.copy(), other.copy()
    rest_got[three, g] = 0
    rest_want[three, g] = 0
    assert np.array_equal(np.sort(rest_got, axis=2), np.sort(rest_want, axis=2))
    f = FingerprintFilter(c.ff_buckets, c.dedup_filter_gens, c.dedup_filter_ids)
    f.tab[:] = tab.reshape(-1)
    assert all(f.has(h) for h in chain)
    assert not any(f.has(h) for _, h in control_ids(bmask))


def same(got, want, *keys):
    for k in keys:
        assert got[k] == want[k], k


OBS = ("n_persisted", "status", "alt_hash", "reject_v0", "etype", "assignment", "event_date", "v0")


def check_chain_add(c, got, want):
    """Scenario 1."""
    G = c.dedup_filter_gens
    assert got["live_before"] == want["live_before"] == G - 1               # >= 4 for 5 and 8 generations
    same(got["add"], want["add"], *OBS)
    assert got["add"]["n_persisted"] == N_CHAIN and not got["add"]["status"]
    assert got["filter_after_add"] == want["filter_after_add"]
    assert got["filter_after_add"]["dropped"] == 0 and got["filter_after_add"]["live_ids"] == N_CHAIN
    assert got["stats_after_add"] == want["stats_after_add"]
    # buckets last / 0 / 1 of the live generation were empty in the walk's table: the fresh ids of the
    # generations before are in other generations, so `want` minus the chain is `got` minus the chain
    check_chain_in_table(c, got["table_after_add"], G - 1, want["table_after_add"])


def check_chain_probe(c, got, want):
    """Scenario 2."""
    bmask = c.ff_buckets - 1
    chain = sorted(h for _, h in chain_ids(bmask))
    control = control_ids(bmask)
    p = got["probe"]
    same(p, want["probe"], *OBS)
    assert p["rechecks"] == chain and p["status"] == [ST_RECHECK] * N_CHAIN      # every chain id, nothing else
    assert p["n_persisted"] == len(control) == want["probe"]["n_persisted"]
    assert sorted(values(p)) == [float(200 + N_CHAIN + k) for k in range(len(control))]
    assert got["filter_after_probe"] == want["filter_after_probe"]
    assert got["filter_after_probe"]["dropped"] == 0
    assert got["filter_after_probe"]["live_ids"] == N_CHAIN + len(control)
    assert got["stats_after_probe"] == want["stats_after_probe"]
    assert got["stats_after_probe"]["dedup_rechecks"] == N_CHAIN


def check_repeats(c, got, want, seeded_other):
    """Scenario 3."""
    bmask, G = c.ff_buckets - 1, c.dedup_filter_gens
    chain = sorted(h for _, h in chain_ids(bmask))
    control = control_ids(bmask)
    n = N_CHAIN + len(control)
    assert got["filter_seeded"] == want["filter_seeded"] and got["filter_seeded"]["live"] == 0
    check_chain_in_table(c, got["table_seeded"], G - 1, seeded_other)
    r = got["repeat"]
    same(r, want["repeat"], *OBS)
    # the first copy of a chain id is the recheck (values 200 ..), its second the duplicate
    assert r["rechecks"] == chain
    assert r["duplicates"] == sorted(chain + [h for _, h in control])
    assert r["status"].count(ST_RECHECK) == N_CHAIN and r["status"].count(ST_DUPLICATE) == n
    v = dict(zip(zip(r["alt_hash"], r["status"]), np.array(r["reject_v0"], np.uint64).view(np.float64).tolist()))
    for k, (_, h) in enumerate(chain_ids(bmask)):
        assert v[(h, ST_RECHECK)] == 200.0 + k and v[(h, ST_DUPLICATE)] == 200.0 + 2 * n - 1 - k
    # control ids persist their first copy
    assert r["n_persisted"] == len(control)
    assert sorted(values(r)) == [float(200 + N_CHAIN + k) for k in range(len(control))]
    assert got["filter"] == want["filter"] and got["filter"]["dropped"] == 0
    assert got["stats"] == want["stats"]
    assert got["stats"]["dedup_rechecks"] == N_CHAIN and got["stats"]["duplicates"] == n


def check_first_occurrence(c, got, want):
    """Scenario 4."""
    msgs, lay, _ = first_occurrence_batch(c.dedup_slots - 1)
    assert len(msgs) == c.rec_cap == 2 * BLK
    assert got["prime"]["n_persisted"] == len(cluster_ids(c.dedup_slots - 1)) and not got["prime"]["status"]
    first = [int(np.nonzero(lay == k)[0][0]) for k in range(N_REPEATED)]
    fresh = np.nonzero(lay < 0)[0].tolist()
    same(got["prime"], want["prime"], *OBS)
    b = got["batch"]
    same(b, want["batch"], *OBS)
    assert got["stats_batch"] == want["stats_batch"]
    # exactly one row per repeated id, the lowest batch index's (message i carries value i)
    assert sorted(values(b)) == sorted(float(i) for i in first + fresh)
    assert b["n_persisted"] == N_REPEATED + len(fresh)
    assert b["status"] == [ST_DUPLICATE] * (N_REPEATED * (N_COPIES - 1))
    assert got["stats_batch"]["dedup_overflow"] == 0
    a = got["again"]
    same(a, want["again"], *OBS)
    assert a["n_persisted"] == 0 and a["status"] == [ST_DUPLICATE] * len(msgs)
    assert got["stats_again"] == want["stats_again"]


def check_window_wrap(c, got, want):
    """Scenario 5."""
    dd_mask = c.dedup_slots - 1
    slot = sorted(h for _, h in slot_ids(dd_mask))
    assert c.dedup_slots // 2 >= 3 * c.rec_cap            # a generation takes several batches
    for k in ("a", "b", "c"):
        same(got[k], want[k], *OBS)
    assert len(got["fill"]) == len(want["fill"]) >= 2
    for x, y in zip(got["fill"], want["fill"]):
        same(x, y, *OBS)
        assert not x["status"]
    for k in ("stats0", "stats_a", "stats_b", "stats_fill", "stats_c"):
        assert got[k] == want[k], k
        assert got[k]["dedup_overflow"] == 0
    assert got["a"]["n_persisted"] == N_SLOT and not got["a"]["status"]
    rot0 = got["stats_a"]["dedup_rotations"]
    # step B: the same generation, all duplicates
    assert got["stats_b"]["dedup_rotations"] == rot0
    assert got["b"]["n_persisted"] == 0 and got["b"]["duplicates"] == slot
    assert got["b"]["status"] == [ST_DUPLICATE] * N_SLOT
    # exactly one rotation, then the ids are the retired generation's
    assert got["stats_fill"]["dedup_rotations"] == rot0 + 1 == got["stats_c"]["dedup_rotations"]
    assert got["c"]["n_persisted"] == 0 and got["c"]["duplicates"] == slot
    assert got["c"]["status"] == [ST_DUPLICATE] * N_SLOT
    assert got["stats_c"]["dedup_rechecks"] == 0


def seeded_reference(c):
    """The oracle's filter table after ``seed_chain``'s fresh ids alone (generation 0)."""
    from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
    e = make_engine(CpuInboundEngine, c)
    e.filter_seed_begin()
    e.filter_seed(hash64_strs(fresh_ids("seed", c.dedup_filter_ids)))
    return filter_table(e)[1]
