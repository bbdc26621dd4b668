"""The MI355X engine's alternate-id dedup where probes chain, against the CPU oracle
(``dedup_scenarios``), and the store-backed filter's own kernels (sw_ff_add, sw_ff_clear) on a
test-owned table against ``FingerprintFilter``.

The engine scenarios reach the "bucket full, go on" branch and the wrap from the last bucket to
bucket 0 of all four forms of the chain rule in csrc/hip/swgpu.hip -- k_ff_add_rows (a step's
persisted ids), ff_add (seeding), k_ff_probe (16 lanes per id; its second load round with 5 and 8
generations, idle lanes with 3) and ff_has (dedup_verdict, in-batch repeats) -- then the lowest-index
rule over 48 copies of an id spread over lanes, waves and workgroups, and window chains that wrap the
table end in dedup_claim, dedup_verdict and dd_find."""
import ctypes
import functools

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

if gpu_available():
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine

from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.dedup_filter import MAX_PROBE, SLOTS, FingerprintFilter, ff_key, meta_words

import dedup_scenarios as S


# ------------------------------------------------------------------ engine scenarios
def _cfg(story, gens):
    return (S.small_window_cfg if story == "window_wrap_story" else S.cfg)(gens)


@functools.lru_cache(maxsize=None)
def oracle_run(story, gens):
    return getattr(S, story)(S.make_engine(CpuInboundEngine, _cfg(story, gens)))


@functools.lru_cache(maxsize=None)
def gpu_run(story, gens):
    return getattr(S, story)(S.make_engine(GpuInboundEngine, _cfg(story, gens), device="cuda:0"))


@pytest.mark.parametrize("gens", S.GENS)
def test_chain_add_fills_last_first_and_second_bucket(gens):
    """k_ff_add_rows: 40 ids homed in the last bucket, persisted in one step into generation gens - 1."""
    S.check_chain_add(S.cfg(gens), gpu_run("chain_story", gens), oracle_run("chain_story", gens))


@pytest.mark.parametrize("gens", S.GENS)
def test_chain_ids_are_rechecked_controls_persist(gens):
    """k_ff_probe along the chain (no id met a claimed key: its verdict is final)."""
    S.check_chain_probe(S.cfg(gens), gpu_run("chain_story", gens), oracle_run("chain_story", gens))


@pytest.mark.parametrize("gens", S.GENS)
def test_chain_probe_with_in_batch_repeats(gens):
    """ff_add (the chain is seeded) and ff_has (dedup_verdict settles every id of a batch with repeats)."""
    c = S.cfg(gens)
    S.check_repeats(c, gpu_run("repeat_story", gens), oracle_run("repeat_story", gens), S.seeded_reference(c))


@pytest.mark.parametrize("gens", (0,) + S.GENS)
def test_first_occurrence_is_the_lowest_index(gens):
    c = S.cfg(gens)
    got = gpu_run("first_occurrence_story", gens)
    S.check_first_occurrence(c, got, oracle_run("first_occurrence_story", gens))
    # the claim's own record: every repeated id holds one slot, and min(win - sb, lmin) is its first index
    _, lay, hashes = S.first_occurrence_batch(c.dedup_slots - 1)
    tab = got["window"]
    keys = tab[:, 0].view(np.uint64)
    for k, h in enumerate(hashes):
        at = np.nonzero(keys == np.uint64(h))[0]
        assert len(at) == 1, (k, at)
        word = int(tab[at[0], 1]) & M64
        win, lmin = ((word & 0xFFFFFFFF) - got["seq_base"]) & 0xFFFFFFFF, word >> 32
        copies = np.nonzero(lay == k)[0]
        assert win in copies.tolist() and min(win, lmin) == copies[0], (k, win, lmin)
        # lmin: the lowest index among the copies that lost the CAS
        assert lmin == (copies[0] if win != copies[0] else copies[1]), (k, win, lmin)


@pytest.mark.parametrize("gens", (0,) + S.GENS)
def test_window_chain_wraps_the_table_end(gens):
    c = S.small_window_cfg(gens)
    got = gpu_run("window_wrap_story", gens)
    S.check_window_wrap(c, got, oracle_run("window_wrap_story", gens))
    # step A's table: the twelve ids sit in the last slot and slots 0 .. 10
    keys = got["window_keys"].view(np.uint64)
    where = [c.dedup_slots - 1] + list(range(S.N_SLOT - 1))
    assert sorted(keys[where].tolist()) == sorted(h for _, h in S.slot_ids(c.dedup_slots - 1))
    assert np.count_nonzero(keys) == S.N_SLOT


# ------------------------------------------------------------------ the filter's kernels on a test-owned table
PATTERN = 0xA5A5A5A5        # what the generations a call must not touch hold
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def int_ids(bmask, n, home=None, n_home=0):
    """``n`` uint64 hashes with pairwise distinct fingerprints, found by brute force: ``n_home`` of them
    (first in the list) homed in bucket ``home``, the others wherever they fall."""
    homed, free, fps = [], [], set()
    i = 0
    while len(homed) < n_home or len(free) < n - n_home:
        i += 1
        assert i < 200000
        h = (i * GOLD) & M64
        b, fp = ff_key(h, bmask)
        if fp in fps:
            continue
        if b == home and len(homed) < n_home:
            homed.append(h)
        elif len(free) < n - n_home:
            free.append(h)
        else:
            continue
        fps.add(fp)
    ids = homed + free
    assert len(ids) == n and len({ff_key(h, bmask)[1] for h in ids}) == n
    return tuple(ids)


class DeviceFilter:
    """A filter table on the GPU, generation ``g`` empty and every other one ``PATTERN``, and the
    oracle over the same bytes."""

    def __init__(self, gens, bmask, g):
        import torch
        from sitewhere_amd._native import gpu
        self.lib, self.d = gpu(), torch.device("cuda", 0)
        self.gens, self.bmask, self.g = gens, bmask, g
        host = np.full((bmask + 1, gens, SLOTS), PATTERN, np.uint32)
        host[:, g] = 0
        self.start = host
        self.tab = torch.from_numpy(host.view(np.int32).reshape(-1).copy()).to(self.d)
        self.meta = torch.from_numpy(meta_words(gens, 1 << 20)).to(self.d)
        self.oracle = FingerprintFilter(bmask + 1, gens, 1 << 20)
        self.oracle.tab[:] = host.reshape(-1)

    def _call(self, fn, *args):
        import torch
        s = torch.cuda.current_stream(self.d)
        rc = fn(*args, ctypes.c_void_p(s.cuda_stream))
        s.synchronize()
        return rc

    def add(self, hashes, gens=None, g=None):
        import torch
        P = ctypes.c_void_p
        h = torch.from_numpy(np.asarray(hashes, np.uint64).view(np.int64).copy()).to(self.d)
        return self._call(self.lib.sw_ff_add, P(self.tab.data_ptr()), self.bmask, self.gens if gens is None else gens,
                          self.g if g is None else g, P(self.meta.data_ptr()), P(h.data_ptr() if len(h) else None),
                          len(h))

    def clear(self, g, gens=None):
        return self._call(self.lib.sw_ff_clear, ctypes.c_void_p(self.tab.data_ptr()), self.bmask,
                          self.gens if gens is None else gens, g)

    def table(self):
        return self.tab.cpu().numpy().view(np.uint32).reshape(self.bmask + 1, self.gens, SLOTS)

    def dropped(self):
        return int(self.meta.cpu().numpy()[5])

    def others_untouched(self, tab, g=None):
        g = self.g if g is None else g
        keep = [x for x in range(self.gens) if x != g]
        return np.array_equal(tab[:, keep], self.start[:, keep])

    def oracle_add(self, hashes):
        for h in hashes:
            self.oracle.add(int(h), self.g)
        return self.oracle.tab.reshape(self.bmask + 1, self.gens, SLOTS)


def _fits_ids(bmask):
    n = 56 if bmask == 3 else 600          # 56 of the 64 slots of a 4-bucket generation
    return int_ids(bmask, n, home=bmask, n_home=40)


@pytest.mark.parametrize("bmask,gens,last", [(3, 2, False), (3, 2, True), (63, 3, False), (63, 3, True),
                                             (63, 8, False), (63, 8, True)])
def test_ff_add_chains_that_fit(bmask, gens, last):
    g = gens - 1 if last else 0
    ids = _fits_ids(bmask)
    assert sum(ff_key(h, bmask)[0] == bmask for h in ids) >= 40 and len(ids) <= (bmask + 1) * SLOTS
    f = DeviceFilter(gens, bmask, g)
    assert f.add(ids) == 0
    got, want = f.table(), f.oracle_add(ids)
    assert f.others_untouched(got) and f.others_untouched(want)
    assert f.dropped() == 0 == int(f.oracle.meta[5])
    assert ((got[:, g] != 0).sum(axis=1) == (want[:, g] != 0).sum(axis=1)).all()         # per-bucket fills
    assert (want[bmask, g] != 0).all() and (want[0, g] != 0).all()                       # the chain wraps
    fps = {ff_key(h, bmask)[1]: ff_key(h, bmask)[0] for h in ids}
    assert sorted(x for x in got[:, g].ravel().tolist() if x) == sorted(fps)
    assert sorted(got[:, g].ravel().tolist()) == sorted(want[:, g].ravel().tolist())
    probe = FingerprintFilter(bmask + 1, gens, 1)
    probe.tab[:] = 0
    probe.tab.reshape(got.shape)[:, g] = got[:, g]
    assert all(probe.has(h) for h in ids)
    # a fingerprint sits in the first bucket of its chain that had room: every bucket before it is full
    full = (got[:, g] != 0).all(axis=1)
    for b in range(bmask + 1):
        for fp in got[b, g][got[b, g] != 0].tolist():
            k = fps[fp]
            while k != b:
                assert full[k], (fp, fps[fp], b, k)
                k = (k + 1) & bmask


def _check_bounded(f, ids, placed, buckets):
    """``placed`` of ``ids`` are in generation g, all in ``buckets`` (every one of them full), the rest
    counted as dropped, as many as the oracle drops."""
    g, bmask = f.g, f.bmask
    assert f.add(ids) == 0
    got, want = f.table(), f.oracle_add(ids)
    assert f.others_untouched(got)
    have = [x for x in got[:, g].ravel().tolist() if x]
    assert len(have) == placed == np.count_nonzero(want[:, g])
    assert len(set(have)) == len(have) and set(have) <= {ff_key(h, bmask)[1] for h in ids}
    assert f.dropped() == len(ids) - placed == int(f.oracle.meta[5])
    fill = (got[:, g] != 0).sum(axis=1)
    assert fill.tolist() == [SLOTS if b in buckets else 0 for b in range(bmask + 1)]
    assert fill.tolist() == (want[:, g] != 0).sum(axis=1).tolist()


def test_ff_add_one_bucket_drops_the_rest():
    _check_bounded(DeviceFilter(2, 0, 1), int_ids(0, 20), 16, {0})


def test_ff_add_full_generation_drops_the_rest():
    assert MAX_PROBE == 64
    _check_bounded(DeviceFilter(3, MAX_PROBE - 1, 1), int_ids(MAX_PROBE - 1, 1100), MAX_PROBE * SLOTS, set(range(MAX_PROBE)))


def test_ff_add_probe_bound_in_a_table_with_room():
    """1034 ids homed in bucket 100 of 128: the chain takes MAX_PROBE buckets, 100 .. 127 and 0 .. 35."""
    ids = int_ids(127, 1034, home=100, n_home=1034)
    assert all(ff_key(h, 127)[0] == 100 for h in ids)
    _check_bounded(DeviceFilter(2, 127, 0), ids, MAX_PROBE * SLOTS, set(range(100, 128)) | set(range(36)))


def test_ff_add_again_changes_nothing_and_skips_zero():
    bmask, gens, g = 63, 3, 2
    ids = _fits_ids(bmask)
    f = DeviceFilter(gens, bmask, g)
    assert f.add(ids) == 0
    first = f.table().copy()
    assert f.add(ids) == 0 and f.add(ids[::-1]) == 0
    assert np.array_equal(f.table(), first) and f.dropped() == 0
    # a full generation: the ids it dropped are dropped (and counted) again, the table stays
    full = DeviceFilter(2, 0, 0)
    some = int_ids(0, 20)
    assert full.add(some) == 0
    t1, d1 = full.table().copy(), full.dropped()
    kept = [h for h in some if ff_key(h, 0)[1] in set(t1[0, 0].tolist())]
    assert d1 == 4 and len(kept) == SLOTS
    assert full.add(kept) == 0
    assert np.array_equal(full.table(), t1) and full.dropped() == d1
    # hash 0 is no id
    z = DeviceFilter(gens, bmask, g)
    assert z.add([0, 0, 0]) == 0
    assert np.array_equal(z.table(), z.start) and z.dropped() == 0
    assert z.add([0, ids[0], 0]) == 0
    assert np.count_nonzero(z.table()[:, g]) == 1 and z.table()[ff_key(ids[0], bmask)[0], g, 0] == ff_key(ids[0], bmask)[1]


def test_ff_add_and_clear_reject_bad_generations():
    f = DeviceFilter(3, 63, 1)
    ids = _fits_ids(63)[:50]
    assert f.add([]) == 0                                   # nothing to launch
    assert f.add([], gens=9) == 0
    for gens, g in ((1, 0), (9, 0), (3, 3), (3, -1)):
        assert f.add(ids, gens=gens, g=g) == -2, (gens, g)
        assert f.clear(g, gens=gens) == -2, (gens, g)
    assert np.array_equal(f.table(), f.start) and f.dropped() == 0


@pytest.mark.parametrize("gens,bmask", [(2, 0), (3, 63), (8, 255)])
def test_ff_clear_clears_one_generation(gens, bmask):
    """(2, 0): four 16-byte words, four threads of work."""
    import torch
    for g in sorted({0, gens // 2, gens - 1}):
        f = DeviceFilter(gens, bmask, g)
        rng = np.random.default_rng(gens * 1000 + bmask + g)
        host = rng.integers(1, 1 << 32, (bmask + 1, gens, SLOTS), dtype=np.uint64).astype(np.uint32)
        f.tab.copy_(torch.from_numpy(host.view(np.int32).reshape(-1)))
        assert f.clear(g) == 0
        got = f.table()
        want = host.copy()
        want[:, g] = 0
        assert np.array_equal(got, want), g
