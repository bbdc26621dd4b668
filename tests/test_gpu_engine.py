"""GPU engine (libswgpu.so on gfx950) vs the CPU oracle engine -- bitwise parity where deterministic.

Validated events persist in stable order on both engines, so their event ids, store rows and
outbound rows match exactly; generated rule/presence events are compared as multisets.
"""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X GPU")]

if gpu_available():
    import torch
    from sitewhere_amd.pipeline.gpu_engine import GpuInboundEngine, PipelinedRunner

from sitewhere_amd.models.columnar import EV_STATE_CHANGE
from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine

from pipeline_scenarios import NOW, setup_fleet, small_cfg, hand_batch, fleet_batch, canon_out
from state_scenarios import full_state, state_diff


def pair(**kw):
    g = GpuInboundEngine(small_cfg(**kw))
    c = CpuInboundEngine(small_cfg(**kw))
    setup_fleet(g, n_dev=1000)
    setup_fleet(c, n_dev=1000)
    return g, c


def assert_same_step(rg, rc, names):
    assert rg.n_events == rc.n_events
    assert rg.n_persisted == rc.n_persisted
    assert canon_out(rg.out, names) == canon_out(rc.out, names)
    # rejected records: same multiset of (status, bytes)
    kg = sorted(zip(rg.reject_status.tolist(), [bytes(x) for x in rg.rejects.view(np.uint8).reshape(-1, 80)]))
    kc = sorted(zip(rc.reject_status.tolist(), [bytes(x) for x in rc.rejects.view(np.uint8).reshape(-1, 80)]))
    assert kg == kc


def test_abi_sizes_match():
    from sitewhere_amd._native import gpu
    from sitewhere_amd.ops.engine_abi import abi_sizes, SwEngineArgs
    import ctypes
    s = abi_sizes(gpu())
    assert s["event_rec"] == 80 and s["out_rec"] == 32 and s["name_ref"] == 16
    assert s["engine_args"] == ctypes.sizeof(SwEngineArgs)
    assert [s["reg_slot"], s["asg_state"], s["ms_slot"]] == [32, 32, 32]
    from sitewhere_amd.models.columnar import WIRE_REC
    assert s["wire_rec"] == WIRE_REC.itemsize == 64
    from sitewhere_amd.models.columnar import STEP_SNAPSHOT
    assert s["step_snapshot"] == STEP_SNAPSHOT.itemsize == 128


def test_hand_batch_parity():
    g, c = pair()
    raw, offs = hand_batch()
    rg = g.step(raw, offs, NOW, presence=False)
    rc = c.step(raw, offs, NOW, presence=False)
    assert_same_step(rg, rc, c.names)
    assert g.stats_dict() == c.stats_dict()
    assert rg.new_names == rc.new_names


def test_fleet_parity_multi_step_with_state():
    g, c = pair()
    for k in range(4):
        raw, offs = fleet_batch(3000, seed=100 + k)
        rg = g.step(raw, offs, NOW + k * 1000, presence=False)
        rc = c.step(raw, offs, NOW + k * 1000, presence=False)
        assert_same_step(rg, rc, c.names)
    assert g.stats_dict() == c.stats_dict()
    # store contents (ordered part: everything but generated rows)
    cg, eg = g.store_rows()
    cc, ec = c.store_rows()
    assert np.array_equal(eg, ec)
    for k in ("etype", "dev", "asg", "cust", "area", "asset", "date", "recv"):
        assert sorted(cg[k].tolist()) == sorted(cc[k].tolist()), k
    # the whole device state: every assignment, every (name, kind) entry, dates and winning event ids
    sg, sc = full_state(g), full_state(c)
    assert sg == sc, state_diff(sg, sc)


def test_presence_parity():
    g, c = pair()
    raw, offs = fleet_batch(2000, seed=5)
    g.step(raw, offs, NOW, presence=False)
    c.step(raw, offs, NOW, presence=False)
    later = NOW + g.cfg.presence_missing_ms + 5
    empty_raw, empty_off = np.zeros(64, np.uint8), np.zeros(1, np.uint32)
    rg = g.step(empty_raw, empty_off, later, presence=True)
    rc = c.step(empty_raw, empty_off, later, presence=True)
    assert (rg.out["etype"] == EV_STATE_CHANGE).sum() == (rc.out["etype"] == EV_STATE_CHANGE).sum() > 0
    assert sorted(rg.out["assignment"].tolist()) == sorted(rc.out["assignment"].tolist())


@pytest.mark.parametrize("mode", ["direct", "push", "sdma", "hsa"])
def test_pipelined_runner_matches_sync(mode):
    g, c = pair()
    seen = []
    runner = PipelinedRunner(g, max_raw_bytes=1 << 20, on_outbound=lambda rows: seen.append(rows.copy()), mode=mode)
    batches = [fleet_batch(2000, seed=300 + k) for k in range(5)]
    total = 0
    cpu_rows = []
    for k, (raw, offs) in enumerate(batches):
        rh = torch.from_numpy(raw).pin_memory()
        oh = torch.from_numpy(offs.view(np.int32)).pin_memory()
        runner.submit(rh, oh, len(offs) - 1, now_ms=NOW + k)
        r = c.step(raw, offs, NOW + k, presence=False)
        total += r.n_persisted
        cpu_rows.append(r.out)
    runner.flush()
    assert runner.delivered == total == sum(len(x) for x in seen)
    assert g.stats_dict() == c.stats_dict()
    assert canon_out(np.concatenate(seen), None) == canon_out(np.concatenate(cpu_rows), None)


def test_varint_framing_kernel_matches_host_offsets():
    from sitewhere_amd.pipeline.framing import varint_lengths
    g = GpuInboundEngine(small_cfg(max_msgs=8192))
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.integers(0, 128, 5000), rng.integers(128, 70000, 200), [0, 127, 128, 16383, 16384]])
    rng.shuffle(lens)
    offs = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    stream = varint_lengths(offs)
    assert len(stream) > len(lens)              # some multi-byte varints cross tile boundaries
    ld = torch.from_numpy(stream).cuda()
    od = torch.full((len(lens) + 8,), -1, dtype=torch.int32, device="cuda")
    g.frame_varint(ld, len(stream), len(lens), od, int(offs[-1]))
    torch.cuda.synchronize()
    assert np.array_equal(od[:len(lens) + 1].cpu().numpy().view(np.uint32).astype(np.int64), offs)


def test_pipelined_runner_varint_framing_matches_sync():
    from sitewhere_amd.pipeline.framing import varint_lengths
    g, c = pair()
    seen = []
    runner = PipelinedRunner(g, max_raw_bytes=1 << 20, on_outbound=lambda rows: seen.append(rows.copy()))
    total = 0
    cpu_rows = []
    for k in range(4):
        raw, offs = fleet_batch(2000, seed=700 + k)
        rh = torch.from_numpy(raw).pin_memory()
        lh = torch.from_numpy(varint_lengths(offs)).pin_memory()
        runner.submit(rh, None, len(offs) - 1, now_ms=NOW + k, lens_host=lh, raw_bytes=int(offs[-1]))
        r = c.step(raw, offs, NOW + k, presence=False)
        total += r.n_persisted
        cpu_rows.append(r.out)
    runner.flush()
    assert runner.delivered == total == sum(len(x) for x in seen)
    assert g.stats_dict() == c.stats_dict()
    assert canon_out(np.concatenate(seen), None) == canon_out(np.concatenate(cpu_rows), None)


def test_standalone_pip_kernel():
    import ctypes
    from sitewhere_amd._native import gpu
    from sitewhere_amd.pipeline.cpu_engine import pip
    rng = np.random.default_rng(0)
    poly = np.array([(0, 0), (0, 4), (2, 2), (4, 4), (4, 0)], np.float64)
    pts = rng.uniform(-1, 5, size=(4096, 2))
    d = torch.device("cuda")
    out = torch.zeros(len(pts), dtype=torch.uint8, device=d)
    vt = torch.from_numpy(poly.ravel()).to(d)
    off = torch.tensor([0, len(poly)], dtype=torch.int32, device=d)
    pt = torch.from_numpy(pts.ravel()).to(d)
    rc = gpu().sw_pip_batch(pt.data_ptr(), len(pts), vt.data_ptr(), off.data_ptr(), 1, out.data_ptr(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = out.cpu().numpy().astype(bool)
    want = np.array([pip(poly, x, y) for x, y in pts])
    assert (got == want).all()


def test_graph_replay_matches_direct_launches_and_recaptures_on_zone_change():
    """The hipGraph-captured process phase gives the same results as direct launches, including
    across a zone-rule change (which must re-capture: zone pointers are by-value kernel args)."""
    from sitewhere_amd.pipeline.engine_base import Zone, ZoneTest
    g = GpuInboundEngine(small_cfg())
    d = GpuInboundEngine(small_cfg())
    d.use_graph = False
    for e in (g, d):
        setup_fleet(e, n_dev=1000)
    for k in range(6):
        if k == 3:
            for e in (g, d):
                e.set_zone_rules([Zone("z2", [(32.0, -86.0), (32.0, -84.0), (34.5, -84.0), (34.5, -86.0)])],
                                 [ZoneTest("z2", "inside", "zone2.enter", 3)])
        raw, offs = fleet_batch(2500, seed=700 + k)
        rg = g.step(raw, offs, NOW + k * 1000, presence=(k == 5))
        rd = d.step(raw, offs, NOW + k * 1000, presence=(k == 5))
        assert canon_out(rg.out, None) == canon_out(rd.out, None)
        assert g.stats_dict() == d.stats_dict()
    assert g._graph is not None


def test_store_ring_wraparound_parity():
    """The HBM event ring wraps (store_cap << events): GPU ring contents and ids match the oracle."""
    g, c = pair(store_cap=4096)
    for k in range(5):
        raw, offs = fleet_batch(1500, seed=900 + k)
        rg = g.step(raw, offs, NOW + k * 1000, presence=False)
        rc = c.step(raw, offs, NOW + k * 1000, presence=False)
        assert rg.first_seq == rc.first_seq
        assert canon_out(rg.out, None) == canon_out(rc.out, None)
    assert g.cursor == c.cursor > 4096
    cg, eg = g.store_rows()
    cc, ec = c.store_rows()
    assert len(eg) == 4096 and np.array_equal(eg, ec)
    for k in ("etype", "asg", "date"):
        assert sorted(cg[k].tolist()) == sorted(cc[k].tolist()), k


@pytest.mark.gpu
def test_hot_store_query_kernel_matches_cpu_oracle():
    """k_store_filter + device ordering vs the CPU oracle's query_store after the HBM ring wrapped."""
    from sitewhere_amd.models.columnar import EV_ALERT, EV_LOCATION, EV_MEASUREMENT
    g = GpuInboundEngine(small_cfg(store_cap=1 << 12), device="cuda:0")
    c = CpuInboundEngine(small_cfg(store_cap=1 << 12))
    for e in (g, c):
        setup_fleet(e, n_dev=200)
    for k in range(5):
        raw, offs = fleet_batch(1500, seed=70 + k, n_dev=200)
        g.step(raw, offs, NOW + k, presence=False)
        c.step(raw, offs, NOW + k, presence=False)
    assert g.cursor == c.cursor > g.cfg.store_cap
    for et, asg, lo, hi, pn, ps in ((EV_MEASUREMENT, [1, 2, 3, 150], None, None, 1, 10),
                                    (EV_LOCATION, list(range(0, 200, 3)), NOW - 40_000, NOW, 2, 25),
                                    (EV_ALERT, list(range(200)), None, None, 1, 0)):
        tg, pg, eg = g.query_store(et, asg, lo, hi, pn, ps)
        tc, pc, ec = c.query_store(et, asg, lo, hi, pn, ps)
        assert tg == tc and np.array_equal(eg, ec)
        for k in ("date", "asg", "v0", "v1", "etype"):
            assert np.array_equal(pg[k], pc[k]), k


def test_hot_store_query_dense_partial_chunk_stray_indices_and_empty():
    """query_store against the CPU oracle, all exact, where the match compactor can go wrong: an
    unwrapped ring whose row count is a multiple of neither the wave (64) nor the 1024-row chunk, with
    most rows of every chunk matching; an assignment set with indices outside [0, max_assignments),
    which are ignored; a query nothing matches; a ring no step has written to."""
    from sitewhere_amd.models.columnar import EV_ALERT, EV_MEASUREMENT
    g = GpuInboundEngine(small_cfg(store_cap=1 << 12), device="cuda:0")
    c = CpuInboundEngine(small_cfg(store_cap=1 << 12))

    def same(*q):
        (tg, pg, eg), (tc, pc, ec) = g.query_store(*q), c.query_store(*q)
        assert tg == tc and np.array_equal(eg, ec)
        for k in ("date", "asg", "etype", "v0", "v1"):
            assert np.array_equal(pg[k], pc[k]), k
        return tg, len(eg)

    every = list(range(g.cfg.max_assignments))
    assert same(EV_MEASUREMENT, every, None, None, 1, 0) == (0, 0)            # no step yet: an empty page
    for e in (g, c):
        setup_fleet(e, n_dev=200)
        raw, offs = fleet_batch(1500, seed=70, n_dev=200)
        e.step(raw, offs, NOW, presence=False)
    n = g.cursor
    assert n == c.cursor and 2048 < n < g.cfg.store_cap and n % 64 and n % 1024      # two full chunks and a part
    total, page = same(EV_MEASUREMENT, every, None, None, 1, 0)
    assert total == page and 2 * total > n
    stray = [-1, -4097, 3, 150, g.cfg.max_assignments, g.cfg.max_assignments + 31, 1 << 20]
    assert same(EV_MEASUREMENT, stray, None, None, 1, 0) == same(EV_MEASUREMENT, [3, 150], None, None, 1, 0)
    assert same(EV_MEASUREMENT, stray, None, None, 1, 0)[0] > 0
    assert same(EV_MEASUREMENT, every, NOW + 10_000_000, None, 1, 0) == (0, 0)
    assert same(EV_ALERT, [199 + 1000], None, None, 1, 10) == (0, 0)


def test_overlapped_framed_steps_match_sync_oracle():
    """submit_framed / drain_framed (the service tenant's overlapped steps): batch k is returned when
    batch k+2 is submitted, from pinned zero-copy records.  Every result -- rows, rejects, learned
    names, first store sequence -- equals the CPU oracle's synchronous step of the same batch, and a
    synchronous step is refused while a submission is pending."""
    from sitewhere_amd.pipeline.bus_io import RawBatchRecord, parse_raw_batch
    from sitewhere_amd.pipeline.framing import varint_lengths
    g, c = pair()
    recs, want, got = [], [], []
    for k in range(6):
        raw, offs = fleet_batch(2500, seed=700 + k)
        rec = RawBatchRecord(raw[:int(offs[-1])], varint_lengths(offs), len(offs) - 1)
        recs.append(rec)
        want.append(c.step(raw, offs, NOW + k, presence=False))
        got += g.submit_framed(parse_raw_batch(rec.buf.numpy()[:rec.value_len]), NOW + k, token=k, presence=False)
        assert [t for t, _ in got] == list(range(max(0, k - 1)))   # rows of k-1 are still copying
        assert g.framed_pending == min(k + 1, 2)
        if k == 2:
            with pytest.raises(RuntimeError, match="pending"):
                g.step(raw, offs, NOW, presence=False)
    got += g.drain_framed()
    assert [t for t, _ in got] == list(range(6)) and not g.framed_pending
    for (_, rg), rc in zip(got, want):
        assert_same_step(rg, rc, c.names)
        assert rg.first_seq == rc.first_seq and rg.new_names == rc.new_names
        assert rg.n_msgs == rc.n_msgs and rg.n_events == rc.n_events
    assert g.stats_dict() == c.stats_dict()
    assert sum(len(r.rejects) for _, r in got) > 0                # unregistered devices were rejected


class _StubSink:
    """A durable-block sink over mapped pinned host memory: ``target`` hands out a buffer the copy
    engine writes, ``publish`` seals the block and keeps a copy of it."""

    def __init__(self, lib, boot):
        self.lib, self.boot, self.published = lib, boot, []

    def target(self, nbytes):
        from sitewhere_amd.pipeline.gpu_engine import HostBuffer
        hb = HostBuffer(self.lib, nbytes)
        return hb.host, hb

    def publish(self, buf, nbytes, first_seq, now, tag):
        from sitewhere_amd.persistence import segments as sg
        blk = buf.view(np.uint8, nbytes).copy()
        sg.seal(blk, first_seq, now, self.boot, 0, 1)
        self.published.append((tag, int(first_seq), blk))


@pytest.mark.parametrize("block_index", [False, True], ids=["plain", "indexed"])
def test_pipelined_runner_block_sink_and_rejects_match_oracle(block_index):
    """The runner as the benchmark drives it: a durable-block sink (the encoder's last workgroup
    writes the step snapshot; with ``block_index`` the index build's patches the block bytes) and a
    reject callback, five batches over the three-slot ring.  Every step's block, first sequence, tag
    and routed rejects equal the CPU oracle's synchronous step of the same batch."""
    from sitewhere_amd.persistence import segments as sg
    from sitewhere_amd.pipeline import routing
    from tests.test_gpu_index import _strip_trailer
    from tests.test_gpu_segments import _decoded_equal
    g, c = pair(block_index=block_index)
    sink = _StubSink(g.lib, boot=0xabc)
    rejects = {}
    runner = PipelinedRunner(g, max_raw_bytes=1 << 20, deliver_outbound=False, block_sink=sink,
                             on_rejects=lambda tag, refs, comp: rejects.__setitem__(tag, (refs.copy(), comp.copy())))
    parts = (8, 4, 8, 2)
    want, total = [], 0
    for k in range(5):
        raw, offs = fleet_batch(2000, seed=300 + k)
        rh = torch.from_numpy(raw).pin_memory()
        oh = torch.from_numpy(offs.view(np.int32)).pin_memory()
        runner.submit(rh, oh, len(offs) - 1, now_ms=NOW + k, tag=k)
        rc = c.step(raw, offs, NOW + k, presence=False)
        host = routing.route_rejects(raw, offs, rc.rejects["aux_off"], rc.reject_status, "gpu-inbound", parts)
        want.append((rc.first_seq, c.encode_block(NOW + k, rc, boot=0xabc), host))
        total += rc.n_persisted
    runner.flush()
    assert runner.delivered == total > 0
    assert [t for t, _, _ in sink.published] == list(range(5))
    gi = {i: h for h, i in g.intern_table().items()}
    ci = {i: h for h, i in c.intern_table().items()}
    to_hash = lambda ids, inv: [inv.get(int(i), -1) if i != 0xFFFF else -1 for i in ids]  # noqa: E731
    for k, ((_, first, bg), (cfirst, bc, host)) in enumerate(zip(sink.published, want)):
        assert first == cfirst, f"step {k}"
        assert sg.verify(bg) == 0
        cg, cc = sg.decode_block(bg), sg.decode_block(bc)
        _decoded_equal(cg, cc, f"step {k}")
        assert to_hash(cg["name"], gi) == to_hash(cc["name"], ci), f"step {k}: names differ"
        assert cg["header"]["first_seq"] == cfirst
        if block_index:
            assert np.array_equal(sg.index_block(_strip_trailer(bg), g.ctx_table()), bg), f"step {k}: trailer"
        if k not in rejects:                    # no callback: the step had nothing to route
            assert len(host) == 0, f"step {k}"
            continue
        gpu = routing.route_refs(rejects[k][1], rejects[k][0], 0, "gpu-inbound", parts)
        assert len(gpu) > 0 and gpu.payloads == host.payloads, f"step {k}"
        gk = sorted((q, p, bytes(kh), bytes(vh)) for q, p, kh, ko, vh, vo in gpu.groups())
        hk = sorted((q, p, bytes(kh), bytes(vh)) for q, p, kh, ko, vh, vo in host.groups())
        assert gk == hk, f"step {k}"
    assert len(rejects) > 0
    assert g.stats_dict() == c.stats_dict()


def test_step_snapshot_kernel_writes_the_named_layout():
    """``k_step_snapshot`` on its own, after a synchronous step, its block encode and its reject
    snapshot: every word of the record it writes into mapped host memory against the device values
    it copies; without a produced step only the carry words are set."""
    from sitewhere_amd.models.columnar import SC_NAMES, SEG_ST_BYTES, SEG_ST_FIRST, STEP_SNAPSHOT
    from sitewhere_amd.pipeline.gpu_engine import HostBuffer
    g, _ = pair()
    raw, offs = hand_batch()
    g.step(raw, offs, NOW, presence=False)
    slot = g._last_sel
    meta = g.encode_block_async(slot)
    cnt, _ = g.reject_refs_async(slot, g._stg[2], g._stg[3], len(offs) - 1)
    carry = torch.tensor([7, 9], dtype=torch.int32, device=g.device)      # one rank keeps no carry: stand-ins
    hb = HostBuffer(g.lib, 256)
    stream = torch.cuda.current_stream(g.device)

    def snapshot(produced):
        hb.view(np.uint8, 256)[:] = 0
        hb.view(np.uint8, STEP_SNAPSHOT.fields["pad"][1])[:] = 0xA5       # every word the kernel owns
        rc =g.lib.sw_step_snapshot(g.t["scalars"].data_ptr(), meta.data_ptr(), cnt.data_ptr(), carry.data_ptr(),
                                    produced, hb.dev, stream.cuda_stream)
        assert rc == 0
        stream.synchronize()
        return hb.view(STEP_SNAPSHOT, 1)[0].copy()

    s = snapshot(1)
    sc = g.scalars()
    assert sc["n_out"] > 0 and sc["n_rej"] > 0
    words = g.t["scalars"][:16].cpu().numpy().view(np.uint32)
    assert s["scalars"].tolist() == words.tolist()
    assert {n: int(s["scalars"][i]) for i, n in enumerate(SC_NAMES)} == sc
    _, state, pages, cap = g._seg_buffers(slot)
    st = state[pages + SEG_ST_BYTES:pages + SEG_ST_FIRST + 1].cpu().numpy().view(np.uint64)
    assert [int(s["block_bytes"]), int(s["block_errors"]), int(s["block_first_seq"])] == [int(x) for x in st]
    assert 0 < int(s["block_bytes"]) <= cap and int(s["block_errors"]) == 0
    counters = cnt.cpu().numpy().view(np.uint32)
    assert [int(s["rej_refs"]), int(s["rej_bytes"])] == [int(counters[0]), int(counters[1])]
    assert int(s["rej_refs"]) > 0
    assert s["n_carry"].tolist() == [7, 9]
    s0 = snapshot(0)
    assert s0["n_carry"].tolist() == [7, 9]
    s0["n_carry"] = 0
    assert s0.tobytes() == bytes(STEP_SNAPSHOT.itemsize)
