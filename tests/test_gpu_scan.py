"""The device-wide exclusive scan (csrc/hip/swgpu.hip launch_scan, through sw_scan_u32) against
numpy's cumsum in uint32 (wrap-around is part of the contract): the single-workgroup path up to 16384
entries and the two-dispatch reduce-then-scan above it, whose scratch (one u32 per 1024 inputs) needs
no alignment, no prior contents and no re-arming between calls."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

TILE = 1024
BLOCK_MAX = 16384          # the last single-workgroup size
SIZES = [1, 255, 1024, BLOCK_MAX, BLOCK_MAX + 1, BLOCK_MAX + 3 * TILE + 1, 262151]   # the last: > 256 tiles
SENTINEL = 0x5A5A5A5A


def _scan(lib, d, x, tmp, tmp_len, with_total):
    """(rc, out, total) of one sw_scan_u32 call; out and total start as SENTINEL."""
    import torch
    n = len(x)
    xin = torch.from_numpy(x.view(np.int32)).to(d)
    out = torch.full((n,), SENTINEL, dtype=torch.int32, device=d)
    total = torch.full((1,), SENTINEL, dtype=torch.int32, device=d)
    s = torch.cuda.current_stream(d)
    P = ctypes.c_void_p
    rc = lib.sw_scan_u32(P(xin.data_ptr()), n, P(out.data_ptr()), P(total.data_ptr()) if with_total else None,
                         P(tmp.data_ptr()), tmp_len, P(s.cuda_stream))
    s.synchronize()
    return rc, out.cpu().numpy().view(np.uint32), int(total.cpu().numpy().view(np.uint32)[0])


@pytest.mark.parametrize("n", SIZES)
def test_scan_u32_matches_cumsum(n):
    import torch
    from sitewhere_amd._native import gpu
    lib = gpu()
    d = torch.device("cuda", 0)
    x = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    incl = np.cumsum(x, dtype=np.uint32)
    want = np.concatenate([np.zeros(1, np.uint32), incl[:-1]])
    nt = (n + TILE - 1) // TILE
    # scratch of exactly ceil(n / 1024) words at an odd word offset, every byte 0xFF, never cleared
    buf = torch.full((nt + 1,), -1, dtype=torch.int32, device=d)
    tmp = buf[1:]
    for with_total in (True, False):
        rc, out, total = _scan(lib, d, x, tmp, nt, with_total)
        assert rc == 0
        assert np.array_equal(out, want)
        assert total == (int(incl[-1]) if with_total else SENTINEL)
    if n > BLOCK_MAX:       # the single-workgroup path uses no scratch
        rc, out, total = _scan(lib, d, x, tmp, nt - 1, True)
        assert rc == -2
        assert np.all(out == SENTINEL) and total == SENTINEL
