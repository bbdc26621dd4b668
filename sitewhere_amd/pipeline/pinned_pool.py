"""Pinned host buffers a step's rows (or its durable block) are returned in without a copy."""
from __future__ import annotations

import sys

import torch


class PinnedPool:
    """Pinned host buffers (torch tensor + its full numpy view) with ``HEADROOM`` bytes in front of
    the payload, handed out once no earlier ``StepResult`` references them: a live ``result.out``
    view pins its base array, so results are returned without a copy and without fresh pageable
    pages per step.  ``full``: the largest payload a buffer ever holds; ``limit`` / ``spill``: how
    many pooled and spill buffers are kept."""

    HEADROOM = 1 << 16          # bytes kept free in front of the rows: a columnar batch header is
                                # written there, making header + rows one contiguous payload

    def __init__(self, full: int, limit: int, spill: int):
        self.full, self.limit, self.spill_limit = int(full) + self.HEADROOM, limit, spill
        self.pool, self.spill = [], []
        self.stats = {"reused": 0, "new_pooled": 0, "spill": 0, "new_unpooled": 0}

    def get(self, nbytes: int):
        """(tensor, array, pooled) for ``nbytes`` of payload; a result whose buffer is not pooled
        must not be retained (``StepResult.frame_base`` is left unset)."""
        need = nbytes + self.HEADROOM
        pool, spill, st, full = self.pool, self.spill, self.stats, self.full
        for pin, arr in pool:
            if arr.nbytes >= need and sys.getrefcount(arr) <= 3:   # pool tuple, loop variable, the call
                st["reused"] += 1
                return pin, arr, True
        # sized to this step's rows plus slack (steps of one tenant are about the same size), not to
        # the engine's full output capacity: pinning a buffer costs time in proportion to its size
        size = max(need, min(full, -(-(need + need // 4) // (1 << 20)) * (1 << 20)))
        # never smaller than the largest pooled buffer: steps of a tenant that coalesces records vary
        # in size, and pinning a fresh buffer for each new maximum costs milliseconds per step
        if pool:
            size = max(size, min(full, max(a.nbytes for _, a in pool)))
        # results held by an overlapped tenant: in flight + store queue + storing, and -- with zero-copy
        # columnar payloads -- the batches the store and the enriched-batch topic retain
        if len(pool) < self.limit:
            pin = torch.empty(size, dtype=torch.uint8).pin_memory()
            pool.append((pin, pin.numpy()))
            st["new_pooled"] += 1
            return pin, pool[-1][1], True
        # every pooled buffer is retained downstream: hand out a spill buffer that must not be
        # retained (the caller copies its rows), so a full pool costs a copy, not a pinned
        # allocation per step
        for pin, arr in spill:
            if arr.nbytes >= need and sys.getrefcount(arr) <= 3:
                st["spill"] += 1
                return pin, arr, False
        pin = torch.empty(size, dtype=torch.uint8).pin_memory()
        if len(spill) < self.spill_limit:
            spill.append((pin, pin.numpy()))
            st["spill"] += 1
            return pin, spill[-1][1], False
        st["new_unpooled"] += 1
        return pin, pin.numpy(), False
