"""The ctypes mirror of the engine's argument block (sitewhere_amd/ops/engine_abi.py) against the
struct it mirrors (csrc/include/swengine.h): the same fields, of the same kind, in the same order.
The size alone (tests/test_gpu_engine.py test_abi_sizes_match) cannot tell two swapped fields apart."""
from __future__ import annotations

import ctypes
import re

import numpy as np
from pathlib import Path

from sitewhere_amd.ops import engine_abi

HEADER = Path(__file__).resolve().parent.parent / "csrc" / "include" / "swengine.h"


def test_engine_args_fields_match_header():
    text = HEADER.read_text()
    body = re.search(r"typedef struct SwEngineArgs \{(.*?)\} SwEngineArgs;", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
        assert m, f"unparsed declaration in SwEngineArgs: {decl!r}"
        ctype, ptr, name = m.groups()
        kind = ctypes.c_void_p if ptr else {"int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}[ctype]
        fields.append((name, kind))
    assert len(fields) == 132
    assert fields == engine_abi.FIELDS
    assert ctypes.sizeof(engine_abi.SwEngineArgs) == 8 * len(fields)


def test_step_snapshot_matches_header():
    """STEP_SNAPSHOT and the SC_* word indices (sitewhere_amd/models/columnar.py) against
    SwStepSnapshot and the SW_SC_* enum: same names, offsets, sizes and values."""
    from sitewhere_amd.models import columnar as col
    text = re.sub(r"//[^\n]*", "", HEADER.read_text())
    enum, nxt = {}, 0
    for item in re.search(r"enum \{\s*(SW_SC_N_RECS.*?)\};", text, re.S).group(1).split(","):
        if item.strip():
            m = re.fullmatch(r"(SW_SC_\w+)(?:\s*=\s*(\d+))?", item.strip())
            assert m, f"unparsed enumerator: {item!r}"
            nxt = int(m.group(2)) if m.group(2) else nxt
            enum[m.group(1)] = nxt
            nxt += 1
    words = enum.pop("SW_SC_WORDS")
    assert words == col.SC_WORDS == 16
    assert enum == {"SW_" + k: getattr(col, k) for k in dir(col) if k.startswith("SC_N_") or k == "SC_OVERFLOW"}
    assert [k[6:].lower() for k in sorted(enum, key=enum.get)] == list(col.SC_NAMES)
    assert sorted(enum.values()) == list(range(len(col.SC_NAMES)))
    body = re.search(r"typedef struct SwStepSnapshot \{(.*?)\} SwStepSnapshot;", text, re.S).group(1)
    fields, off = [], 0
    for decl in body.split(";"):
        if not decl.strip():
            continue
        ctype, names = decl.split(None, 1)
        size = {"uint32_t": 4, "uint64_t": 8}[ctype]
        for name in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", name.strip())
            assert m, f"unparsed declaration in SwStepSnapshot: {decl!r}"
            n = 1 if m.group(2) is None else words if m.group(2) == "SW_SC_WORDS" else int(m.group(2))
            off = -(-off // size) * size
            fields.append((m.group(1), off, size, n))
            off += size * n
    dt = col.STEP_SNAPSHOT
    got = [(k, dt.fields[k][1], dt.fields[k][0].base.itemsize, int(np.prod(dt.fields[k][0].shape, dtype=int)))
           for k in dt.names]
    assert got == fields
    assert dt.itemsize == off == 128


def test_ring_view_heads_the_hot_store_queries():
    """RING_QUERY against SwRingView, field by field, and as the head of the two query word lists."""
    from sitewhere_amd.models.columnar import NEAR_QUERY, RING_QUERY, SERIES_QUERY
    text = re.sub(r"//[^\n]*", "", HEADER.read_text())
    body = re.search(r"typedef struct SwRingView \{(.*?)\} SwRingView;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)", decl.strip())
            assert m, f"unparsed declaration in SwRingView: {decl!r}"
            assert m.group(2) or m.group(1) == "int64_t"           # every field 8 bytes
            fields += [f.strip() for f in m.group(3).split(",")]
    assert tuple(fields) == RING_QUERY
    assert "static_assert(sizeof(SwRingView) == %d" % (8 * len(RING_QUERY)) in text
    for words, name, size in ((SERIES_QUERY, "SwSeriesQuery", 144), (NEAR_QUERY, "SwNearQuery", 176)):
        assert words[:len(RING_QUERY)] == RING_QUERY and len(set(words)) == len(words)
        # the view is the first member, of the query or of the position view that is the query's first
        first = re.search(r"typedef struct %s \{\s*(\w+) \w+;" % name, text).group(1)
        assert first == ("SwPositionView" if name == "SwNearQuery" else "SwRingView")
        assert re.search(r"typedef struct SwPositionView \{\s*SwRingView \w+;", text)
        assert 8 * len(words) == size and "static_assert(sizeof(%s) == %d" % (name, size) in text
