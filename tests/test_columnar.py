"""The ctypes mirror of the engine's argument block (sitewhere_amd/ops/engine_abi.py) against the
struct it mirrors (csrc/include/swengine.h): the same fields, of the same kind, in the same order.
The size alone (tests/test_gpu_engine.py test_abi_sizes_match) cannot tell two swapped fields apart."""
from __future__ import annotations

import ctypes
import re
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
