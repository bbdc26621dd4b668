"""csrc/include/swengine.h as the layout tests read it: a struct's fields in order, with the structs it
holds by value (``SwRingView`` in every hot-store query, ``SwPositionView`` in the location queries)
expanded in place, so a query's fields are its 8-byte words."""
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "csrc" / "include" / "swengine.h"


def struct_fields(name):
    """(the header without its comments, [(field, "ptr" or its type)]) of ``typedef struct name``."""
    text = re.sub(r"//[^\n]*", "", HEADER.read_text())
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.+)", decl.strip(), re.S)
            assert m, f"unparsed declaration in {name}: {decl!r}"
            if m.group(1).startswith("Sw") and not m.group(2):     # a struct by value: its words stand here
                assert "," not in m.group(3)
                fields += struct_fields(m.group(1))[1]
                continue
            for f in m.group(3).split(","):
                fields.append((f.strip(), "ptr" if m.group(2) else m.group(1)))
    return text, fields
