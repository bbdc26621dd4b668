"""Columnar / fixed-width record layouts shared by the host runtime and the gfx950 kernels.

These numpy dtypes mirror the C structs in ``csrc/include/swtypes.h`` and
``csrc/include/swengine.h`` byte for byte (``tests/test_columnar.py`` checks
them against ``sw_abi_sizes`` and field offsets).
"""
from __future__ import annotations

import numpy as np

# Event types (GDeviceEventType in the reference's device-event-model.proto).
EV_MEASUREMENT = 0
EV_LOCATION = 1
EV_ALERT = 2
EV_COMMAND_INVOCATION = 3
EV_COMMAND_RESPONSE = 4
EV_STATE_CHANGE = 5
EV_REGISTRATION = 16
EV_ACK = 17
EV_STREAM_CREATE = 18
EV_STREAM_DATA = 19
EV_STREAM_DATA_REQUEST = 20
EV_DECODE_ERROR = 255

# Validation status (InboundPayloadProcessingLogic outcomes).
ST_OK = 0
ST_UNREGISTERED = 1
ST_UNASSIGNED = 2
ST_DUPLICATE = 3
ST_DECODE_ERROR = 4
ST_CONTROL = 5
ST_RECHECK = 6          # id new to the dedup window, maybe stored before: host checks the store

F_HAS_UPDATE_STATE = 0x1
F_UPDATE_STATE = 0x2
F_HAS_DATE = 0x4
F_HAS_ELEVATION = 0x8
F_SETTLED = 0x40       # store-backed dedup settled on the host: the filter skips the record

EVENT_REC = np.dtype([
    ("fp_lo", "<u8"), ("fp_hi", "<u8"), ("event_date", "<i8"), ("name_hash", "<u8"),
    ("v0", "<f8"), ("v1", "<f8"), ("v2", "<f8"), ("alt_hash", "<u8"),
    ("aux_off", "<u4"), ("aux2_off", "<u4"), ("aux_len", "<u2"), ("aux2_len", "<u2"),
    ("etype", "u1"), ("flags", "u1"), ("src_rank", "u1"), ("level", "u1"),
], align=True)
assert EVENT_REC.itemsize == 80

# String refs of a decoded event (SwStrRef, csrc/include/swtypes.h): where its alternate id and
# metadata span sit in the raw batch, and its measurement index (alternate id "<alt>:<k>").
STR_REF = np.dtype([("alt_off", "<u4"), ("meta_off", "<u4"), ("alt_len", "<u2"), ("meta_len", "<u2"),
                    ("k", "<u2"), ("has", "u1"), ("pad", "u1")], align=True)
assert STR_REF.itemsize == 16
SR_ALT, SR_META, SR_MULTI = 0x1, 0x2, 0x4
EV_OVERSIZE = 21

# Exchange form (SwWireRec, csrc/include/swtypes.h): lossless 64-byte packing of EVENT_REC.
WIRE_REC = np.dtype([
    ("fp_lo", "<u8"), ("fp_hi", "<u8"), ("event_date", "<i8"), ("w0", "<u8"), ("w1", "<u8"), ("w2", "<u8"),
    ("alt_hash", "<u8"), ("aux_off", "<u4"), ("aux_len", "<u2"), ("etype", "u1"), ("flags", "u1"),
], align=True)
assert WIRE_REC.itemsize == 64


def wire_pack(r: np.ndarray) -> np.ndarray:
    """EVENT_REC -> WIRE_REC (same rule as ``sw_wire_pack``)."""
    w = np.zeros(len(r), WIRE_REC)
    for k in ("fp_lo", "fp_hi", "event_date", "alt_hash", "aux_off", "aux_len", "etype", "flags"):
        w[k] = r[k]
    loc = r["etype"] == 1
    val = (r["etype"] == 0) | loc
    w["w0"] = np.where(loc, r["v2"].view(np.uint64), r["name_hash"])
    aux2 = (r["aux2_off"].astype(np.uint64) | (r["aux2_len"].astype(np.uint64) << np.uint64(32)) |
            (r["level"].astype(np.uint64) << np.uint64(48)))
    w["w1"] = np.where(val, r["v0"].view(np.uint64), aux2)
    w["w2"] = r["v1"].view(np.uint64)
    return w


def wire_unpack(w: np.ndarray, src_rank: int) -> np.ndarray:
    """WIRE_REC -> EVENT_REC (``sw_wire_unpack``); ``src_rank`` = the slab the records came from."""
    r = np.zeros(len(w), EVENT_REC)
    for k in ("fp_lo", "fp_hi", "event_date", "alt_hash", "aux_off", "aux_len", "etype", "flags"):
        r[k] = w[k]
    loc = w["etype"] == 1
    val = (w["etype"] == 0) | loc
    r["name_hash"] = np.where(loc, np.uint64(0), w["w0"])
    r["v2"] = np.where(loc, w["w0"], np.uint64(0)).view(np.float64)
    r["v0"] = np.where(val, w["w1"], np.uint64(0)).view(np.float64)
    r["v1"] = w["w2"].view(np.float64)
    aux = np.where(val, np.uint64(0), w["w1"])
    r["aux2_off"] = (aux & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    r["aux2_len"] = ((aux >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.uint16)
    r["level"] = ((aux >> np.uint64(48)) & np.uint64(0xFF)).astype(np.uint8)
    r["src_rank"] = src_rank
    return r


OUT_REC = np.dtype([
    ("event_date", "<i8"), ("v0", "<f8"), ("v1", "<f8"), ("assignment", "<i4"), ("name_id", "<u2"),
    ("etype", "u1"), ("level", "u1"),
])
OUT_REC_SIZE = 32
assert OUT_REC.itemsize == OUT_REC_SIZE
NO_NAME = 0xFFFF

NAME_REF = np.dtype([("hash", "<u8"), ("off", "<u4"), ("len", "<u2"), ("src_rank", "u1"), ("etype", "u1")])
assert NAME_REF.itemsize == 16

REG_SLOT = np.dtype([("lo", "<u8"), ("hi", "<u8"), ("dev", "<i4"), ("asg", "<i4"), ("pad", "<u8")])
assert REG_SLOT.itemsize == 32
ASG_STATE = np.dtype([("last", "<u8"), ("missing", "<u8"), ("loc_date", "<u8"), ("loc_eid1", "<u8")])
MS_SLOT = np.dtype([("key", "<u8"), ("date", "<u8"), ("eid1", "<u8"), ("pad", "<u8")])

ZONE_TEST = np.dtype([("zone", "<i4"), ("condition", "<i4"), ("alert_name_id", "<i4"), ("level", "<i4")])
MX_TEST = np.dtype([("name_hash", "<u8"), ("lo", "<f8"), ("hi", "<f8")])     # SwMxTest

# A step's u32 scalar words (SW_SC_* in swengine.h), in word order; SC_WORDS words are kept.
SC_NAMES = ("n_recs", "n_new_names", "overflow", "n_work", "n_ok", "n_rej", "n_gen", "n_out", "n_rule")
SC_N_RECS, SC_N_NEW_NAMES, SC_OVERFLOW, SC_N_WORK, SC_N_OK, SC_N_REJ, SC_N_GEN, SC_N_OUT, SC_N_RULE = range(9)
SC_WORDS = 16

# End-of-step snapshot the kernels write into mapped host memory (SwStepSnapshot in swengine.h).
STEP_SNAPSHOT = np.dtype([
    ("scalars", "<u4", (SC_WORDS,)), ("block_bytes", "<u8"), ("block_errors", "<u8"), ("block_first_seq", "<u8"),
    ("n_carry", "<u4", (2,)), ("rej_refs", "<u4"), ("rej_bytes", "<u4"), ("pad", "<u4", (6,)),
])
assert STEP_SNAPSHOT.itemsize == 128

# One (measurement name, time bucket) cell of a bucketed series (SwSeriesCell in swengine.h); an empty
# cell is all zero bytes.  first / last: the row with the smallest / largest (date, event id).
SERIES_CELL = np.dtype([
    ("count", "<i8"), ("sum", "<f8"), ("min", "<f8"), ("max", "<f8"), ("first", "<f8"), ("last", "<f8"),
    ("first_date", "<i8"), ("last_date", "<i8"), ("first_id", "<i8"), ("last_id", "<i8"),
])
assert SERIES_CELL.itemsize == 80
SERIES_MAX_NAMES = 64          # SW_SERIES_MAX_NAMES
SERIES_MAX_CELLS = 65536       # SW_SERIES_MAX_CELLS
# The int64 words of the ring view every hot-store query begins with (SwRingView in swengine.h), in order.
RING_QUERY = ("etype", "asg", "date", "n_rows", "seq0", "head", "bits", "n_asg", "start", "end")
# The int64 words of a series query (SwSeriesQuery in swengine.h), in order.
SERIES_QUERY = RING_QUERY + ("name", "v0", "names", "n_names", "bucket_ms", "n_buckets", "rounds", "grid")
# The 8-byte words of the position view the three location queries begin with (SwPositionView in
# swengine.h), in order: the ring view, the latitude and longitude columns, `latest` and its two tables.
POSITION_QUERY = RING_QUERY + ("v0", "v1", "latest", "best_date", "best_seq")
# The 8-byte words of a locations-near query (SwNearQuery in swengine.h), in order: the position view,
# then NEAR_WORDS, the query's own; NEAR_QUERY_F64 are the doubles among them (written by their bits).
NEAR_WORDS = ("lat", "lon", "radius_m", "lat_lo", "lat_hi", "lon_lo", "lon_hi")
NEAR_QUERY = POSITION_QUERY + NEAR_WORDS
NEAR_QUERY_F64 = ("lat", "lon", "radius_m", "lat_lo", "lat_hi", "lon_lo", "lon_hi")
# The 8-byte words of a locations-in-zone query (SwZoneQuery in swengine.h), in order; ZONE_QUERY_F64 are
# the doubles among them.
ZONE_WORDS = ("vtx", "n_vtx", "lat_lo", "lat_hi", "lon_lo", "lon_hi", "outside")
ZONE_QUERY = POSITION_QUERY + ZONE_WORDS
ZONE_QUERY_F64 = ("lat_lo", "lat_hi", "lon_lo", "lon_hi")
# One cell of a location density grid (SwGridCell in swengine.h): the locations in it and the newest of
# their dates; an empty cell is all zero bytes.
GRID_CELL = np.dtype([("count", "<i8"), ("last_date", "<i8")])
assert GRID_CELL.itemsize == 16
# The 8-byte words of a density-grid query (SwGridQuery in swengine.h), in order; GRID_QUERY_F64 are the
# doubles among them.  Its n_rows (the grid's rows) shares its name with the ring view's (the ring's rows):
# a query's own words are filled in apart from the view's.
GRID_WORDS = ("lat_lo", "lat_hi", "lon_lo", "lon_hi", "d_lat", "d_lon", "n_rows", "n_cols", "crossing")
GRID_QUERY = POSITION_QUERY + GRID_WORDS
GRID_QUERY_F64 = ("lat_lo", "lat_hi", "lon_lo", "lon_hi", "d_lat", "d_lon")
# One group of a ranking over the ring (SwRankCell in swengine.h): its key, its rows, min / max / last of
# their v0 (0.0 for a type that has no value) and the (date, event id) of its newest row.
RANK_CELL = np.dtype([("key", "<i8"), ("count", "<i8"), ("min", "<f8"), ("max", "<f8"), ("last", "<f8"),
                      ("last_date", "<i8"), ("last_id", "<i8")])
assert RANK_CELL.itemsize == 56
# The int64 words of a ranking query (SwRankQuery in swengine.h), in order.
RANK_QUERY = RING_QUERY + ("level", "name", "v0", "key", "event_type", "name_on", "name_hash", "min_level", "n_keys",
                           "stat")
RANK_MAX_KEYS = 1 << 22        # SW_RANK_MAX_KEYS

# Durable-block encoder state (u64 words): the result words follow the max_pages look-back words
# (SEG_ST_* in swseg.h) -- block bytes (~0 on error), errors, store sequence of the first row.
SEG_ST_BYTES, SEG_ST_ERRORS, SEG_ST_FIRST = 1, 2, 3
SEG_ST_WORDS = 8

# Stats slots (SW_STAT_* in swengine.h).
N_STATS = 24            # SW_N_STATS (csrc/include/swengine.h): slots of the stats arrays
STAT_NAMES = [
    "messages", "events", "persisted", "unregistered", "unassigned", "duplicates", "decode_errors",
    "control", "rule_alerts", "presence_events", "shuffle_overflow", "new_names", "state_overflow",
    "shuffle_deferred", "dedup_overflow", "dedup_rotations", "dedup_rechecks",
]

# Alert levels (GAlertLevel) and sources.
ALERT_LEVELS = ["Info", "Warning", "Error", "Critical"]

EVENT_TYPE_NAMES = {
    EV_MEASUREMENT: "Measurement", EV_LOCATION: "Location", EV_ALERT: "Alert",
    EV_COMMAND_INVOCATION: "CommandInvocation", EV_COMMAND_RESPONSE: "CommandResponse",
    EV_STATE_CHANGE: "StateChange",
}
