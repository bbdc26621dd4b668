"""The alternate-id dedup where probes chain (``dedup_scenarios``), Python oracle against the native
engine: a full filter bucket sends an id on, the last bucket's chain wraps to bucket 0, 2 / 3 / 5 / 8
generations, many copies of one id in a batch (the lowest index is the first occurrence), and window
chains that wrap the table end.  Each test compares the two engines event for event and asserts what
its scenario is for; ``tests/test_gpu_dedup.py`` runs the same scenarios on the MI355X engine."""
import functools

import pytest

from sitewhere_amd.pipeline.cpu_engine import CpuInboundEngine
from sitewhere_amd.pipeline.native_engine import NativeCpuEngine

import dedup_scenarios as S

ENGINES = (CpuInboundEngine, NativeCpuEngine)


@functools.lru_cache(maxsize=None)
def run(story, cls, gens):
    make_cfg = S.small_window_cfg if story == "window_wrap_story" else S.cfg
    return getattr(S, story)(S.make_engine(cls, make_cfg(gens)))


def both(story, gens):
    return [run(story, cls, gens) for cls in ENGINES]


# ------------------------------------------------------------------ oracle against native engine
def test_crafted_id_sets():
    for gens in S.GENS:
        S.check_config(S.cfg(gens))
    S.check_config(S.cfg(0))
    S.check_id_sets(S.cfg(S.GENS[0]))


@pytest.mark.parametrize("gens", S.GENS)
def test_chain_add_fills_last_first_and_second_bucket(gens):
    c = S.cfg(gens)
    oracle, native = both("chain_story", gens)
    S.check_chain_add(c, native, oracle)
    S.check_chain_add(c, oracle, oracle)


@pytest.mark.parametrize("gens", S.GENS)
def test_chain_ids_are_rechecked_controls_persist(gens):
    oracle, native = both("chain_story", gens)
    S.check_chain_probe(S.cfg(gens), native, oracle)
    S.check_chain_probe(S.cfg(gens), oracle, oracle)


@pytest.mark.parametrize("gens", S.GENS)
def test_chain_probe_with_in_batch_repeats(gens):
    c = S.cfg(gens)
    oracle, native = both("repeat_story", gens)
    ref = S.seeded_reference(c)
    S.check_repeats(c, native, oracle, ref)
    S.check_repeats(c, oracle, oracle, ref)


@pytest.mark.parametrize("gens", (0,) + S.GENS)
def test_first_occurrence_is_the_lowest_index(gens):
    oracle, native = both("first_occurrence_story", gens)
    S.check_first_occurrence(S.cfg(gens), native, oracle)
    S.check_first_occurrence(S.cfg(gens), oracle, oracle)


@pytest.mark.parametrize("gens", (0,) + S.GENS)
def test_window_chain_wraps_the_table_end(gens):
    c = S.small_window_cfg(gens)
    oracle, native = both("window_wrap_story", gens)
    S.check_window_wrap(c, native, oracle)
    S.check_window_wrap(c, oracle, oracle)
