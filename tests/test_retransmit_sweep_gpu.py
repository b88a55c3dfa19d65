"""The retransmission sweep (include/gpx_timers.h) on the GPU.  Every case applies one history to a HIP engine and to the
CPU oracle (tests/timers_common.py); the expected answer of a call is tests/timers_model.py fed with the ORACLE's dense
poke rows, bit for bit: counts, the ten columns, and the sentinel from the last written entry on - both forms write into
sentinel-filled buffers with padding behind cap.  The timer words are compared through the call's outputs over successive
sweeps: which waits are due, after how long and for the how-manyth time.  tests/test_retransmit_sweep_model.py runs the
same histories on the oracle alone and shows that each has hits, waiting entries that are not hits and, where it claims
one, a key that changed between two sweeps."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import timers_common as TC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [pytest.param("edges", marks=pytest.mark.gpu_fast), "hole", "all", "none"])
def test_hits_by_construction(hip_lib, oracle_lib, name):
    TC.hits_by_construction(hip_lib, oracle_lib, name)


def test_six_sweeps_of_backoff(hip_lib, oracle_lib):
    TC.six_sweeps_of_backoff(hip_lib, oracle_lib)


def test_prepare_kind_election_and_preemption(hip_lib, oracle_lib):
    stats = TC.prepare_kind(hip_lib, oracle_lib)
    assert stats["rekeyed"] > 0


def test_count_saturates_at_255(hip_lib, oracle_lib):
    TC.saturation(hip_lib, oracle_lib)


def test_clock_wrap(hip_lib, oracle_lib):
    TC.clock_wrap(hip_lib, oracle_lib)


def test_cap_cuts_and_counts_only(hip_lib, oracle_lib):
    TC.cap_cuts(hip_lib, oracle_lib)


def test_peek_twice_then_the_real_sweep(hip_lib, oracle_lib):
    TC.peek_twice(hip_lib, oracle_lib)


def test_listed_sweep_with_dead_rows_and_entries_out_of_range(hip_lib, oracle_lib):
    TC.listed_sweep(hip_lib, oracle_lib)


@pytest.mark.parametrize("kmax,k,window", [(3, 3, 4), (3, 3, 64), (16, 16, 8), (3, 1, 8)])
def test_windows_and_group_sizes(hip_lib, oracle_lib, kmax, k, window):
    TC.shapes(hip_lib, oracle_lib, kmax, k, window)


def test_130561_groups_one_due_in_a_thousand(hip_lib, oracle_lib):
    """also: which kernels ran, from the engine's profile - no k_rtx_move under cap == 0"""
    TC.many_tiles(hip_lib, oracle_lib, 130561)


@pytest.mark.skipif(os.environ.get("GPX_FULL_MATRIX") != "1", reason="the untrimmed matrix: GPX_FULL_MATRIX=1")
def test_a_million_groups_one_due_in_a_thousand(hip_lib, oracle_lib):
    TC.many_tiles(hip_lib, oracle_lib, (1 << 20) + 1)


def test_host_twin_on_pageable_and_allocated_memory(hip_lib, oracle_lib):
    TC.host_twin(hip_lib, oracle_lib)


def test_lost_accepts_end_to_end(hip_lib, oracle_lib):
    TC.end_to_end(hip_lib, oracle_lib)


def test_capacity_limit_and_a_sweep_after_a_refusal(hip_lib):
    from gigapaxos_amd import timers

    eh = TC.engine(hip_lib, 100)
    counts = timers.RtxCounts()
    cfg = timers.make_cfg([0])
    n_max = max(int(eh.cfg.max_groups), int(eh.cfg.max_batch))
    assert eh.lib.fn["retransmit_sweep"](eh.h, n_max + 1, None, 0, C.byref(cfg), 0, 0, *[None] * 10, C.byref(counts)) == -2
    TC.propose(eh, np.arange(100, dtype=np.int32))
    cols, counts = timers.retransmit_sweep(eh, 5, cfg)
    assert (counts.n_hits, counts.n_nogroup, counts.n_waiting, counts.n_fired) == (0, 0, 100, 0)
    cols, counts = timers.retransmit_sweep(eh, 6, cfg)
    assert cols[0].tolist() == list(range(100)) and counts.n_fired == 100 and set(cols[9].tolist()) == {1}
    eh.close()
