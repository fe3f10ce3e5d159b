"""The rank a workgroup of the one-wave literal kernel takes
(place_assign, quadrupedal_loco_amd/csrc/qloco_srbd_place.hpp, through
qloco_srbd_place_assign_host), and what the CPU time model
(tools/lit_placement_model.py) gives for it.  CPU only.

The map is integer arithmetic, so those checks are exact.  Every bound on a
modelled time is the figure of the placement map before it (place_rank: what
order[] alone gave), computed here on the same counts; the new figures are
recorded in profiles/lit_assignment_model.txt, not here."""
import functools
import os
import sys

import numpy as np
import pytest

from quadrupedal_loco_amd import _lib, srbd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMDS = [1, 8, 1024]


def _batches(S):
    return sorted(b for b in {S + 1, 2 * S - 1, 2 * S, 3 * S + 5, 4 * S} if S < b <= 4 * S)


def _assign(B, S):
    rank = np.full(B, -7, np.int32)
    rc = _lib.lib().qloco_srbd_place_assign_host(B, S, _lib.ptr(rank))
    assert rc == 0, rc
    return rank


def _model():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lit_placement_model as M
    finally:
        sys.path.pop(0)
    return M


@pytest.mark.parametrize("S", SIMDS)
def test_assignment_is_a_bijection(S):
    for B in _batches(S):
        assert np.array_equal(np.sort(_assign(B, S)), np.arange(B)), (S, B)


def test_assignment_is_a_bijection_for_every_small_shape():
    """Every S <= 40 with every placed batch: the zone limits S / 64 and
    3 S / 16 round to 0, to each other and to distinct values in this range."""
    for S in range(1, 41):
        for B in range(S + 1, 4 * S + 1):
            assert np.array_equal(np.sort(_assign(B, S)), np.arange(B)), (S, B)


@pytest.mark.parametrize("S", SIMDS)
def test_first_row_keeps_the_longest_one_per_simd(S):
    """Position s < S takes rank s: each SIMD's first workgroup is one of the
    S longest, and they stay one per SIMD."""
    for B in _batches(S):
        assert np.array_equal(_assign(B, S)[:S], np.arange(S)), (S, B)


def test_one_companion_row_is_the_placement_map():
    """B <= 2 S: at most one companion per SIMD, nothing to deal again."""
    M = _model()
    for S in SIMDS:
        for B in (b for b in _batches(S) if b <= 2 * S):
            assert np.array_equal(_assign(B, S), M.place_rank(B, S)), (S, B)


def test_assign_host_refuses_batches_outside_the_placed_range():
    L = _lib.lib()
    o = np.zeros(64, np.int32)
    for B, S in ((8, 8), (4, 8), (33, 8), (8, 0), (8, -1), ((1 << 30) + 1, 1 << 30)):
        assert L.qloco_srbd_place_assign_host(B, S, _lib.ptr(o)) != 0, (B, S)
    assert L.qloco_srbd_place_assign_host(9, 8, None) != 0
    assert not o.any()


@functools.lru_cache(maxsize=None)
def _counts(which):
    M = _model()
    if which == "headline":
        c = M.headline_counts()
    elif which == "hardware":
        c = M.headline_counts(weights="hardware")
    else:  # ticks 0 and 1 of the drifting control loop
        seq = srbd.control_loop_sequence(M.SEED, 10, 4096, 2, "trot", switch_every=6)
        c = np.stack([M.oracle_counts(*tick, 10) for tick in seq])
    c.setflags(write=False)
    return c


def test_headline_span_is_below_the_placement_maps():
    M = _model()
    S, c = 1024, _counts("headline")
    old = M.simd_max_us(c, M.placement_order(c, S), S)
    new = M.simd_max_us(c, M.assigned_order(c, S), S)
    print("headline: placement map %.1f us, assigned %.1f us" % (old, new))
    assert round(old) == 222, old  # the figure tests/test_srbd_lit_placement.py pins
    assert new < old, (new, old)


def test_hardware_weights_span_is_not_above_the_placement_maps():
    M = _model()
    S, c = 1024, _counts("hardware")
    old = M.simd_max_us(c, M.placement_order(c, S), S)
    new = M.simd_max_us(c, M.assigned_order(c, S), S)
    print("hardware weights: placement map %.1f us, assigned %.1f us" % (old, new))
    assert new <= old, (new, old)


def test_drift_tick_span_is_not_above_the_placement_maps():
    """Tick 1 ordered by tick 0's counts: what the state holds when the inputs
    change between calls."""
    M = _model()
    S = 1024
    prev, c = _counts("drift")
    old = M.simd_max_us(c, M.placement_order(prev, S), S)
    new = M.simd_max_us(c, M.assigned_order(prev, S), S)
    print("drift tick 1 by tick 0: placement map %.1f us, assigned %.1f us" % (old, new))
    assert new <= old, (new, old)
