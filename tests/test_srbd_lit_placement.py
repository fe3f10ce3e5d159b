"""The placement order of the one-wave literal kernel on the host
(qloco_srbd_place_order_host: the ordering kernel's own functions,
quadrupedal_loco_amd/csrc/qloco_srbd_place.hpp), and the CPU
model of what the placement is worth (tools/lit_placement_model.py).  CPU only.

Everything here is integer arithmetic, so every check is exact."""
import os
import sys

import numpy as np
import pytest

from quadrupedal_loco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
SIMDS = [1, 8, 1024]
CHECK = 25  # OSQP's check_termination default: one class per check


def _batches(S):
    """S + 1, 2 S - 1, 2 S, 3 S + 5, 4 S where they are placed batches
    (S < B <= 4 S: at S = 1 that leaves 2 and 4)."""
    return sorted(b for b in {S + 1, 2 * S - 1, 2 * S, 3 * S + 5, 4 * S} if S < b <= 4 * S)


def _hints(kind, B):
    rng = np.random.default_rng(B)
    if kind == "constant":
        return np.full(B, 75, np.int32)
    if kind == "random":
        return (CHECK * rng.integers(1, 17, B)).astype(np.int32)
    if kind == "negative":
        return rng.integers(-INT_MAX, 0, B).astype(np.int32)
    if kind == "int_max":
        h = np.full(B, INT_MAX, np.int32)
        h[::3] = rng.integers(-5, 400, len(h[::3]))
        return h
    if kind == "garbage":
        return rng.integers(-INT_MAX - 1, INT_MAX, B, dtype=np.int64).astype(np.int32)
    raise ValueError(kind)


def _order(B, S, hint, check=CHECK):
    order = np.full(B, -7, np.int32)
    rc = _lib.lib().qloco_srbd_place_order_host(B, S, check, _lib.ptr(hint), _lib.ptr(order))
    assert rc == 0, rc
    return order


def _class(hint, check=CHECK):
    # C division truncates toward zero; negative counts fall into class 0 either way
    return np.clip(np.maximum(hint.astype(np.int64), 0) // max(check, 1), 0, 255)


def _rank_of_position(B, S):
    """The issue's rank map, restated: position p = s + S q -> rank."""
    T = B - S
    m = -(-T // S)
    r = T - (m - 1) * S
    p = np.arange(B)
    s, q = p % S, p // S
    return np.where(q == 0, s, B - 1 - (s * (m - 1) + np.minimum(s, r) + (q - 1)))


@pytest.mark.parametrize("S", SIMDS)
def test_rank_map_is_a_bijection(S):
    for B in _batches(S):
        rank = _rank_of_position(B, S)
        assert np.array_equal(np.sort(rank), np.arange(B)), (S, B)


@pytest.mark.parametrize("kind", ["constant", "random", "negative", "int_max", "garbage"])
@pytest.mark.parametrize("S", SIMDS)
def test_order_is_a_permutation_sorted_by_class(S, kind):
    for B in _batches(S):
        hint = _hints(kind, B)
        order = _order(B, S, hint)
        assert np.array_equal(np.sort(order), np.arange(B)), (S, B, kind)
        # the instance of rank k: classes never increase along the ranks
        by_rank = np.empty(B, np.int64)
        by_rank[_rank_of_position(B, S)] = order
        cls = _class(hint)[by_rank]
        assert np.all(np.diff(cls) <= 0), (S, B, kind)


@pytest.mark.parametrize("S", SIMDS)
def test_full_batch_puts_the_three_shortest_with_each_head(S):
    """B = 4 S: the block at position s + S q (q >= 1) holds rank
    B - 1 - 3 s - (q - 1), position s rank s.  With counts that fall along the
    index, instance i has rank i (the host sort keeps the index order inside a
    class), so order[] is the rank map itself."""
    B = 4 * S
    hint = np.arange(B, 0, -1).astype(np.int32)
    order = _order(B, S, hint)
    s, q = np.arange(B) % S, np.arange(B) // S
    want = np.where(q == 0, s, B - 1 - 3 * s - (q - 1))
    assert np.array_equal(order, want)
    assert np.array_equal(_rank_of_position(B, S), want)


def test_order_host_refuses_batches_outside_the_placed_range():
    L = _lib.lib()
    h = np.zeros(64, np.int32)
    o = np.zeros(64, np.int32)
    for B, S in ((8, 8), (4, 8), (33, 8), (8, 0)):
        assert L.qloco_srbd_place_order_host(B, S, CHECK, _lib.ptr(h), _lib.ptr(o)) != 0, (B, S)
    assert L.qloco_srbd_place_order_host(9, 8, CHECK, None, _lib.ptr(o)) != 0
    assert L.qloco_srbd_place_bytes(4096) == 4 * (4 + 2 * 4096)
    assert L.qloco_srbd_place_bytes(0) == 16


def test_model_tool_reproduces_the_headline_figures():
    """tools/lit_placement_model.py on the headline batch's oracle counts: the
    given order models 323 us of iterations on the most loaded SIMD, the
    placement with exact counts 222 us (round times 0.557 / 0.804 / 1.14 /
    1.477 us for one to four live waves, profiles/lit_iter_ab.txt; figures
    rounded to the microsecond as the tool prints them)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lit_placement_model as M
    finally:
        sys.path.pop(0)
    counts = M.headline_counts()
    assert counts.shape == (4096,)
    S = 1024
    given = M.simd_max_us(counts, np.arange(4096), S)
    placed = M.simd_max_us(counts, M.placement_order(counts, S), S)
    assert round(given) == 323, given
    assert round(placed) == 222, placed
    # plain iteration sums of the most loaded SIMD
    assert M.simd_max_sum(counts, np.arange(4096), S) == 800
    assert M.simd_max_sum(counts, M.placement_order(counts, S), S) <= 600
