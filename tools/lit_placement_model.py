#!/usr/bin/env python3
"""CPU model of the one-wave literal kernel's SIMD placement.

A launch of B = 4 S one-wave workgroups is resident at once, workgroup p on
SIMD p mod S, and ends with its most loaded SIMD.  This tool takes the
iteration counts of the oracle's float64 restatement of the same OSQP calls
(qo_srbd_batch; equal to the kernel's on > 99 % of instances, §3k) and models
the iteration phase of every SIMD under these orders:

  given     workgroup p solves instance p
  snake     sorted by count, dealt to the SIMDs boustrophedon
  exact     the placement map (place_rank, qloco_srbd_place.hpp) on the counts
            of this very call
  previous  the same map on the counts of the call before (what the
            placement state holds when the inputs change between calls)
  assigned  the solve kernel's choice of rank (place_assign) on
            the counts of this very call, and `assigned prev` on those of the
            call before

over the headline batch, the reference's gazebo and hardware weight sets, the
first 3 S + 5 instances of the headline batch (a partial last row) and a
drifting control-loop sequence (srbd.control_loop_sequence, every tick solved
cold).

Time model of a SIMD with sorted counts c1 <= c2 <= c3 <= c4: a round of
iterations takes ROUND_US[k] with k live waves (profiles/lit_iter_ab.txt, this
tree at B = 1024 / 2048 / 4096; the three-wave figure is interpolated, not
measured), so T = 1.477 c1 + 1.14 (c2 - c1) + 0.804 (c3 - c2) + 0.557 (c4 - c3).

  python tools/lit_placement_model.py [--ticks 4] > profiles/lit_assignment_model.txt
(profiles/lit_placement_model.txt: the output before the assigned columns)
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 20261015  # bench.py's
ROUND_US = {1: 0.557, 2: 0.804, 3: 1.14, 4: 1.477}
CHECK = 25


def oracle_counts(x0, xr, ft, ct, N, weights=None):
    """Iteration counts of the float64 restatement of the literal OSQP call
    (weights: a (q_weights, r_weights) pair, default the Go1 set)."""
    import oracle_lib as O
    B = len(x0)
    kw = {} if weights is None else dict(q_w=weights[0], r_w=weights[1])
    sp, st = O.srbd_spec(N=N, **kw), O.admm_settings()
    iters = np.zeros(B, np.int32)
    secs = C.c_double(0)
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    rc = O.lib().qo_srbd_batch(C.byref(sp), C.byref(st), 0, B, O.P(x0, C.c_float), O.P(xr, C.c_float),
                               O.P(ft, C.c_float), 0, O.P(ct, C.c_uint8), 1, None,
                               O.P(iters, C.c_int), None, None, threads, C.byref(secs))
    assert rc == 0, rc
    return iters


def headline_counts(N=10, B=4096, weights=None):
    from quadrupedal_loco_amd import srbd
    if weights is not None:
        weights = srbd.REFERENCE_WEIGHTS[weights]
    return oracle_counts(*srbd.generate(SEED, N, B, "trot"), N, weights)


def placement_order(hint, S, check=CHECK):
    """order[p] = instance at workgroup position p (qloco_srbd_place_order_host)."""
    from quadrupedal_loco_amd import _lib
    hint = np.ascontiguousarray(hint, np.int32)
    order = np.zeros(len(hint), np.int32)
    rc = _lib.lib().qloco_srbd_place_order_host(len(hint), S, check, _lib.ptr(hint), _lib.ptr(order))
    assert rc == 0, rc
    return order


def place_rank(B, S):
    """rank[p] of the placement map (place_rank, qloco_srbd_place.hpp):
    order[p] is the instance of rank rank[p]."""
    T = B - S
    m = -(-T // S)
    r = T - (m - 1) * S
    p = np.arange(B)
    s, q = p % S, p // S
    return np.where(q == 0, s, B - 1 - (s * (m - 1) + np.minimum(s, r) + (q - 1)))


def assigned_rank(B, S):
    """rank[p] that workgroup p solves (qloco_srbd_place_assign_host)."""
    from quadrupedal_loco_amd import _lib
    rank = np.zeros(B, np.int32)
    rc = _lib.lib().qloco_srbd_place_assign_host(B, S, _lib.ptr(rank))
    assert rc == 0, rc
    return rank


def assigned_order(hint, S, check=CHECK):
    """The instance workgroup p solves: placement_order's instance of rank
    assigned_rank[p]."""
    order = placement_order(hint, S, check)
    by_rank = np.empty(len(order), np.int64)
    by_rank[place_rank(len(order), S)] = order
    return by_rank[assigned_rank(len(order), S)]


def snake_order(counts, S):
    by_len = np.argsort(-counts.astype(np.int64), kind="stable")
    order = np.empty(len(counts), np.int64)
    for q in range(-(-len(counts) // S)):
        row = by_len[q * S:(q + 1) * S]
        cols = np.arange(len(row)) if q % 2 == 0 else S - 1 - np.arange(len(row))
        order[q * S + cols] = row
    return order


def _per_simd(counts, order, S):
    """(S, 4) counts per SIMD, sorted ascending, for a batch S < B <= 4 S
    (position p on SIMD p mod S; a wave slot left empty counts zero)."""
    assert S < len(order) <= 4 * S
    slots = np.zeros(4 * S)
    slots[:len(order)] = counts[np.asarray(order)]
    return np.sort(slots.reshape(4, S).T, axis=1)


def simd_us(counts, order, S):
    c = _per_simd(counts, order, S)
    return (ROUND_US[4] * c[:, 0] + ROUND_US[3] * (c[:, 1] - c[:, 0]) +
            ROUND_US[2] * (c[:, 2] - c[:, 1]) + ROUND_US[1] * (c[:, 3] - c[:, 2]))


def simd_max_us(counts, order, S):
    return float(simd_us(counts, order, S).max())


def simd_max_sum(counts, order, S):
    return int(_per_simd(counts, order, S).sum(axis=1).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=4, help="ticks of the drift sequence (switch_every = 6: "
                    "half the controllers flip phase at tick 3)")
    ap.add_argument("--batch", type=int, default=4096)
    args = ap.parse_args()
    from quadrupedal_loco_amd import srbd
    N, B = 10, args.batch
    S = B // 4
    names = ("given", "snake", "exact", "previous", "assigned", "assigned prev")
    print("# tools/lit_placement_model.py: modelled iteration phase of the most loaded SIMD, us (largest per-SIMD")
    print("# iteration sum in brackets); N = %d trot, S = %d, round times %s us" % (N, S, ROUND_US))
    print("# %-34s" % "inputs" + "".join(" %14s" % n for n in names))

    def row(name, counts, prev):
        n = len(counts)
        ident = np.arange(n)
        cols = [ident, snake_order(counts, S) if n == 4 * S else None, placement_order(counts, S),
                None if prev is None else placement_order(prev, S), assigned_order(counts, S),
                None if prev is None else assigned_order(prev, S)]
        cells = ["%14s" % "-" if o is None else "%7.1f [%4d]" % (simd_max_us(counts, o, S), simd_max_sum(counts, o, S))
                 for o in cols]
        print("  %-34s" % name + "".join(" %14s" % c for c in cells))

    head = headline_counts(N, B)
    print("# headline counts (B = %d): mean %.1f, max %d, mean SIMD sum %.0f" % (
        B, head.mean(), head.max(), 4 * head.mean()))
    row("headline batch", head, None)
    for w in ("gazebo", "hardware"):
        row("%s weights" % w, headline_counts(N, B, w), None)
    row("headline's first 3 S + 5 = %d" % (3 * S + 5), head[:3 * S + 5], None)
    seq = srbd.control_loop_sequence(SEED, N, B, args.ticks, "trot", switch_every=6)
    prev = None
    for t, tick in enumerate(seq):
        c = oracle_counts(*tick, N)
        extra = ""
        if prev is not None:
            extra = " r=%.3f eq=%.0f%%" % (np.corrcoef(prev, c)[0, 1], 100.0 * (prev == c).mean())
        row("drift tick %d%s" % (t, extra), c, prev)
        prev = c


if __name__ == "__main__":
    main()
