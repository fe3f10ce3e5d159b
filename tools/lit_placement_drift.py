#!/usr/bin/env python3
"""The placement state on changing inputs: a cold literal
solver over srbd.control_loop_sequence (drifting states, half the controllers
flipping their trot phase every switch_every / 2 ticks), placement on against
off, the two alternating pass by pass, every call between two HIP events (with
the state, the ordering kernel after the solve is inside the pair).

A pass starts from a zeroed state, so tick 0 runs in the given order and
tick t is ordered by the counts of tick t - 1.

    python tools/lit_placement_drift.py [--ticks 24] [--switch-every 6] [--batch 4096] [--passes 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261015


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=24)
    ap.add_argument("--switch-every", type=int, default=6)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args()
    import torch

    from quadrupedal_loco_amd import srbd
    N, B, K = 10, args.batch, args.switch_every
    dev = torch.device("cuda:0")
    seq = [[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in tick]
           for tick in srbd.control_loop_sequence(SEED, N, B, args.ticks, "trot", switch_every=K)]
    solvers = {"on": srbd.BatchedConvexMpc(horizon=N, literal_full_qp=1),
               "off": srbd.BatchedConvexMpc(horizon=N, literal_full_qp=1, placement=False)}
    out = solvers["on"].alloc_outputs(B, dev)
    stream = torch.cuda.current_stream(dev)
    for _ in range(60):  # past the clock ramp
        solvers["off"].solve(*seq[0], out=out, max_legs=4 * N)
    torch.cuda.synchronize()
    us = {m: np.zeros((args.passes, args.ticks)) for m in solvers}
    iters = np.zeros((args.ticks, B), np.int32)
    for p in range(args.passes):
        for m in (("on", "off") if p % 2 == 0 else ("off", "on")):
            s = solvers[m]
            if m == "on":
                s.place_state(B, dev, stream.cuda_stream).zero_()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(args.ticks)]
            for t, tick in enumerate(seq):
                ev[t][0].record(stream)
                s.solve(*tick, out=out, max_legs=4 * N)
                ev[t][1].record(stream)
                if p == 0 and m == "on":
                    iters[t] = out.iters.cpu().numpy()
            torch.cuda.synchronize()
            us[m][p] = [1e3 * a.elapsed_time(b) for a, b in ev]
    flips = [t for t in range(1, args.ticks)
             if (t // K) % 2 != ((t - 1) // K) % 2 or ((t + K // 2) // K) % 2 != ((t - 1 + K // 2) // K) % 2]
    med = {m: np.median(us[m], axis=0) for m in us}
    spread = {m: float((us[m].max(axis=0) - us[m].min(axis=0))[1:].mean()) for m in us}
    print("# tools/lit_placement_drift.py: N = %d trot, B = %d, %d ticks, switch_every = %d, %d passes; us per call"
          % (N, B, args.ticks, K, args.passes))
    print("# tick  flip   off (median)   on (median)   on - off   r(prev, this)   equal")
    for t in range(args.ticks):
        r = eq = float("nan")
        if t:
            r = float(np.corrcoef(iters[t - 1], iters[t])[0, 1])
            eq = float((iters[t - 1] == iters[t]).mean())
        print("  %4d  %4s  %12.1f  %12.1f  %9.1f  %14.3f  %6.2f" % (
            t, "flip" if t in flips else "", med["off"][t], med["on"][t], med["on"][t] - med["off"][t], r, eq))
    rest = [t for t in range(1, args.ticks) if t not in flips]
    for name, sel in (("all ticks but 0", list(range(1, args.ticks))), ("phase-flip ticks", flips),
                      ("other ticks", rest)):
        a, b = med["off"][sel].mean(), med["on"][sel].mean()
        print("# %-18s off %.1f us  on %.1f us  on - off %+.1f us (%+.1f %%)" % (name, a, b, b - a, 100 * (b - a) / a))
    print("# tick 0 (zero state: the given order plus the ordering kernel): off %.1f  on %.1f" % (
        med["off"][0], med["on"][0]))
    print("# mean max - min over the passes, per tick: off %.1f us  on %.1f us" % (spread["off"], spread["on"]))


if __name__ == "__main__":
    main()
