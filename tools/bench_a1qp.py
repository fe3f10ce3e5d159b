#!/usr/bin/env python
"""Throughput of the A1 single-step force QP (a1_qp_kernel behind
qloco_a1_qp_solve_body, include/qloco.h section 9) with and without per-robot
bodies.  Not the headline benchmark (bench.py); the record it feeds is
profiles/a1qp_body_rows_ab.txt.

  python tools/bench_a1qp.py --body none|same|mixed [--batch 65536] [--seed 2026]

  none   body = NULL: the instantiation without rows
  same   every row holds the params' values: the rows' own cost, at the
         iteration counts of `none`
  mixed  robot b holds body b % 10 of the ten-body mix of the tests (other
         iteration counts: for the record, not comparable)

Inputs are a1qp.synth_states(seed, batch).  Warm-up launches, then enough
timed launches for a window of at least --window seconds between two device
events, closed by a synchronise.  Prints one JSON line.  There is no host
path: without a GPU the tool fails.

--entry solve times qloco_a1_qp_solve (body none only): for a library built
before the rows existed, named by QLOCO_LIB, in parent-against-tree runs.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quadrupedal_loco_amd import _lib, a1qp  # noqa: E402

# the body-only cases of tests/a1qp_cases.py, in the order of tests/a1qp_body_cases.py
MIX = (
    {}, dict(f_min=20.0), dict(f_min=40.0, f_max=40.0), dict(mu=0.0), dict(mu=0.2), dict(f_max=40.0),
    dict(robot_mass=30.0, f_max=60.0),
    dict(kp_linear=(600.0, 800.0, 1500.0), kd_linear=(100.0, 140.0, 60.0), kp_angular=(300.0, 70.0, 5.0),
         kd_angular=(9.0, 2.0, 15.0)),
    dict(q_diag=(2.0, 0.5, 3.0, 100.0, 250.0, 40.0)), dict(r=1e-2),
)


def mixed_rows(B):
    ten = np.concatenate([a1qp.body_rows(1, **ov) for ov in MIX])
    return np.ascontiguousarray(ten[np.arange(B) % len(MIX)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--body", choices=("none", "same", "mixed"), default="none")
    ap.add_argument("--entry", choices=("solve_body", "solve"), default="solve_body")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least timed window, seconds")
    args = ap.parse_args()
    if args.entry == "solve" and args.body != "none":
        ap.error("--entry solve takes no rows")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_a1qp: no GPU; the A1 QP has no host path")
    dev = torch.device("cuda:0")
    B = args.batch
    S, CT = a1qp.synth_states(args.seed, B)
    s, c = torch.from_numpy(S).to(dev), torch.from_numpy(CT).to(dev)
    prm = a1qp.default_params()
    rows = None
    if args.body == "same":
        rows = torch.from_numpy(a1qp.body_rows(B, params=prm)).to(dev)
    elif args.body == "mixed":
        rows = torch.from_numpy(mixed_rows(B)).to(dev)
    forces = torch.empty((B, 12), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    head = (C.byref(prm), B, _lib.ptr(s), _lib.ptr(c), _lib.ptr(forces), None, _lib.ptr(status), _lib.ptr(iters),
            None, None)

    def launch():
        if args.entry == "solve":
            _lib.check(L.qloco_a1_qp_solve(*head, stream), "qloco_a1_qp_solve")
        else:
            _lib.check(L.qloco_a1_qp_solve_body(*head, _lib.ptr(rows), stream), "qloco_a1_qp_solve_body")

    def timed(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    n = max(3, int(np.ceil(1.2 * args.window / (timed(3) / 3))))
    t = timed(n)
    if t < args.window:                                # the estimate was short: once more, longer
        n = int(np.ceil(n * 1.5 * args.window / t))
        t = timed(n)
    st, it = status.cpu().numpy(), iters.cpu().numpy()
    print(json.dumps({
        "bench": "a1qp", "entry": args.entry, "body": args.body, "batch": B, "seed": args.seed,
        "launches": n, "window_s": round(t, 4), "us_per_launch": round(1e6 * t / n, 2),
        "robots_per_s": round(B * n / t, 1), "mean_iters": round(float(it.mean()), 3),
        "solved": int((st == 0).sum())}))


if __name__ == "__main__":
    main()
