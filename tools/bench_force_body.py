#!/usr/bin/env python
"""Throughput of the Go1 force QP (qloco_force_qp_solve_body, include/qloco.h
section 3) and of the Go1 servo tick (qloco_go1_servo_tick_body, section 16)
with and without per-robot bodies.  Not the headline benchmark (bench.py); the
record it writes is profiles/force_body_rows_ab.txt.

One measurement, one JSON line:

  python tools/bench_force_body.py --what qp|tick --body none|same|mixed
         [--entry body|plain] [--batch 65536] [--window 0.4]

  none   body = NULL: the kernels without rows
  same   every row holds the params' values: the rows' own cost, at the
         iteration counts of `none`
  mixed  robot b holds body b % 8 of the eight-body mix of the tests, masses
         and momenta included (other iteration counts: for the record)

  qp     the grouped launch, B robots of tests/cases.force_inputs, member and
         grouping state carried; timed twice in the process: `changing` (eight
         input sets cycled, as a servo tick sees them) and `repeated` (one set,
         so the previous iteration count predicts the next exactly)
  tick   the gait branch of the servo tick, the inputs of go1servo.synth_inputs
         for 256 robots tiled over the batch, windows of 16 ticks from one saved
         state record (as tools/bench_go1_servo.py)

--entry plain calls qloco_force_qp_solve_ordered / qloco_go1_servo_tick (body
none only): for a library built before the rows existed, named by QLOCO_LIB.

The whole A/B, one fresh process per measurement, one at a time, alternating
parent / none / same / mixed, six rounds:

  python tools/bench_force_body.py --ab --parent-lib PATH [--rounds 6] [--out profiles/force_body_rows_ab.txt]

There is no host path: without a GPU the tool fails.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# the bodies of tests/force_body_cases.py (overrides of the defaults) and its servo masses
MIX = ({}, dict(mu=0.5, gamma=100.0), dict(mu=0.12, fz_max=130.0), dict(fz_max=90.0, mu=0.2), dict(alpha=2000.0),
       dict(beta=300.0, gamma=400.0), dict(mu=0.4, fz_max=120.0), dict(alpha=5e4, beta=2000.0, gamma=1.0, mu=0.3))
MASS = (12.0, 14.0, 10.5, 9.0, 13.25, 11.0, 17.5, 15.75)
TICK_PARAMS = dict(stand_duration=0.007, t_walk_start=0.1, t_period=0.1)
T0, K = 48, 16


def rows_for(body, B, params):
    from quadrupedal_loco_amd import qp
    if body == "none":
        return None
    if body == "same":
        return qp.force_body_rows(B, params=params)
    eight = np.concatenate([qp.force_body_rows(1, params=params, mass=m, **ov) for ov, m in zip(MIX, MASS)])
    eight[:, 6:15] *= (eight[:, 0:1] / 12.0)
    return np.ascontiguousarray(eight[np.arange(B) % len(MIX)])


def windows(launch, sync, elapsed, window_s, warmup):
    """us per launch over one window of at least window_s seconds."""
    for _ in range(warmup):
        launch()
    sync()
    n = max(3, int(np.ceil(1.2 * window_s / (elapsed(launch, 3) / 3))))
    t = elapsed(launch, n)
    if t < window_s:                                   # the estimate was short: once more, longer
        n = int(np.ceil(n * 1.5 * window_s / t))
        t = elapsed(launch, n)
    return 1e6 * t / n, n


def measure(args):
    import torch
    from quadrupedal_loco_amd import _lib, go1servo, qp
    if not torch.cuda.is_available():
        raise SystemExit("bench_force_body: no GPU; there is no host path")
    if args.entry == "plain" and args.body != "none":
        raise SystemExit("--entry plain takes no rows")
    dev = torch.device("cuda:0")
    B = args.batch
    L = _lib.lib()
    dt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def elapsed(launch, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    line = {"bench": "force_body", "what": args.what, "entry": args.entry, "body": args.body, "batch": B,
            "lib": os.path.relpath(_lib.LIB_PATH, ROOT)}
    if args.what == "qp":
        from cases import force_inputs
        solver = qp.ForceQP(batch=B, device=dev)
        rows = rows_for(args.body, B, solver.params)
        rows = dt(rows) if rows is not None else None
        rng = np.random.default_rng(3)
        sets = [{k: dt(v) for k, v in force_inputs(rng, B).items()} for _ in range(8)]
        keys = ("com_des", "leg_des", "F_force_des", "rfoot_des", "lfoot_des", "base_p", "feet_p", "FT_total_des",
                "mode", "right_support", "y_coef")
        tail = [_lib.ptr(getattr(solver, k)) for k in ("F_leg_ref", "grf_opt", "F_leg_guess", "qp_solution", "status",
                                                        "iters", "order_ws")]
        calls = [[C.byref(solver.params), B] + [_lib.ptr(s[k]) for k in keys] + tail for s in sets]
        for mode, n_sets in (("changing", 8), ("repeated", 1)):
            k = [0]

            def launch():
                a = calls[k[0] % n_sets]
                k[0] += 1
                if args.entry == "plain":
                    _lib.check(L.qloco_force_qp_solve_ordered(*a, stream), "qloco_force_qp_solve_ordered")
                else:
                    _lib.check(L.qloco_force_qp_solve_body(*a, _lib.ptr(rows), stream), "qloco_force_qp_solve_body")

            us, n = windows(launch, torch.cuda.synchronize, elapsed, args.window, 16)
            st, it = solver.status.cpu().numpy(), solver.iters.cpu().numpy()
            line[mode] = {"us_per_launch": round(us, 3), "launches": n, "solves_per_s": round(B / (us * 1e-6), 1),
                          "mean_iters": round(float(it.mean()), 4), "status_ok": int((st == 0).sum())}
    else:
        base = go1servo.synth_inputs(20261020, min(B, 256), T0 + K)
        reps = -(-B // min(B, 256))
        tile = lambda a, ax: dt(np.concatenate([a] * reps, ax).take(range(B), ax))
        q_mea, quat, gait = (tile(base[k], 1) for k in ("q_mea", "quat", "gait_msg"))
        mode, yoff = tile(base["gait_mode"], 0), tile(base["y_offset"], 0)
        tk = go1servo.Go1ServoTick(B, dev, diag=False, **TICK_PARAMS)
        rows = rows_for(args.body, B, tk.params.force)
        rows = dt(rows) if rows is not None else None
        o = tk.out

        def tick(t):
            head = (C.byref(tk.params), B, _lib.ptr(tk.ws), t, _lib.ptr(q_mea[t]), _lib.ptr(quat[t]), _lib.ptr(gait[t]),
                    _lib.ptr(mode), _lib.ptr(yoff), _lib.ptr(o["q_cmd"]), _lib.ptr(o["ctrl_msg"]), _lib.ptr(o["tau"]),
                    _lib.ptr(o["grf_opt"]), None, None)
            if args.entry == "plain":
                _lib.check(L.qloco_go1_servo_tick(*head, stream), "qloco_go1_servo_tick")
            else:
                _lib.check(L.qloco_go1_servo_tick_body(*head, _lib.ptr(rows), stream), "qloco_go1_servo_tick_body")

        for t in range(T0):
            tick(t)
        rec0 = tk.get_state().clone()

        def window():
            tk.set_state(rec0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(K):
                tick(T0 + k)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / K

        for _ in range(4):
            window()
        ws = sorted(window() for _ in range(args.tick_windows))
        if not bool(torch.isfinite(o["tau"]).all().item()):
            raise SystemExit("the timed ticks did not stay finite")
        line["tick"] = {"us_per_launch": round(ws[len(ws) // 2], 3), "windows": len(ws), "ticks_per_window": K,
                        "robot_ticks_per_s": round(B / (ws[len(ws) // 2] * 1e-6), 1)}
    print(json.dumps(line), flush=True)


def ab(args):
    """Fresh child processes, one at a time; the table and what it says."""
    parent = os.path.abspath(args.parent_lib)
    if not os.path.exists(parent):
        raise SystemExit("--parent-lib: %s not found" % parent)
    configs = [("parent", "none", "plain", parent), ("tree", "none", "body", None), ("tree", "same", "body", None),
               ("tree", "mixed", "body", None)]
    got = {}
    for r in range(args.rounds):
        for what in ("qp", "tick"):
            for who, body, entry, lib_path in configs:
                env = dict(os.environ)
                env.pop("QLOCO_LIB", None)
                if lib_path:
                    env["QLOCO_LIB"] = lib_path
                cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--body", body, "--entry", entry,
                       "--batch", str(args.batch), "--window", str(args.window)]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    raise SystemExit("child failed: %s\n%s%s" % (" ".join(cmd), p.stdout, p.stderr))
                rec = json.loads(p.stdout.strip().splitlines()[-1])
                print(json.dumps(rec), flush=True)
                for mode in ("changing", "repeated", "tick"):
                    if mode in rec:
                        got.setdefault((mode, who, body), []).append(rec[mode])
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["Go1 force QP and servo tick with per-robot bodies (qloco_force_qp_solve_body,",
             "qloco_go1_servo_tick_body; DESIGN.md §4f) -- the A/B of the rows.", "",
             "Tool: tools/bench_force_body.py --ab, B = %d, one MI355X, one session, one fresh" % args.batch,
             "process per figure, one at a time, alternating parent / none / same / mixed, %d rounds." % args.rounds,
             "\"parent\" is the library built from the commit before the rows, through",
             "qloco_force_qp_solve_ordered / qloco_go1_servo_tick; \"tree\" is this tree through the",
             "_body entry points.  qp: grouped launch, cases.force_inputs(seed 3), 16 warm-up launches,",
             "one window of >= %.1f s between two device events; changing = eight input sets cycled," % args.window,
             "repeated = one set.  tick: gait branch, windows of %d ticks from one saved record, median" % K,
             "of %d windows per process.  Median of the %d runs (upper median); spread = max - min." % (
                 args.tick_windows, args.rounds), ""]
    for mode, title in (("changing", "force QP, changing inputs"), ("repeated", "force QP, repeated inputs"),
                        ("tick", "servo tick, gait branch")):
        lines.append("%s -- us per launch" % title)
        lines.append("%-22s" % "" + "".join("%10s" % ("run %d" % (i + 1)) for i in range(args.rounds)) +
                     "    median    spread  mean iters")
        stats = {}
        for who, body, _, _ in configs:
            v = [x["us_per_launch"] for x in got[(mode, who, body)]]
            stats[(who, body)] = (med(v), max(v) - min(v))
            it = got[(mode, who, body)][0].get("mean_iters")
            lines.append("%-7s%-15s" % (who, {"none": "body = NULL", "same": "rows = params", "mixed": "eight-body mix"}[body]) +
                         "".join("%10.2f" % x for x in v) + "%10.2f%10.2f" % stats[(who, body)] +
                         ("%12.3f" % it if it is not None else ""))
        (pm, ps), (nm, _) = stats[("parent", "none")], stats[("tree", "none")]
        sm, mm = stats[("tree", "same")][0], stats[("tree", "mixed")][0]
        unit = "solves" if mode != "tick" else "robot-ticks"
        lines.append("%s/s (median): parent %.2f M, tree none %.2f M, same %.2f M, mixed %.2f M." % (
            unit, args.batch / pm, args.batch / nm, args.batch / sm, args.batch / mm))
        lines.append("body = NULL against the parent: %+.2f us (%+.2f %%); the parent's own spread is %.2f us: %s." % (
            nm - pm, 100 * (nm - pm) / pm, ps, "inside it" if nm - pm <= ps else "OUTSIDE it -- a finding to explain"))
        lines.append("rows = params against body = NULL on the tree (the rows' own cost): %+.2f us, %+.2f %%, %.2f ns per robot." % (
            sm - nm, 100 * (sm - nm) / nm, 1e3 * (sm - nm) / args.batch))
        lines.append("")
    out = os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=("qp", "tick"), default="qp")
    ap.add_argument("--body", choices=("none", "same", "mixed"), default="none")
    ap.add_argument("--entry", choices=("body", "plain"), default="body")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--window", type=float, default=0.4, help="least timed window of the qp, seconds")
    ap.add_argument("--tick-windows", type=int, default=9)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join("profiles", "force_body_rows_ab.txt"))
    args = ap.parse_args()
    if args.ab:
        if not args.parent_lib:
            ap.error("--ab needs --parent-lib")
        return ab(args)
    measure(args)


if __name__ == "__main__":
    main()
