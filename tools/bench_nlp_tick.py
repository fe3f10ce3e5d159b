"""Measurement of the full planner tick (include/qloco.h section 15:
`qloco_nlp_tick` = the step-timing SQP kernel of section 14 followed by the
CoM-height / ZMP / DCM / swing-foot kernel) against the step-timing call alone.

    python tools/bench_nlp_tick.py [--robots N] [--steps K] [--warmup W] [--repeats R] [--out FILE]

Workload: that of tools/bench_nlp.py -- N robots (default 65,536) resident in
HBM, per-robot step length in [0.04, 0.09] and width within +-10 %, here on
stepped ground (per-robot step height in [0.01, 0.03], so the 7 x 7 system has
a right-hand side that is not constant).  A window is K consecutive ticks
i = I0 .. I0 + K - 1 from one saved pair of records (re-seeded, untimed, before
every window): 16 ticks from i = 20 cross the first step boundary, so the
window holds the initial branch, the double-support hold and ten cubic ticks
of the first swing.  Device events around the K ticks, R windows after W
warm-up ticks, the median window reported with all windows.  Timed in the same
session, on the same records and inputs: `qloco_nlp_tick` and
`qloco_nlp_step_timing` alone.  The new kernel cannot be launched on its own
through the C ABI; its time is the difference of the two medians, which
includes the launch boundary between the two kernels.

Bytes moved by the new kernel per robot-tick are counted from its code (logical
bytes: every value it loads or stores once, not the sectors the strided
gathers from the row-per-robot ts / tx touch); the fraction of HBM peak uses
the 8 TB/s of the specification.

Both forms of the new kernel are timed (one robot per lane, shipped; one robot
per 8-lane group, `nlp.set_tick_group_width(8)`).

One JSON record on stdout and in --out (default profiles/bench_nlp_tick.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

I0 = 20          # first tick of a window, as in tools/bench_nlp.py
HBM_PEAK = 8.0e12

# the new kernel's loads and stores per robot-tick on a cubic tick (doubles unless noted)
LOADS = dict(step_status_i32=0.5, sched_i32=2, t_int_stop_i32=1, com=18, tick_scalars=5, tx0=27, footz_ref=6,
             lift=1, ts_tx_td_gathers=6, footholds=4, step_slots=3, ring=12)
STORES = dict(com_traj=38, rlfoot_traj=18, right_support_status_i32=1, ring=12, bjx1_last_ry=3)


def kernel_figures():
    import test_kernel_resources as K
    out = {}
    for name, k in K._kernels().items():
        if "nlp_tick_kernel" not in name:
            continue
        regs = k[".vgpr_count"] + k[".agpr_count"]
        alloc = -(-regs // 8) * 8
        out[name] = {"vgpr": k[".vgpr_count"], "agpr": k[".agpr_count"], "sgpr": k[".sgpr_count"],
                     "vgpr_spill": k[".vgpr_spill_count"], "scratch_bytes": k[".private_segment_fixed_size"],
                     "lds_bytes": k[".group_segment_fixed_size"], "waves_per_simd_by_registers": min(8, 512 // alloc)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_nlp_tick.json"))
    args = ap.parse_args()
    import torch
    from quadrupedal_loco_amd import nlp
    if not torch.cuda.is_available():
        raise SystemExit("bench_nlp_tick needs a GPU")
    dev = torch.device("cuda:0")
    N, K = args.robots, args.steps
    rng = np.random.default_rng(20261019)
    sl = torch.from_numpy(rng.uniform(0.04, 0.09, N)).to(dev)
    sw = torch.from_numpy(2 * 0.12675 * rng.uniform(0.9, 1.1, N)).to(dev)
    sh = torch.from_numpy(rng.uniform(0.01, 0.03, N)).to(dev)
    pl = nlp.PlannerTick(N, dev, steplength=sl, stepwidth=sw, stepheight=sh)
    z6 = torch.zeros((N, 6), dtype=torch.float64, device=dev)
    rf = torch.tensor([0.0, -0.12675], dtype=torch.float64, device=dev).expand(N, 2).contiguous()
    lf = torch.tensor([0.0, 0.12675], dtype=torch.float64, device=dev).expand(N, 2).contiguous()
    ti = [torch.full((N,), i, dtype=torch.int32, device=dev) for i in range(1, I0 + K)]
    out = None
    for i in range(1, I0):
        out = pl.tick(ti[i - 1], z6, rf, lf, out=out)
    rec0, trec0 = pl.get_state().clone(), pl.get_tick_state().clone()

    def window(full):
        pl.set_state(rec0)
        pl.set_tick_state(trec0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(K):
            if full:
                pl.tick(ti[I0 - 1 + k], z6, rf, lf, out=out)
            else:
                pl.step_timing_tick(ti[I0 - 1 + k], z6, rf, lf, out=out.step_timing)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / K

    med = lambda v: sorted(v)[len(v) // 2]
    res = {}
    for name, full, gw in (("tick", True, 1), ("step_timing", False, 1), ("tick_group8", True, 8)):
        prev = nlp.set_tick_group_width(gw)
        for _ in range(max(1, args.warmup // K)):
            window(full)
        w = sorted(window(full) for _ in range(args.repeats))
        nlp.set_tick_group_width(prev)
        res[name] = {"us_per_tick": 1e3 * med(w), "us_per_tick_windows": [1e3 * x for x in w],
                     "robot_ticks_per_s": N / (med(w) * 1e-3)}
    window(True)
    finite = bool(torch.isfinite(out.com_traj).all().item() and torch.isfinite(out.rlfoot_traj).all().item())
    ok = bool((out.status == 0).all().item())
    swing = float((out.right_support != 2).double().mean().item())
    if not finite or not ok:
        raise SystemExit("the timed ticks did not stay finite / OK")
    own_us = res["tick"]["us_per_tick"] - res["step_timing"]["us_per_tick"]
    loads, stores = 8 * sum(LOADS.values()), 8 * sum(STORES.values())
    line = {"metric": "full planner tick (step-timing SQP + CoM height, ZMP / DCM, swing feet) of every resident "
                      "robot, robot-ticks/sec (fp64)",
            "value": res["tick"]["robot_ticks_per_s"], "unit": "robot-ticks/s", "n_gpus": 1, "steps": K,
            "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True, "dtype": "f64",
            "data": "synthetic", "config": {"workload": "%d robots, ticks %d..%d, stepped ground" % (N, I0, I0 + K - 1)},
            "qloco_nlp_tick": res["tick"], "qloco_nlp_step_timing_alone": res["step_timing"],
            "new_kernel": {"us_per_tick": own_us, "how": "difference of the two medians (includes the launch boundary)",
                           "bytes_per_robot_tick": {"loads": loads, "stores": stores, "what": "logical, from the code"},
                           "bytes_per_tick": (loads + stores) * N,
                           "fraction_of_hbm_peak": ((loads + stores) * N / (own_us * 1e-6)) / HBM_PEAK if own_us > 0 else None,
                           "hbm_peak_bytes_per_s": HBM_PEAK},
            "kernel_forms": {"lane_us_per_tick": own_us,
                             "group8_us_per_tick": res["tick_group8"]["us_per_tick"] - res["step_timing"]["us_per_tick"],
                             "qloco_nlp_tick_group8": res["tick_group8"], "shipped": "lane"},
            "last_tick": {"all_finite": finite, "all_ok": ok, "fraction_in_single_support": swing},
            "kernels": kernel_figures()}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
