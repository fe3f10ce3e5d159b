"""Measurement of the planner node tick (include/qloco.h section 17:
`qloco_nlp_node_tick` = a pre-kernel, section 15's `qloco_nlp_tick` unchanged
and a post-kernel that writes the /MPC/Gait row) against the planner tick alone
and against the host round trip it replaces.

    python tools/bench_nlp_node.py [--robots N] [--steps K] [--warmup W] [--repeats R] [--out FILE]

Workload: that of tools/bench_nlp_tick.py -- N robots (default 65,536) resident
in HBM on stepped ground, a window of K consecutive walking ticks i = 20 ..
20 + K - 1 from one saved set of records (re-seeded, untimed, before every
window); the node reaches i = 20 through one not-started tick, the 40 ticks of
the squat and 19 walking ticks.  Device events around the K ticks, R windows
after W warm-up ticks, the median window reported with all windows.  Timed in
the same session, on the same records:

  node        `qloco_nlp_node_tick`, both forms of the row store
              (`nlp.set_node_form`);
  tick        `qloco_nlp_tick` alone -- the parent, so the node's own cost (the
              two new kernels and their launch boundaries) is the difference;
  host        what a caller did before: `PlannerTick.tick`, the device-to-host
              copy of its outputs, a numpy packing of the row's copied slots and
              the host-to-device copy of the B x 100 rows.  The packing leaves
              out Zmp_distributor (slots 15..26), which a host caller would
              also have to run per robot, so this figure is a lower bound.

Bytes moved by the two new kernels per robot-tick are counted from their code
(logical bytes of a walking tick with _nTdx = 7: every value loaded or stored
once); the row store's LDS traffic is not HBM traffic, so both forms count the
same.  The fraction of HBM peak uses the 8 TB/s of the specification.

One JSON record on stdout and in --out (default profiles/bench_nlp_node.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

I0 = 20          # first tick of a window, as in tools/bench_nlp_tick.py
LEAD = 41        # one not-started tick and the squat
HBM_PEAK = 8.0e12

# loads and stores per robot-tick, doubles unless noted
PRE_LOADS = dict(msg=5, count_latch_stop_restart=4, bjx1_td1=2)
PRE_STORES = dict(count_latch=2, t_int_branch_i32=1, estimated_state=6, feedback=4, bjx1_td1=2, sched_i32=1)
POST_LOADS = dict(ints_i32=4, bjx1_td1=2, com_traj=38, rlfoot_traj=18, ts_tx_td_gathers=4, footz_ref=6, tx0=27,
                  boundary_state=6, co=6, ring=12, row=100)
POST_STORES = dict(ring=21, co=6, row_slots=72, status_sched_i32=4.5, gait_msg=100)


def kernel_figures():
    import test_kernel_resources as K
    out = {}
    for name, k in K._kernels().items():
        if "nlp_node_pre_kernel" not in name and "nlp_node_post_kernel" not in name:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_nlp_node.json"))
    args = ap.parse_args()
    import torch
    from quadrupedal_loco_amd import nlp
    if not torch.cuda.is_available():
        raise SystemExit("bench_nlp_node needs a GPU")
    dev = torch.device("cuda:0")
    N, K = args.robots, args.steps
    rng = np.random.default_rng(20261019)
    sl = torch.from_numpy(rng.uniform(0.04, 0.09, N)).to(dev)
    sw = torch.from_numpy(2 * 0.12675 * rng.uniform(0.9, 1.1, N)).to(dev)
    sh = torch.from_numpy(rng.uniform(0.01, 0.03, N)).to(dev)
    node = nlp.PlannerNode(N, dev, steplength=sl, stepwidth=sw, stepheight=sh)
    msg = torch.zeros((N, 25), dtype=torch.float64, device=dev)
    msg[:, 20], msg[:, 23] = 0.12675, -0.12675
    out = node.tick(msg)                                         # not started
    msg[:, 0] = 1.0
    for _ in range(LEAD - 1 + I0 - 1):
        out = node.tick(msg, out=out)
    recs = [node.get_state().clone(), node.get_tick_state().clone(), node.get_node_state().clone()]
    z6 = torch.zeros((N, 6), dtype=torch.float64, device=dev)
    rf, lf = msg[:, 22:24].contiguous(), msg[:, 19:21].contiguous()
    ti = [torch.full((N,), I0 + k, dtype=torch.int32, device=dev) for k in range(K)]
    pt = node.planner_tick(ti[0], z6, rf, lf)
    host_row = np.zeros((N, 100))
    staged = torch.from_numpy(host_row)
    gait = torch.empty((N, 100), dtype=torch.float64, device=dev)

    def host_step(k):
        o = node.planner_tick(ti[k], z6, rf, lf, out=pt)
        ct, rl = o.com_traj.cpu().numpy(), o.rlfoot_traj.cpu().numpy()
        rs, sc = o.right_support.cpu().numpy(), o.step_timing.sched.cpu().numpy()
        r = host_row
        r[:, 0:3], r[:, 36:39], r[:, 39:42] = ct[:, 0:3], ct[:, 3:6], ct[:, 6:9]
        r[:, 9:12], r[:, 6:9] = rl[:, 0:3], rl[:, 3:6]
        r[:, 12:14], r[:, 34:36] = ct[:, 9:11], ct[:, 11:13]
        r[:, 42:46], r[:, 46:58], r[:, 76:97] = ct[:, 13:17], rl[:, 6:18], ct[:, 17:38]
        r[:, 27], r[:, 99] = sc[:, 3], rs
        gait.copy_(staged)

    def window(kind):
        node.set_state(recs[0])
        node.set_tick_state(recs[1])
        node.set_node_state(recs[2])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(K):
            if kind == "node":
                node.tick(msg, out=out)
            elif kind == "tick":
                node.planner_tick(ti[k], z6, rf, lf, out=pt)
            else:
                host_step(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / K

    med = lambda v: sorted(v)[len(v) // 2]
    res = {}
    for name, kind, form in (("node_lane", "node", 0), ("node_lds", "node", 1), ("tick", "tick", None),
                             ("host", "host", None)):
        prev = nlp.set_node_form(form) if form is not None else None
        for _ in range(max(1, args.warmup // K)):
            window(kind)
        w = sorted(window(kind) for _ in range(args.repeats))
        if prev is not None:
            nlp.set_node_form(prev)
        res[name] = {"us_per_tick": 1e3 * med(w), "us_per_tick_windows": [1e3 * x for x in w],
                     "robot_ticks_per_s": N / (med(w) * 1e-3)}
    window("node")
    finite = bool(torch.isfinite(out.gait_msg).all().item())
    ok = bool((out.status == 0).all().item() and (out.sched[:, 0] == 2).all().item()
              and (out.sched[:, 2] == I0 + K - 1).all().item())
    if not finite or not ok:
        raise SystemExit("the timed ticks did not stay finite / OK / walking")
    shipped = "lane" if nlp.set_node_form(0) == 0 else "lds"
    nlp.set_node_form(0 if shipped == "lane" else 1)
    nbytes = 8 * (sum(PRE_LOADS.values()) + sum(PRE_STORES.values()) + sum(POST_LOADS.values())
                  + sum(POST_STORES.values()))
    forms = {}
    for name in ("node_lane", "node_lds"):
        own = res[name]["us_per_tick"] - res["tick"]["us_per_tick"]
        forms[name] = {"own_us_per_tick": own, "how": "node - tick medians (two kernels and their launch boundaries)",
                       "bytes_per_robot_tick": nbytes, "bytes_per_tick": nbytes * N,
                       "fraction_of_hbm_peak": (nbytes * N / (own * 1e-6)) / HBM_PEAK if own > 0 else None}
    best = res["node_" + shipped]
    line = {"metric": "planner node tick (/rt2nrt/state in, planner tick, Zmp_distributor, /MPC/Gait row out) of every "
                      "resident robot, robot-ticks/sec (fp64)",
            "value": best["robot_ticks_per_s"], "unit": "robot-ticks/s", "n_gpus": 1, "steps": K,
            "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "%d robots, walking ticks %d..%d, stepped ground" % (N, I0, I0 + K - 1)},
            "qloco_nlp_node_tick_lane": res["node_lane"], "qloco_nlp_node_tick_lds": res["node_lds"],
            "qloco_nlp_tick_alone": res["tick"],
            "host_round_trip": dict(res["host"], what="PlannerTick.tick, D2H of its outputs, numpy packing of the "
                                    "copied slots (no Zmp_distributor), H2D of the rows"),
            "speedup_over_host_round_trip": res["host"]["us_per_tick"] / best["us_per_tick"],
            "new_kernels": dict(forms, shipped=shipped, hbm_peak_bytes_per_s=HBM_PEAK,
                                bytes_what="logical, from the code, a walking tick with _nTdx = 7"),
            "last_tick": {"all_finite": finite, "all_ok_and_walking": ok},
            "kernels": kernel_figures()}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
