"""Measurement of the A1 state-estimation front end (include/qloco.h sections
11 and 12): leg kinematics + one A1BasicEKF update per robot and tick.

    python tools/bench_a1_est.py [--robots N] [--steps K] [--warmup W] [--repeats R] [--out FILE]

Workload: N robots (default 65,536), a1est.synth_inputs tiled to N and
resident in HBM before the timed region; every step runs qloco_a1_leg_kin on
the joint state and qloco_a1_ekf_update on its outputs (device events around
K steps, R windows, the median window reported with the spread).  The filters
are initialised once and keep running, as in the control loop.

Algorithmic HBM bytes per robot-tick (fp64; the model, not a measurement):
  kin: in joint_pos 96 + joint_vel 96 + root_quat 32 = 224,
       out foot_pos_rel 96 + j_foot 288 + foot_vel_rel 96 + root_rot_mat 72 +
       root_euler 24 + root_rot_mat_z 72 + foot_pos_abs 96 + foot_vel_abs 96 = 840
  ekf: x + packed P read 1512 + written 1512, inputs dt 8 + movement_mode 4 +
       root_rot_mat 72 + imu 48 + foot_pos_rel 96 + foot_vel_rel 96 +
       foot_force 32 = 356, outputs 24 + 24 + 4 = 52
Peak HBM 8.0 TB/s (MI355X_MICROARCH.md).  The fraction of peak is the
whole-step rate over the peak, not a kernel's share.  One JSON record on
stdout and in --out (default profiles/bench_a1_est.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
BYTES_KIN = 224 + 840
BYTES_EKF = 2 * 1512 + 356 + 52


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_a1_est.json"))
    args = ap.parse_args()
    import torch
    from quadrupedal_loco_amd import a1est
    if not torch.cuda.is_available():
        raise SystemExit("bench_a1_est needs a GPU")
    dev = torch.device("cuda:0")
    N = args.robots
    base = a1est.synth_inputs(20261019, min(N, 4096), 1)
    rep = (N + 4095) // 4096

    def tile(a):
        return torch.from_numpy(np.ascontiguousarray(np.concatenate([a] * rep)[:N])).to(dev)

    jp, jv, qt = (tile(base[k][0]) for k in ("joint_pos", "joint_vel", "root_quat"))
    acc, om, ff, dt = (tile(base[k][0]) for k in ("imu_acc", "imu_ang_vel", "foot_force", "dt"))
    mode = tile(base["movement_mode"])
    kin = a1est.A1LegKin()
    est = a1est.A1Estimator(N, dev)
    k0 = kin.forward(jp, jv, qt)
    est.init(k0.root_rot_mat, k0.foot_pos_rel)
    res = a1est.A1EstResult(*(torch.empty((N, n), dtype=t, device=dev)
                              for n, t in ((3, torch.float64), (3, torch.float64), (4, torch.uint8))))

    def step(both=True, ekf=True):
        k = kin.forward(jp, jv, qt, out=k0) if both else k0
        if ekf:
            est.update(dt, mode, k.root_rot_mat, acc, om, k.foot_pos_rel, k.foot_vel_rel, ff, out=res)

    def window(**kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            step(**kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms_all = sorted(window() for _ in range(args.repeats))
    ms_ekf = sorted(window(both=False) for _ in range(args.repeats))
    ms_kin = sorted(window(ekf=False) for _ in range(args.repeats))
    x, P = est.state()
    finite = bool(torch.isfinite(x).all().item() and torch.isfinite(P).all().item())
    med = lambda v: v[len(v) // 2]
    ms = med(ms_all)
    gbs = (BYTES_KIN + BYTES_EKF) * N / (ms * 1e-3) / 1e9
    line = {"metric": "A1 leg kinematics + A1BasicEKF update, robot-ticks/sec (fp64)",
            "value": N / (ms * 1e-3), "unit": "robot-ticks/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "repeats": args.repeats, "ms_per_step": ms,
            "ms_per_step_windows": ms_all, "higher_is_better": True, "dtype": "f64",
            "data": "synthetic", "state_finite": finite,
            "config": {"workload": "%d robots, kin + ekf update per step" % N},
            "parts": {"ekf_update_only_ms": med(ms_ekf), "leg_kin_only_ms": med(ms_kin),
                      "ekf_update_only_robot_ticks_per_s": N / (med(ms_ekf) * 1e-3),
                      "ekf_update_only_gbs": BYTES_EKF * N / (med(ms_ekf) * 1e-3) / 1e9,
                      "leg_kin_only_gbs": BYTES_KIN * N / (med(ms_kin) * 1e-3) / 1e9},
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": gbs / HBM_PEAK_GBS,
                         "algorithmic_bytes_per_robot_tick": {"kin": BYTES_KIN, "ekf": BYTES_EKF,
                                                              "total": BYTES_KIN + BYTES_EKF}}}
    if not finite:
        raise SystemExit("non-finite filter state after the timed steps")
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
