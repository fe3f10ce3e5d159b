"""Measurement of the A1 gait plan / swing-leg control / terrain pitch / joint
torque kernels (include/qloco.h section 13) and of the whole device-resident
A1 tick without the force solver.

    python tools/bench_a1_ctrl.py [--robots N] [--steps K] [--warmup W] [--repeats R] [--out FILE]

Workload: N robots (default 65,536), a1ctrl.synth_inputs tiled to N and
resident in HBM before the timed region, movement_mode 1 for three robots in
four (the gait runs, the filter rings advance and wrap).  Device events around
K steps, R windows, the median window reported with all windows.  Timed: each
of qloco_a1_ctrl_plan_swing (every optional output requested), _terrain and
_joint_torques alone, and the whole tick kin + plan_swing + EKF update +
terrain + torques (ground forces given, no solver).

Algorithmic HBM bytes per robot-tick (fp64; the model, not a measurement; the
workspace keeps flags and ring indices as doubles):
  plan_swing  inputs dt 8 + movement_mode 4 + root_lin_vel 24 + root_lin_vel_d 24
              + root_pos 24 + root_rot_mat 72 + root_rot_mat_z 72 + foot_pos_abs 96
              + foot_force 32 = 356;
              workspace read: gait_counter 32 + early 32 + foot_pos_start 96 +
              the two *_last_time 192 + ring fill / head 64 + sum_ / correction_
              192 + the oldest ring slot 96 = 704;
              workspace written: gait_counter / plan / early / contacts 128 +
              target_rel, joint_torques (zeroed), start, the two *_last_time,
              foot_forces_kin 576 + sum_ / correction_ / recent 288 + the new
              ring slot 96 + fill / head 64 = 1152;
              outputs: flags 12 + gait_counter 32 + six 3x4 arrays 576 = 620
  terrain     recent 96 + root_pos 24 + root_euler_d 8 + 8 + filter scalars 32 +
              32 + one ring slot read 8 and written 8 + angle 8 + 8 + surf_coef 24 = 256
  torques     j_foot 288 + forces 96 + counter 8 + 8 + contacts 32 + held torques
              96 + foot_forces_kin 96 + torques 96 + 96 = 816
  kin, ekf    tools/bench_a1_est.py: 1064 and 3432
The ring traffic is one slot in and one slot out whatever the window length.
Peak HBM 8.0 TB/s (MI355X_MICROARCH.md).  One JSON record on stdout and in
--out (default profiles/bench_a1_ctrl.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
BYTES = {"plan_swing": 356 + 704 + 1152 + 620, "terrain": 256, "joint_torques": 816,
         "kin": 224 + 840, "ekf": 2 * 1512 + 356 + 52}
BYTES_TICK = sum(BYTES.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_a1_ctrl.json"))
    args = ap.parse_args()
    import torch
    from quadrupedal_loco_amd import a1ctrl, a1est
    if not torch.cuda.is_available():
        raise SystemExit("bench_a1_ctrl needs a GPU")
    dev = torch.device("cuda:0")
    N = args.robots
    base = a1ctrl.synth_inputs(20261019, min(N, 4096), 1)
    rep = (N + 4095) // 4096

    def tile(a):
        return torch.from_numpy(np.ascontiguousarray(np.concatenate([a] * rep)[:N])).to(dev)

    d = {k: tile(v[0]) for k, v in base.items()}
    kin = a1est.A1LegKin()
    est = a1est.A1Estimator(N, dev)
    ctrl = a1ctrl.A1GaitSwing(N, dev)
    k0 = kin.forward(d["joint_pos"], d["joint_vel"], d["root_quat"])
    est.init(k0.root_rot_mat, k0.foot_pos_rel)
    eres = a1est.A1EstResult(*(torch.empty((N, n), dtype=t, device=dev)
                               for n, t in ((3, torch.float64), (3, torch.float64), (4, torch.uint8))))
    eres.root_pos.copy_(d["root_pos"])
    eres.root_lin_vel.zero_()
    sw = ctrl.plan_swing(d["dt"], d["movement_mode"], d["root_pos"], d["root_lin_vel"], d["root_lin_vel_d"],
                         k0.root_rot_mat, k0.root_rot_mat_z, k0.foot_pos_abs, d["foot_force"])
    ter = ctrl.terrain(d["root_pos"], d["root_euler_d"])
    tau = ctrl.joint_torques(k0.j_foot, d["foot_forces_grf"])

    def plan():
        ctrl.plan_swing(d["dt"], d["movement_mode"], eres.root_pos, eres.root_lin_vel, d["root_lin_vel_d"],
                        k0.root_rot_mat, k0.root_rot_mat_z, k0.foot_pos_abs, d["foot_force"], out=sw)

    def terrain():
        ctrl.terrain(eres.root_pos, d["root_euler_d"], out=ter)

    def torques():
        ctrl.joint_torques(k0.j_foot, d["foot_forces_grf"], out=tau)

    def tick():
        kin.forward(d["joint_pos"], d["joint_vel"], d["root_quat"], out=k0)
        plan()
        est.update(d["dt"], d["movement_mode"], k0.root_rot_mat, d["imu_acc"], d["imu_ang_vel"],
                   k0.foot_pos_rel, k0.foot_vel_rel, d["foot_force"], out=eres)
        terrain()
        torques()

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    for _ in range(args.warmup):
        tick()
    torch.cuda.synchronize()
    med = lambda v: v[len(v) // 2]
    ms = {name: sorted(window(fn) for _ in range(args.repeats))
          for name, fn in (("tick", tick), ("plan_swing", plan), ("terrain", terrain), ("joint_torques", torques))}
    state = ctrl.get_state()
    finite = bool(torch.isfinite(state).all().item() and torch.isfinite(tau).all().item())
    wrapped = bool((state[:, 102:106] == 60).any().item())
    rate = lambda name: N / (med(ms[name]) * 1e-3)
    gbs = lambda name, nbytes: nbytes * N / (med(ms[name]) * 1e-3) / 1e9
    parts = {}
    for name in ("plan_swing", "terrain", "joint_torques"):
        parts[name] = {"ms_per_step": med(ms[name]), "ms_per_step_windows": ms[name],
                       "robot_ticks_per_s": rate(name), "algorithmic_bytes_per_robot_tick": BYTES[name],
                       "gbs": gbs(name, BYTES[name]), "frac_hbm_peak": gbs(name, BYTES[name]) / HBM_PEAK_GBS}
    g = gbs("tick", BYTES_TICK)
    line = {"metric": "device-resident A1 tick without the solver (kin + plan_swing + EKF + terrain + torques), "
                      "robot-ticks/sec (fp64)",
            "value": rate("tick"), "unit": "robot-ticks/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "repeats": args.repeats, "ms_per_step": med(ms["tick"]),
            "ms_per_step_windows": ms["tick"], "higher_is_better": True, "dtype": "f64", "data": "synthetic",
            "state_finite": finite, "recent_contact_rings_full": wrapped,
            "config": {"workload": "%d robots" % N}, "parts": parts,
            "roofline": {"bound": "hbm", "achieved": g, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": g / HBM_PEAK_GBS,
                         "algorithmic_bytes_per_robot_tick": dict(BYTES, total=BYTES_TICK)}}
    if not finite:
        raise SystemExit("non-finite controller state after the timed steps")
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
