"""Measurement of the batched Go1 servo tick (include/qloco.h section 16:
`qloco_go1_servo_tick` = one kernel for joint state -> IK + the force block's
glue, then the force QP and compute_joint_torques) against what a caller
writes without it.

    python tools/bench_go1_servo.py [--robots N] [--steps K] [--warmup W] [--repeats R] [--out FILE]

Workload: N robots (default 65,536) resident in HBM, the inputs of
`go1servo.synth_inputs` for 256 robots tiled over the batch, the test
parameters (8 stand-up ticks, the walk gate at count 20, n_period 20) so that
the window lies in the gait branch with all of modes 101 / 102 / 103 walking.
A window is K consecutive ticks from one saved state record (re-seeded,
untimed, before every window).  Device events around the K ticks, R windows
after W warm-up ticks (long enough for the clock ramp), the median
window reported with all windows.  Timed in the same session on the same
inputs:
  tick         qloco_go1_servo_tick, the whole tick, no optional output
  composition  kin.leg_fk + torch (Euler angles, 15 filters, targets, velocities)
               + kin.leg_ik + ServoForceBlock: the same work, equal to rounding
               but not held bit for bit, staged through HBM between the calls
  force_block  ServoForceBlock alone on the composition's staged arrays
The new kernel cannot be launched on its own through the C ABI; its time is
tick - force_block, which charges it the difference of the two glue kernels and
the launch boundary.

Bytes moved by the new kernel per robot-tick are counted from its code (logical
bytes: every value it loads or stores once); the fraction of HBM peak uses the
8 TB/s of the specification.

One JSON record on stdout and in --out (default profiles/bench_go1_servo.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
PARAMS = dict(stand_duration=0.007, t_walk_start=0.1, t_period=0.1)
T0 = 48          # first tick of a window: 8 stand-up + 40 gait ticks in
# the tick kernel's loads and stores per robot-tick in the gait branch (doubles unless noted)
LOADS = dict(quat=4, q_mea=12, v_est_rel=12, foot_rel_mea_old=12, count_tint_mode_i32=1.5, gait_slots=16,
             filter_memories=75, comv_des=3, com_des_pre=3, body_p_des=3, body_r_des=3, foot_des=12, y_offset=1,
             foot_homing=12, angle_des=12, foot_rel_des_old=12, swing_i32=2)
STORES = dict(v_est_rel=12, foot_rel_mea=12, ctrl_msg=25, filter_memories_without_call_counts=60, references=18,
              Jaco=36, v_relative=12, foot_rel_des=12, swing_i32=2, F_sum=6, Force_L_R=6, rs_count_tint_i32=1.5, body_p_des=3, body_r_des=3,
              q_cmd=12, angle_des=12, foot_des=12, foot_rel_des_old=12, foot_rel_mea_old=12, com_des_pre=3)


def kernel_figures():
    import test_kernel_resources as K
    out = {}
    for name, k in K._kernels().items():
        if "go1_servo_kernel" not in name:
            continue
        regs = k[".vgpr_count"] + k[".agpr_count"]
        alloc = -(-regs // 8) * 8
        out[name] = {"vgpr": k[".vgpr_count"], "agpr": k[".agpr_count"], "sgpr": k[".sgpr_count"],
                     "vgpr_spill": k[".vgpr_spill_count"], "sgpr_spill": k.get(".sgpr_spill_count", 0),
                     "scratch_bytes": k[".private_segment_fixed_size"],
                     "lds_bytes": k[".group_segment_fixed_size"], "waves_per_simd_by_registers": min(8, 512 // alloc)}
    return out


class Composition:
    """The tick as a caller composes it today: torch for everything between the
    stand-alone kinematics calls and the force block."""

    def __init__(self, N, dev, state, mode, yoff):
        import torch
        from quadrupedal_loco_amd import go1servo as G
        from quadrupedal_loco_amd.qp import ServoForceBlock
        import go1_servo_ref as R
        self.torch, self.N = torch, N
        f = G.STATE_FIELDS
        cut = lambda k: state[:, f[k][0]:f[k][1]].clone()
        self.mem = cut("filters").view(N, 15, 5)
        self.s = {k: cut(k) for k in ("angle_des", "foot_homing", "body_p_des", "body_r_des", "foot_des",
                                      "foot_rel_mea_old", "com_des_pre", "v_est_rel")}
        self.count = cut("count_in_rt_loop")[:, 0].to(torch.int32)
        coef = np.array([R.butter_coef(200.0, fc) for fc in R.filter_cutoffs()])
        self.coef = torch.from_numpy(coef).to(dev)
        self.slots = torch.tensor(G.FILTER_SLOTS, device=dev)
        self.leg = torch.arange(4, dtype=torch.int32, device=dev).repeat(N)
        self.zeros = torch.zeros((4 * N, 3), dtype=torch.float64, device=dev)
        self.mode, self.yoff = mode, yoff
        self.blk = ServoForceBlock(N, dev)
        right = torch.zeros((N, 4), dtype=torch.bool, device=dev)
        for m, legs in ((101, (0, 2)), (102, (0, 3)), (103, (0, 1))):
            for l in legs:
                right[:, l] |= mode == m
        self.right = right[:, :, None]
        self.walk = ((mode >= 101) & (mode <= 103))
        self.staged = None

    def tick(self, q_mea, quat, gait):
        torch, N, s = self.torch, self.N, self.s
        from quadrupedal_loco_amd import kin
        w, x, y, z = quat.unbind(1)
        e = torch.stack([torch.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)),
                         torch.asin(torch.clamp(2 * (w * y - z * x), -1, 1)),
                         torch.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))], 1)
        mea, _ = kin.leg_fk(q_mea.view(-1, 3), self.leg, self.zeros, e.repeat_interleave(4, dim=0))
        mea = mea.view(N, 12)
        s["v_est_rel"] = (mea - s["foot_rel_mea_old"]) / 0.005
        self.count = self.count + 1
        yv = gait[:, self.slots]
        m, c = self.mem, self.coef
        out = c[:, 0] * yv + c[:, 1] * m[:, :, 0] + c[:, 2] * m[:, :, 1] + c[:, 3] * m[:, :, 2] + c[:, 4] * m[:, :, 3]
        self.mem = torch.stack([yv, m[:, :, 0], out, m[:, :, 2], m[:, :, 4]], 2)
        com, rf, lf, coma = out[:, 0:3], out[:, 3:6], out[:, 6:9], out[:, 9:12]
        walk = (self.walk & (self.count.double() * 0.005 >= 0.1))[:, None]
        bp = torch.where(walk, torch.stack([com[:, 0], com[:, 1] * self.yoff, com[:, 2]], 1), s["body_p_des"])
        dn = (self.count - 60).double()
        pitch = torch.where((self.mode == 103) & (dn > 0), -(0.1 * torch.sin(2 * 3.141526 / 0.2 * dn * 0.005)),
                            torch.where(self.mode == 103, s["body_r_des"][:, 1], torch.zeros_like(dn)))
        br = torch.where(walk, torch.stack([torch.zeros_like(pitch), pitch, torch.zeros_like(pitch)], 1), s["body_r_des"])
        hh = torch.tensor([0.0, 0.12675, 0.0], dtype=torch.float64, device=q_mea.device)
        hm = s["foot_homing"].view(N, 4, 3)
        tgt = torch.where(self.right, hm + rf[:, None, :] + hh, hm + lf[:, None, :] - hh)
        fdes = torch.where(walk[:, :, None], tgt, s["foot_des"].view(N, 4, 3)).reshape(N, 12)
        q, _, J, _ = kin.leg_ik(fdes.view(-1, 3), s["angle_des"].view(-1, 3), self.leg,
                                bp.repeat_interleave(4, dim=0), br.repeat_interleave(4, dim=0))
        s.update(angle_des=q.view(N, 12), body_p_des=bp, body_r_des=br, foot_des=fdes, foot_rel_mea_old=mea,
                 com_des_pre=com)
        self.staged = (coma.contiguous(), com.contiguous(), rf.contiguous(), lf.contiguous(), bp, fdes,
                       gait[:, 99].to(torch.int32), self.mode, self.yoff, self.count, J.view(N, 36), mea,
                       s["v_est_rel"])
        return self.blk.step(*self.staged)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_go1_servo.json"))
    args = ap.parse_args()
    import torch
    from quadrupedal_loco_amd import go1servo as G
    if not torch.cuda.is_available():
        raise SystemExit("bench_go1_servo needs a GPU")
    dev = torch.device("cuda:0")
    N, K = args.robots, args.steps
    base = G.synth_inputs(20261020, min(N, 256), T0 + K)
    reps = -(-N // min(N, 256))
    tile = lambda a, ax: torch.from_numpy(np.ascontiguousarray(np.concatenate([a] * reps, ax).take(range(N), ax))).to(dev)
    q_mea, quat, gait = (tile(base[k], 1) for k in ("q_mea", "quat", "gait_msg"))
    mode, yoff = tile(base["gait_mode"], 0), tile(base["y_offset"], 0)
    tk = G.Go1ServoTick(N, dev, diag=False, **PARAMS)
    for t in range(T0):
        tk.step(q_mea[t], quat[t], gait[t], mode, yoff)
    rec0 = tk.get_state().clone()
    comp = [None]

    def window(what):
        if what == "tick":
            tk.set_state(rec0, n_count=T0)
        else:
            comp[0] = Composition(N, dev, rec0, mode, yoff)
            if what == "force_block":
                comp[0].tick(q_mea[T0], quat[T0], gait[T0])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(K):
            if what == "tick":
                o = tk.step(q_mea[T0 + k], quat[T0 + k], gait[T0 + k], mode, yoff)
            elif what == "composition":
                o = comp[0].tick(q_mea[T0 + k], quat[T0 + k], gait[T0 + k])
            else:
                o = comp[0].blk.step(*comp[0].staged)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / K, o

    med = lambda v: sorted(v)[len(v) // 2]
    res, last = {}, {}
    for what in ("tick", "composition", "force_block"):
        for _ in range(max(1, args.warmup // K)):
            window(what)
        ws = []
        for _ in range(args.repeats):
            ms, last[what] = window(what)
            ws.append(ms)
        ws.sort()
        res[what] = {"us_per_tick": 1e3 * med(ws), "us_per_tick_windows": [1e3 * x for x in ws],
                     "robot_ticks_per_s": N / (med(ws) * 1e-3)}
    tau, tau_c = last["tick"].tau, last["composition"]["tau"]
    finite = bool(torch.isfinite(tau).all().item() and torch.isfinite(last["tick"].q_cmd).all().item())
    agree = float((tau - tau_c).abs().max().item())
    if not finite:
        raise SystemExit("the timed ticks did not stay finite")
    own_us = res["tick"]["us_per_tick"] - res["force_block"]["us_per_tick"]
    loads, stores = 8 * sum(LOADS.values()), 8 * sum(STORES.values())
    line = {"metric": "Go1 servo tick (joint state, IMU quaternion and /MPC/Gait row to joint commands and torques) of "
                      "every resident robot, robot-ticks/sec (fp64)",
            "value": res["tick"]["robot_ticks_per_s"], "unit": "robot-ticks/s", "n_gpus": 1, "steps": K,
            "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True, "dtype": "f64",
            "data": "synthetic", "config": {"workload": "%d robots, gait branch, ticks %d..%d" % (N, T0, T0 + K - 1)},
            "qloco_go1_servo_tick": res["tick"], "composition_today": res["composition"],
            "servo_force_block_alone": res["force_block"],
            "speedup_over_composition": res["composition"]["us_per_tick"] / res["tick"]["us_per_tick"],
            "new_kernel": {"us_per_tick": own_us, "how": "tick - force block alone (includes the launch boundary)",
                           "bytes_per_robot_tick": {"loads": loads, "stores": stores, "what": "logical, from the code"},
                           "bytes_per_tick": (loads + stores) * N,
                           "fraction_of_hbm_peak": ((loads + stores) * N / (own_us * 1e-6)) / HBM_PEAK if own_us > 0 else None,
                           "hbm_peak_bytes_per_s": HBM_PEAK},
            "last_tick": {"all_finite": finite, "max_abs_tau_difference_to_composition": agree},
            "kernels": kernel_figures()}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
