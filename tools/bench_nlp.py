"""Measurement of the fused step-timing SQP kernel (include/qloco.h section 14)
against the path a user had before it: the six QP arrays assembled in torch,
three `qloco_eiquadprog_solve` calls at (4, 1, 24) and the updates in torch.

    python tools/bench_nlp.py [--robots N] [--steps K] [--warmup W] [--repeats R] [--out FILE]

Workload: N robots (default 65,536) resident in HBM, per-robot step length in
[0.04, 0.09] and width within +-10 %.  A window is K consecutive planner ticks
i = I0 .. I0 + K - 1 from one saved record (re-seeded, untimed, before every
window), so the inputs change from tick to tick: the remaining-time bounds,
the active sets, one step boundary with its _k_yu == 0 tick and the two
skipped ticks before it.  Device events around the K ticks, R windows after W
warm-up ticks, the median window reported with all windows.  Timed in the same
session: the fused kernel at 4 (shipped), 8 and 16 lanes per robot, and the
torch + qloco_eiquadprog_solve composition (`ComposedPlanner` below, checked
against the fused kernel's results before it is timed).  The kernel that keeps
a CI copy in LDS is selected by the environment (QLOCO_NLP_CI=stored) and is
measured by a second run with --out set; --label names the run.

One JSON record on stdout and in --out (default profiles/bench_nlp_sqp.json).
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

I0 = 20          # first tick of a window: step 1, eight ticks before the step boundary
NS = 27


class ComposedPlanner:
    """The same tick out of library calls that existed before the fused
    kernel: torch assembles G, g0, CE, ce0, CI, ci0 for every robot, three
    batched Goldfarb-Idnani solves, torch applies the updates.  Lockstep loop
    index (one i for every robot), i > 1, inside the plan."""

    def __init__(self, rec, prm):
        import torch
        from quadrupedal_loco_amd import nlp
        self.t = torch
        self.p = prm
        self.f = {k: rec[:, a:b].clone() for k, (a, b) in nlp.STATE_FIELDS.items()}
        self.B = rec.shape[0]
        self.Wn = math.sqrt(prm.g / prm.z_c)
        self.idx = torch.arange(NS, device=rec.device)[None, :]

    def tick(self, i):
        from quadrupedal_loco_amd import qp
        t, p, f, Wn, B = self.t, self.p, self.f, self.Wn, self.B
        dt = p.dt
        period = (((i + 1) * dt > f["tx"] + 0.0001).to(t.int64).cumprod(1)).sum(1, keepdim=True)
        pi = period - 1
        at = lambda k: f[k].gather(1, pi)[:, 0]
        fx, fy, ts_p, Lxr, Lyr = at("footx_ref"), at("footy_ref"), at("ts"), at("Lxx_ref"), at("Lyy_ref")
        k_yu = i - t.round(at("tx") / dt)
        Tk = ts_p - k_yu * dt
        tr1_ref, tr2_ref = t.cosh(Wn * Tk), t.sinh(Wn * Tk)
        ref = t.stack([Lxr, Lyr, tr1_ref, tr2_ref], 1)
        v = f["vari"].clone()
        rem = p.t_min - k_yu * dt
        marg = t.where(rem >= 0.001, rem, t.full_like(rem, 0.001))
        tr1_min, tr2_min = t.cosh(Wn * marg), t.sinh(Wn * marg)
        tr1_max, tr2_max = t.cosh(Wn * (p.t_max - k_yu * dt)), t.sinh(Wn * (p.t_max - k_yu * dt))
        cxf, cvxf, cyf, cvyf = f["feed"][:, 0], f["feed"][:, 1], f["feed"][:, 3], f["feed"][:, 4]
        AxO, BxO, Cx = cxf - fx, cvxf / Wn, -0.5 * Lxr
        AyO, ByO, Cy = cyf - fy, cvyf / Wn, -0.5 * Lyr
        Axv, Bxv, Cxv = Wn * BxO, Wn * AxO, -f["endref"][:, 0]
        Ayv, Byv, Cyv = Wn * ByO, Wn * AyO, -f["endref"][:, 1]
        w = lambda a, b: p.aax * a[0] * b[0] + p.aay * a[1] * b[1] + p.aaxv * a[2] * b[2] + p.aayv * a[3] * b[3]
        A_, B_, C_ = (AxO, AyO, Axv, Ayv), (BxO, ByO, Bxv, Byv), (Cx, Cy, Cxv, Cyv)
        G = t.zeros((B, 16), dtype=t.float64, device=v.device)
        G[:, 0], G[:, 5] = p.bbx, p.bby
        G[:, 10], G[:, 15] = p.rr1 + w(A_, A_), p.rr2 + w(B_, B_)
        G[:, 11] = G[:, 14] = w(A_, B_)
        q = t.stack([-p.bbx * Lxr, -p.bby * Lyr, -p.rr1 * tr1_ref + w(A_, C_), -p.rr2 * tr2_ref + w(B_, C_)], 1)
        hw, fw = p.half_hip_width, p.foot_width
        late = i >= t.round(2 * f["ts"][:, 1] / dt) + 1
        even = (period[:, 0] % 2) == 0
        c = lambda x: t.full((B,), x, dtype=t.float64, device=v.device)
        fy_max = t.where(even, t.where(late, c(-(fw + 0.01)), c(-(hw - 0.03))), c(2 * hw + 0.03))
        fy_min = t.where(even, c(-(2 * hw + 0.03)), t.where(late, c(fw + 0.01), c(hw - 0.03)))
        sh, ch = math.sinh(Wn * dt), math.cosh(Wn * dt)
        moving = (k_yu != 0).to(t.float64)
        # rows of _A_q1 as (B, 24, 4) and what the offsets add to -(row v)
        A = t.zeros((B, 24, 4), dtype=t.float64, device=v.device)
        lim = t.zeros((B, 24), dtype=t.float64, device=v.device)
        half = t.zeros((B, 24), dtype=t.float64, device=v.device)   # block 5: offset row differs in tr2
        for r, (var, sg) in enumerate(((2, 1), (2, -1), (3, 1), (3, -1), (0, 1), (0, -1), (1, 1), (1, -1))):
            A[:, r, var] = sg
        A[:, 8:12] = A[:, 4:8] * moving[:, None, None]
        lim[:, 0:4] = t.stack([tr1_max, -tr1_min, tr2_max, -tr2_min], 1)
        lim[:, 4:8] = t.stack([c(p.footx_max), c(-p.footx_min), fy_max, -fy_min], 1)
        lim[:, 8:12] = t.stack([Lxr + p.footx_vmax * dt, -(Lxr + p.footx_vmin * dt), Lyr + p.footy_vmax * dt,
                                -(Lyr + p.footy_vmin * dt)], 1) * moving[:, None]
        blocks = ((Wn * sh * Wn, -2 * Wn * sh * Wn, 2 * Wn * Wn * ch, 0.0, 1.0, 1.0),
                  (ch * Wn, -2 * ch * Wn, 2 * Wn * sh, -2.0, dt, 1.0),
                  (Wn, -2 * Wn, 0.0, -2.0, dt, 0.5))
        for blk, (a1, a2c, a3c, a3v, scale, hf) in enumerate(blocks):
            for ax, (CC, cv, amax, amin) in enumerate(((AxO, cvxf, p.comax_max, p.comax_min),
                                                      (AyO, cvyf, p.comay_max, p.comay_min))):
                r = 12 + 4 * blk + 2 * ax
                a3 = a3c * CC + a3v * cv
                A[:, r, ax], A[:, r, 2], A[:, r, 3] = a1, a2c * CC, a3 - 2 * amax * scale
                A[:, r + 1, ax], A[:, r + 1, 2], A[:, r + 1, 3] = -a1, -a2c * CC, -(a3 - 2 * amin * scale)
                half[:, r] = -2 * amax * scale * (1 - hf)
                half[:, r + 1] = 2 * amin * scale * (1 - hf)
        CI = (-A).reshape(B, 96).contiguous()          # column i of CI = -row i, column-major 4 x 24
        gate = Tk >= 0.1 * ts_p
        sts, its = [], []
        for _ in range(3):
            g0 = (G.view(B, 4, 4) @ v[:, :, None])[:, :, 0] + q
            CE = t.stack([t.zeros_like(Lxr), t.zeros_like(Lxr), -2 * v[:, 2], 2 * v[:, 3]], 1)
            ce0 = (1 - (v[:, 2] ** 2 - v[:, 3] ** 2))[:, None]
            ci0 = -(A @ v[:, :, None])[:, :, 0] + lim + half * v[:, 3:4]
            o = qp.eiquadprog_solve(G, g0, CE, ce0.contiguous(), CI, ci0, 4, 1, 24)
            v = t.where(gate[:, None], v + o["x"], ref)
            sts.append(o["status"])
            its.append(o["iters"])
        f["vari"] = v
        ts_new = k_yu * dt + t.log(v[:, 2] + v[:, 3]) / Wn
        xi, yi = cxf - fx, cyf - fy
        vxi = (v[:, 0] * 0.5 - xi * v[:, 2]) / (1 / Wn * v[:, 3])
        vyi = (v[:, 1] * 0.5 - yi * v[:, 2]) / (1 / Wn * v[:, 3])
        for k, val in (("Lxx_ref", v[:, 0]), ("Lyy_ref", v[:, 1]), ("ts", ts_new), ("COMx_is", xi), ("COMvx_is", vxi),
                       ("COMy_is", yi), ("COMvy_is", vyi)):
            f[k].scatter_(1, pi, val[:, None])
        f["footx_ref"].scatter_(1, period, (fx + v[:, 0])[:, None])
        f["footy_ref"].scatter_(1, period, (fy + v[:, 1])[:, None])
        f["endref"] = t.stack([Wn * xi * v[:, 3] + vxi * v[:, 2], Wn * yi * v[:, 3] + vyi * v[:, 2]], 1)
        cs = t.cumsum(f["ts"], 1)
        excl = t.cat([t.zeros_like(cs[:, :1]), cs[:, :-1]], 1)         # sum of ts[0:k]
        tx_new = f["tx"].gather(1, pi) + (excl - excl.gather(1, pi))
        f["tx"] = t.where(self.idx >= period, tx_new, f["tx"])
        com = []
        for jxx in (1, 2, 3):
            cw, sw = math.cosh(Wn * dt * jxx), math.sinh(Wn * dt * jxx)
            com += [xi * cw + vxi / Wn * sw + fx, yi * cw + vyi / Wn * sw + fy, Wn * xi * sw + vxi * cw,
                    Wn * yi * sw + vyi * cw, Wn * Wn * xi * cw + vxi * Wn * sw, Wn * Wn * yi * cw + vyi * Wn * sw]
        com = t.stack(com, 1)
        f["feed"] = t.stack([com[:, 0], com[:, 2], com[:, 4], com[:, 1], com[:, 3], com[:, 5]], 1)   # lamda = 0
        bjxx = ((i * dt >= f["tx"]).to(t.int64).cumprod(1)).sum(1)
        bjx1 = (((i + 1) * dt >= f["tx"]).to(t.int64).cumprod(1)).sum(1)
        f["td"] = 0.2 * f["ts"]
        return dict(vari=v, com=com, period=period[:, 0], bjxx=bjxx, bjx1=bjx1, status=sts, iters=its)


def kernel_figures():
    """VGPRs, LDS bytes and the occupancy they allow (waves per SIMD: 512
    registers per lane and SIMD, 160 KB of LDS per CU of four SIMDs, one-wave
    workgroups) of the tick kernels, from the code object's metadata."""
    import test_kernel_resources as K
    out = {}
    for name, k in K._kernels().items():
        if "nlp_step_kernel" not in name:
            continue
        regs = k[".vgpr_count"] + k[".agpr_count"]
        lds = k[".group_segment_fixed_size"]
        alloc = -(-regs // 8) * 8
        out[name] = {"vgpr": k[".vgpr_count"], "agpr": k[".agpr_count"], "sgpr": k[".sgpr_count"],
                     "vgpr_spill": k[".vgpr_spill_count"], "scratch_bytes": k[".private_segment_fixed_size"],
                     "lds_bytes": lds, "waves_per_simd_by_registers": min(8, 512 // alloc),
                     "waves_per_simd_by_lds": min(8.0, (160 * 1024 // lds) / 4.0)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_nlp_sqp.json"))
    args = ap.parse_args()
    import torch
    from quadrupedal_loco_amd import nlp
    if not torch.cuda.is_available():
        raise SystemExit("bench_nlp needs a GPU")
    dev = torch.device("cuda:0")
    N, K = args.robots, args.steps
    rng = np.random.default_rng(20261019)
    sl = torch.from_numpy(rng.uniform(0.04, 0.09, N)).to(dev)
    sw = torch.from_numpy(2 * 0.12675 * rng.uniform(0.9, 1.1, N)).to(dev)
    pl = nlp.StepTimingPlanner(N, dev, steplength=sl, stepwidth=sw)
    z6 = torch.zeros((N, 6), dtype=torch.float64, device=dev)
    rf = torch.tensor([0.0, -0.12675], dtype=torch.float64, device=dev).expand(N, 2).contiguous()
    lf = torch.tensor([0.0, 0.12675], dtype=torch.float64, device=dev).expand(N, 2).contiguous()
    ti = [torch.full((N,), i, dtype=torch.int32, device=dev) for i in range(1, I0 + K)]
    out = None
    for i in range(1, I0):
        out = pl.tick(ti[i - 1], z6, rf, lf, out=out)
    rec0 = pl.get_state().clone()

    def fused_window():
        pl.set_state(rec0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(K):
            pl.tick(ti[I0 - 1 + k], z6, rf, lf, out=out)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / K

    def composed_window():
        cp = ComposedPlanner(rec0, pl.params)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(K):
            r = cp.tick(I0 + k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / K, cp, r

    # the composition computes the same ticks (another association of the same
    # sums: agreement to rounding, same solver outcomes)
    fused_window()
    _, cp, r = composed_window()
    got = pl.get_state()
    same_status = bool((out.pass_status[:, 2] == r["status"][2]).all().item())
    same_iters = float((out.pass_iters[:, 2] == r["iters"][2]).double().mean().item())
    d_vari = float((out.vari_ini - r["vari"]).abs().max().item())
    d_ts = float((got[:, 0:27] - cp.f["ts"]).abs().max().item())
    d_tx = float((got[:, 27:54] - cp.f["tx"]).abs().max().item())
    finite = bool(torch.isfinite(got).all().item())
    if not finite or d_vari > 1e-6 or d_ts > 1e-6 or d_tx > 1e-6:
        raise SystemExit("fused kernel and composition disagree: vari %.3e ts %.3e tx %.3e finite %s" % (
            d_vari, d_ts, d_tx, finite))
    med = lambda v: sorted(v)[len(v) // 2]
    widths = {}
    for gw in (4, 8, 16):
        prev = nlp.set_group_width(gw)
        for _ in range(max(1, args.warmup // K)):
            fused_window()
        w = sorted(fused_window() for _ in range(args.repeats))
        nlp.set_group_width(prev)
        widths[str(gw)] = {"us_per_tick": 1e3 * med(w), "us_per_tick_windows": [1e3 * x for x in w],
                           "robot_ticks_per_s": N / (med(w) * 1e-3)}
    composed_window()
    cw = sorted(composed_window()[0] for _ in range(max(3, args.repeats // 2)))
    fused = widths["4"]
    line = {"metric": "step-timing SQP, one planner tick of every resident robot (three 4 x 1 x 24 EiQuadProg "
                      "passes + updates), robot-ticks/sec (fp64)",
            "value": fused["robot_ticks_per_s"], "unit": "robot-ticks/s", "n_gpus": 1, "steps": K,
            "warmup": args.warmup, "repeats": args.repeats, "us_per_tick": fused["us_per_tick"],
            "us_per_tick_windows": fused["us_per_tick_windows"], "higher_is_better": True, "dtype": "f64",
            "data": "synthetic", "label": args.label,
            "ci_form": "stored" if os.environ.get("QLOCO_NLP_CI", "")[:1] == "s" else "generated",
            "config": {"workload": "%d robots, ticks %d..%d" % (N, I0, I0 + K - 1)},
            "group_width": widths,
            "composition": {"what": "torch assembly + 3 x qloco_eiquadprog_solve(4, 1, 24) + torch update",
                            "us_per_tick": 1e3 * med(cw), "us_per_tick_windows": [1e3 * x for x in cw],
                            "robot_ticks_per_s": N / (med(cw) * 1e-3)},
            "speedup_over_composition": med(cw) / (fused["us_per_tick"] * 1e-3),
            "agreement": {"vari_max_abs": d_vari, "ts_max_abs": d_ts, "tx_max_abs": d_tx,
                          "last_pass_status_equal": same_status, "last_pass_iters_equal_fraction": same_iters},
            "kernels": kernel_figures()}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
