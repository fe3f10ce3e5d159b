"""Dump the full outputs of a fixed list of SRBD batches -- one batch or more
per kernel instantiation of qloco_srbd.hip (one-wave, two-wave buckets, the
wide kernel), qloco_srbd_lit.hip and qloco_srbd_build.hip -- for a
bit-identity comparison of two library builds (QLOCO_LIB, tools/variant_lib.py),
as tools/lit_dump_out.py does for one literal batch.

    [QLOCO_LIB=...] python tools/srbd_dump_out.py dump OUTDIR
    python tools/srbd_dump_out.py compare DIR_A DIR_B      (exit 1 on a difference)

Solve cases write u, u0, iters, status, rho_updates, obj (warm and persistent
cases: of the second call, and the warm buffer / record); build cases write H,
g, lb, ub, Aqp, Bqp."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SEED = 20261015
OUT_KEYS = ("u", "u0", "iters", "status", "rho_updates", "obj")
# name: (N, B, gait, mode, spec overrides); the comment names the kernel reached
CASES = [
    # the literal QP through the wrench space
    ("lit_n10_trot_headline", 10, 4096, "trot", "solve", dict(literal_full_qp=1)),  # srbd_lit_kernel<false>
    ("lit_n7_mixed", 7, 2048, "mixed", "solve", dict(literal_full_qp=1)),
    ("lit_n16_trot", 16, 4096, "trot", "solve", dict(literal_full_qp=1)),  # srbd_lit2_kernel<false>
    ("lit_n10_trot_fzmin10", 10, 4096, "trot", "solve", dict(literal_full_qp=1, fz_min=10.0, fz_max=180.0)),
    ("lit_n10_trot_persist", 10, 256, "trot", "persist", dict(literal_full_qp=1)),  # srbd_lit_kernel<true>
    ("lit_n16_trot_persist", 16, 64, "trot", "persist", dict(literal_full_qp=1)),  # srbd_lit2_kernel<true>
    # the stance-only reduction: one wave
    ("red_n10_trot", 10, 4096, "trot", "solve", {}),  # <1, 4, false, 10>
    ("red_n10_mixed", 10, 4096, "mixed", "solve", {}),  # <1, 4, false, 10> + two-wave buckets
    ("red_n20_mixed_small", 20, 2048, "mixed", "solve", {}),  # <1, 2, false, 20>, two-wave, wide
    ("red_n20_mixed_large", 20, 8192, "mixed", "solve", {}),  # <1, 3, false, 20>, two-wave, wide
    # two waves: buckets C2 = 3 / 6 / 9 / 15
    ("red_n11_trot", 11, 512, "trot", "solve", {}),
    ("red_n13_trot", 13, 512, "trot", "solve", {}),
    ("red_n16_trot", 16, 4096, "trot", "solve", {}),
    ("red_n20_pace", 20, 2048, "pace", "solve", {}),
    # the wide kernel: HC = 96 / 112 / 120
    ("red_n12_stance", 12, 256, "stance", "solve", {}),
    ("red_n17_stance", 17, 128, "stance", "solve", {}),
    ("red_n20_stance", 20, 128, "stance", "solve", {}),
    # warm start (second call) and the persistent solver (second tick) per family
    ("warm_n10_trot", 10, 512, "trot", "warm", {}),  # <1, 4, true, 10>
    ("warm_n20_mixed_small", 20, 512, "mixed", "warm", {}),  # <1, 2, true, 20>, <2, 2, true, 20, 15>, big<true, 128>
    ("warm_n20_mixed_large", 20, 6400, "mixed", "warm", {}),  # <1, 3, true, 20>
    ("warm_n16_trot", 16, 256, "trot", "warm", {}),
    ("warm_n12_stance", 12, 64, "stance", "warm", {}),
    ("persist_n10_trot", 10, 512, "trot", "persist", {}),
    ("persist_n16_trot", 16, 256, "trot", "persist", {}),
    ("persist_n12_stance", 12, 64, "stance", "persist", {}),
    # per-step feet, one per family (tests/test_srbd_gpu.py:
    # test_srbd_per_step_feet_reach_every_solve_kernel)
    ("fps_n3_trot", 3, 8, "trot", "fps", {}),
    ("fps_n11_trot", 11, 4, "trot", "fps", {}),
    ("fps_n11_stance", 11, 2, "stance", "fps", {}),
    ("fps_n3_trot_literal", 3, 4, "trot", "fps", dict(literal_full_qp=1)),
    # the dense build
    ("build_n10_trot", 10, 64, "trot", "build", {}),
    ("build_n20_pace", 20, 16, "pace", "build", {}),
    ("build_n10_mixed_fps", 10, 64, "mixed", "build_fps", {}),
]


def jitter(ft, N):
    rng = np.random.default_rng(9)
    return (np.tile(ft, (1, N)) + rng.uniform(-0.02, 0.02, (len(ft), 12 * N))).astype(np.float32)


def dump(outdir):
    import torch
    from quadrupedal_loco_amd import srbd
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda:0")
    d = lambda arrs: [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]
    for name, N, B, gait, mode, spec in CASES:
        res = {}
        if mode == "persist":
            seq = srbd.control_loop_sequence(SEED, N, B, 2, gait)
            s = srbd.PersistentConvexMpc(B, dev, horizon=N, **spec)
            for tick in seq:
                r = s.solve(*d(tick), full=True)
            res["record"] = s.record
        else:
            x0, xr, ft, ct = srbd.generate(SEED, N, B, gait)
            if mode in ("fps", "build_fps"):
                ft = jitter(ft, N)
            args = d((x0, xr, ft, ct))
            if mode in ("build", "build_fps"):
                res = srbd.BatchedConvexMpc(horizon=N, **spec).build(*args, want=("H", "g", "lb", "ub", "Aqp", "Bqp"))
            elif mode == "warm":
                warm = torch.zeros((B, 32 * N), dtype=torch.float32, device=dev)
                s = srbd.BatchedConvexMpc(horizon=N, warm_start=1, **spec)
                s.solve(*args, full=True, warm=warm)
                r = s.solve(*args, full=True, warm=warm)
                res["warm"] = warm
            else:
                r = srbd.BatchedConvexMpc(horizon=N, **spec).solve(*args, full=True)
        if not mode.startswith("build"):
            res.update({k: getattr(r, k) for k in OUT_KEYS})
        torch.cuda.synchronize()
        np.savez(os.path.join(outdir, name + ".npz"), **{k: v.cpu().numpy() for k, v in res.items()})
        print("dumped", name, flush=True)


def compare(da, db):
    bad = 0
    for name, N, B, gait, mode, spec in CASES:
        a, b = (np.load(os.path.join(p, name + ".npz")) for p in (da, db))
        print("%s (N = %d, B = %d, %s%s%s)" % (name, N, B, gait, ", " + mode if mode != "solve" else "",
                                            "".join(", %s=%s" % kv for kv in spec.items())))
        for k in sorted(a.files):
            same = a[k].tobytes() == b[k].tobytes()
            bad += not same
            extra = ""
            if k == "iters":
                extra = "  iters mean %.1f max %d, status != 0: %d" % (a[k].mean(), a[k].max(), int((a["status"] != 0).sum()))
            print("  %-11s %s (%d B)%s" % (k, "identical" if same else "DIFFERS", a[k].nbytes, extra))
    print("every output identical" if not bad else "%d arrays differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
