"""Records tests/golden/srbd_lit_parent_bits.npz: every output of the one-wave
literal SRBD kernels (u0, u, status, iters, rho_updates, obj), byte for byte,
as the library of the commit BEFORE the matrix-core Gauss-Jordan computed them
on an MI355X.  tests/test_srbd_lit_mfma_gj_gpu.py asserts byte equality with
it: the inverse moved to other instructions and another register layout and
must still perform the same fused multiply-adds in the same order.

Run with the parent's library (needs a GPU):

    python tools/variant_lib.py parent --rev <parent commit>
    QLOCO_LIB=tools/_var/parent/libqloco.so python tests/golden/make_srbd_lit_parent_bits.py [OUT.npz]

The cases and how each is run live here (CASES, run_case) and the test imports
them, so recording and checking cannot drift apart.  Every case is one launch
of B = 64 instances (the persistent one: two), placement off.  A case's seed
is the first of SEED, SEED + 1, ... whose recorded outputs meet the
preconditions the test asserts (preconditions()); it is stored in the fixture.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "srbd_lit_parent_bits.npz")
SEED = 20261015
B = 64
FIELDS = ("u0", "u", "status", "iters", "rho_updates", "obj")

# name: (N, gait, kind); kind: cold | fz (fz_min > 0) | persistent (two ticks, the
# warm-start instantiation) | rows (per-robot model rows: the _rows kernel)
CASES = {
    "n10_trot": (10, "trot", "cold"),        # nc = 60: every pivot, both accumulator halves
    "n6_mixed": (6, "mixed", "cold"),        # nc = 36: pivots cross lane 32
    "n5_trot": (5, "trot", "cold"),          # nc = 30: the second half is padding only
    "n3_mixed": (3, "mixed", "cold"),        # nc = 18
    "n1_trot": (1, "trot", "cold"),          # nc = 6
    "n10_trot_fz": (10, "trot", "fz"),
    "n10_trot_persistent": (10, "trot", "persistent"),
    "n10_trot_rows": (10, "trot", "rows"),
}
FZ = dict(fz_min=10.0, fz_max=180.0)


def run_case(name, seed):
    """The case's outputs as host arrays, {field or field_tick1: array}."""
    import torch

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from quadrupedal_loco_amd import srbd

    N, gait, kind = CASES[name]
    dev = torch.device("cuda:0")

    def to_dev(host):
        return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host]

    def host_out(out, suffix=""):
        torch.cuda.synchronize()
        return {k + suffix: getattr(out, k).cpu().numpy() for k in FIELDS}

    if kind == "persistent":
        solver = srbd.PersistentConvexMpc(B, dev, horizon=N, literal_full_qp=1)
        assert srbd.route(solver.spec) == 1
        res = {}
        for t, host in enumerate(srbd.control_loop_sequence(seed, N, B, 2, gait)):
            res.update(host_out(solver.solve(*to_dev(host), full=True), "_tick%d" % t if t else ""))
        return res
    solver = srbd.BatchedConvexMpc(horizon=N, literal_full_qp=1, placement=False, **(FZ if kind == "fz" else {}))
    assert srbd.route(solver.spec) == 1  # the one-wave literal kernel
    model = None
    if kind == "rows":
        rows = srbd.model_rows(B, solver.spec, mass=np.linspace(9.0, 16.0, B), mu=np.linspace(0.4, 0.8, B),
                               fz_max=np.linspace(150.0, 220.0, B))
        model = torch.from_numpy(rows).to(dev)
    return host_out(solver.solve(*to_dev(srbd.generate(seed, N, B, gait)), full=True, model=model))


def preconditions(name, res):
    """What the fixture must show for the case to exercise the inverse (None if
    it does, else the reason); judged on the recorded outputs alone."""
    N = CASES[name][0]
    ok = (res["status"] == 0).mean()
    if ok < 0.9:
        return "status == 0 on %.0f %% of the instances" % (100 * ok)
    if N >= 3:
        if not (res["rho_updates"] >= 1).any():
            return "no instance with a rho update (no refactorisation ran)"
        if len(np.unique(res["iters"])) < 3:
            return "fewer than three distinct iteration counts"
    return None


def main():
    sys.path.insert(0, ROOT)
    from quadrupedal_loco_amd import _lib
    print("library:", _lib.LIB_PATH)
    store = {}
    for name in CASES:
        for seed in range(SEED, SEED + 16):
            res = run_case(name, seed)
            why = preconditions(name, res)
            print("%-20s seed %d: %s; iters %d..%d (%d distinct), rho updates on %d, status 0 on %d of %d" % (
                name, seed, why or "ok", res["iters"].min(), res["iters"].max(), len(np.unique(res["iters"])),
                int((res["rho_updates"] >= 1).sum()), int((res["status"] == 0).sum()), B))
            if why is None:
                break
        else:
            raise SystemExit("%s: no seed meets the preconditions" % name)
        store[name + "/seed"] = np.int64(seed)
        for k, v in res.items():
            store[name + "/" + k] = v
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(path, **store)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
