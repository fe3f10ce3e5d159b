"""Input families for the body-inclination MPC (body_mpc_kernel) and the
restatement's results on them (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_oracle.py (each family's precondition on
oracle/body_mpc.c alone) and tests/test_qp_gpu.py (the same steps through
qp.BodyMPC).  A family is a run of loop counts i with the references of
test_body_mpc_matches_restatement_over_a_gait (same generator, same draw
order) and one thing changed:

  nan_reference     NaN in zmp_ref(0, 0) on every 4th robot, every step: the
                    solve runs (status OK) to a NaN solution, the !ok fallback
  tilted_reference  angle_ref ~ N(0, 1 rad): theta and torque rows active
                    on every call, the post-solve clamps taken
  nan_accel         NaN in comacc_ref(2, 1) on robots b % 4 == 1 at three
                    steps after a healthy start: G holds pth^2, the Cholesky
                    fails (NOT_PD) and _V_ini keeps its value
"""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O

OK, NOT_PD = 0, 5
BATCH = 16
STEPS = tuple(range(96, 140))  # body_theta_mpc acts from i = 100 on
NAN_ACCEL_STEPS = (110, 111, 125)
FAMILIES = ("nan_reference", "tilted_reference", "nan_accel")

_cm = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1).reshape(a.shape[0], -1))


def steps_of(name, B=BATCH, steps=STEPS, seed=11):
    """[(i, inputs of qp.BodyMPC.step)]: column-major references per robot."""
    rng = np.random.default_rng(seed)
    b = np.arange(B)
    out = []
    for i in steps:
        zmp = rng.normal(0, 0.02, (B, 2, 5))
        ang = rng.normal(0, 1.0 if name == "tilted_reference" else 0.02, (B, 2, 5))
        rf = rng.normal(0, 0.05, (B, 2, 5))
        lf = rng.normal(0, 0.05, (B, 2, 5))
        acc = rng.normal(0, 0.5, (B, 3, 5))
        bs = rng.normal(0, 0.05, (B, 4))
        if name == "nan_reference":
            zmp[b % 4 == 0, 0, 0] = np.nan
        elif name == "nan_accel":
            if i in NAN_ACCEL_STEPS:
                acc[b % 4 == 1, 2, 1] = np.nan
        elif name != "tilted_reference":
            raise KeyError(name)
        out.append((i, dict(i=np.full(B, i, np.int32), bodyangle_state=bs, zmp_ref=_cm(zmp),
                            angle_ref=_cm(ang), rfoot_ref=_cm(rf), lfoot_ref=_cm(lf), comacc_ref=_cm(acc))))
    return out


class OracleRun:
    """qo_body_theta_mpc over the steps, one PRMPCClass per robot: per step
    com_traj (B, 14), status, qp_solution, sched (bjx1, bjx2, t_yu) and
    V_before / V_after (_V_ini around the call)."""

    def __init__(self, steps):
        L = O.lib()
        B = steps[0][1]["i"].shape[0]
        states = (O.BodyState * B)()
        for s in states:
            L.qo_body_init(C.byref(s))
        self.steps = []
        for i, ins in steps:
            r = dict(com_traj=np.zeros((B, 14)), status=np.zeros(B, np.int32),
                     qp_solution=np.zeros(B, np.int32), sched=np.zeros((B, 3), np.int32),
                     V_before=np.zeros((B, 8)), V_after=np.zeros((B, 8)))
            for b in range(B):
                s = states[b]
                r["V_before"][b] = s.V_ini[:]
                ct = np.zeros(14)
                est = C.c_int(0)
                row = lambda k: O.P(np.ascontiguousarray(ins[k][b], dtype=np.float64))
                r["qp_solution"][b] = L.qo_body_theta_mpc(
                    C.byref(s), int(i), row("bodyangle_state"), row("zmp_ref"), row("angle_ref"),
                    row("rfoot_ref"), row("lfoot_ref"), row("comacc_ref"), O.P(np.zeros(9)), O.P(ct),
                    C.byref(est))
                r["com_traj"][b], r["status"][b] = ct, est.value
                r["sched"][b] = (s.bjx1, s.bjx2, s.t_yu)
                r["V_after"][b] = s.V_ini[:]
            self.steps.append(r)
        for s in states:
            L.qo_body_free(C.byref(s))


@functools.lru_cache(maxsize=None)
def family(name):
    """(steps, OracleRun) of a family, computed once and shared; read-only."""
    st = steps_of(name)
    return st, OracleRun(st)
