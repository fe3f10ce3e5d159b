"""The eight-body mix for the per-robot bodies of the Go1 force QP, the servo
force block and the servo tick (qloco_force_body, include/qloco.h section 3)
and the restatement's results on it (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_force_body.py, which asserts the mix's preconditions on
the restatement alone, and tests/test_force_body_gpu.py, which runs it through
qp.ForceQP.step(body=).  The inputs are force_cases' 64 robots and its families
`baseline`, `heavy` and `lateral` (member state carried over their ticks);
robot b takes body (b + b // 8) % 8, so every 8-robot block holds the eight
bodies and every group slot meets every body.

The restatement takes its parameters per call, so the per-robot reference is
qo_force_opt per robot with the robot's own qo_force_params.
"""
import ctypes as C
import functools

import numpy as np

import force_cases as FC
import oracle_lib as O

FIELDS = ("mass", "alpha", "beta", "gamma", "fz_max", "mu")
# overrides of the sim defaults (mass 12, alpha 1e4, beta 1e3, gamma 10, fz_max 160, mu 0.25)
MIX = (
    ("default", {}),
    ("hw_tuned", dict(mass=14.0, mu=0.5, gamma=100.0)),     # the hardware copy's mass and mu
    ("slippery", dict(mu=0.12, fz_max=130.0)),
    ("weak_legs", dict(fz_max=90.0, mass=9.0, mu=0.2)),
    ("low_alpha", dict(alpha=2000.0)),
    ("smooth", dict(beta=300.0, gamma=400.0)),
    ("payload", dict(mass=17.5, mu=0.4, fz_max=120.0)),
    ("stiff", dict(alpha=5e4, beta=2000.0, gamma=1.0, mu=0.3)),
)
FAMILIES = ("baseline", "heavy", "lateral")
BATCH = FC.BATCH
KEYS = ("grf_opt", "F_leg_guess", "F_leg_ref", "qp_solution", "status", "iters")
ERR_ARG = 100  # QLOCO_ERR_ARG


def body_of(b):
    """Index into MIX of robot b's body."""
    return (b + b // 8) % len(MIX)


def bodies(B=BATCH):
    return np.array([body_of(b) for b in range(B)])


def overrides(k):
    """qloco_force_params overrides of a uniform call with body k of the mix."""
    return dict(MIX[k][1])


def momentum_of(k):
    """Momentum_sum of body k: the reference's, scaled with the payload (the
    QP does not read it; the force block and the tick do)."""
    scale = overrides(k).get("mass", 12.0) / 12.0
    return (O.GO1_INERTIA * np.array([[scale, 1.0, 1.0], [1.0, scale, 1.0], [1.0, 1.0, 0.5 + 0.5 * scale]])).reshape(9)


def rows_of(idx):
    """(len(idx), 16) float64 rows: robot b holds body MIX[idx[b]].  Built with
    numpy alone (the product's qp.force_body_rows is under test)."""
    prm = FC.oracle_params()
    rows = np.zeros((len(idx), 16))
    for b, k in enumerate(idx):
        p = {f: getattr(prm, f) for f in FIELDS}
        p.update(overrides(int(k)))
        rows[b, :6] = [p[f] for f in FIELDS]
        rows[b, 6:15] = momentum_of(int(k))
    return rows


class PerRobotOracle:
    """The restatement tick by tick, one Dynamiccclass and one qo_force_params
    per robot.  rows: (B, >= 6) with mass .. mu in the first six columns.
    step(d, skip=None): force_distribution + force_opt on a dict of
    cases.force_inputs' arrays for every robot not in `skip`, whose members
    stay as they were (their entries of the result are the carried members)."""

    def __init__(self, rows):
        L = O.lib()
        self.B = len(rows)
        self.states = (O.DynState * self.B)()
        for s in self.states:
            L.qo_dyn_init(C.byref(s))
        self.set_rows(rows)

    def set_rows(self, rows):
        self.prms = [FC.oracle_params(**{f: float(rows[b, i]) for i, f in enumerate(FIELDS)})
                     for b in range(self.B)]

    def step(self, d, skip=None):
        L, B = O.lib(), self.B
        r = {k: np.zeros((B, 12)) for k in ("grf_before", "grf_opt", "F_leg_guess", "F_leg_ref")}
        r.update({k: np.zeros(B, np.int32) for k in ("qp_solution", "status", "iters")})
        row = lambda k, b: np.ascontiguousarray(d[k][b], dtype=np.float64)
        for b in range(B):
            s = self.states[b]
            r["grf_before"][b] = s.grf_opt[:]
            if skip is None or not skip[b]:
                L.qo_force_distribution(C.byref(s), O.P(row("com_des", b)), O.P(row("leg_des", b)),
                                        O.P(row("F_force_des", b)), int(d["mode"][b]),
                                        float(d["y_coef"][b]), O.P(row("rfoot_des", b)),
                                        O.P(row("lfoot_des", b)))
                fe = [np.ascontiguousarray(d["feet_p"][b, 3 * l:3 * l + 3], dtype=np.float64) for l in range(4)]
                est, eit = C.c_int(0), C.c_int(0)
                ok = L.qo_force_opt(C.byref(s), C.byref(self.prms[b]), O.P(row("base_p", b)), *[O.P(f) for f in fe],
                                    O.P(row("FT_total_des", b)), int(d["mode"][b]),
                                    int(d["right_support"][b]), float(d["y_coef"][b]),
                                    C.byref(est), C.byref(eit))
                r["qp_solution"][b], r["status"][b], r["iters"][b] = ok, est.value, eit.value
            r["grf_opt"][b], r["F_leg_guess"][b], r["F_leg_ref"][b] = s.grf_opt[:], s.F_leg_guess[:], s.F_leg_ref[:]
        return r

    def close(self):
        for s in self.states:
            O.lib().qo_dyn_free(C.byref(s))


class PerRobotRun:
    """PerRobotOracle over a list of ticks (FC.OracleRun with per-robot
    parameters): .ticks[t] = the dict grf_before, grf_opt, F_leg_guess,
    F_leg_ref, qp_solution, status, iters."""

    def __init__(self, ticks, rows):
        orc = PerRobotOracle(rows)
        self.ticks = [orc.step(d) for d, _ in ticks]
        orc.close()


@functools.lru_cache(maxsize=None)
def mix(name):
    """(ticks, bodies (64,), rows (64, 16), PerRobotRun) of the mix on a
    family, computed once per test run and shared; read-only."""
    assert name in FAMILIES
    ticks = FC.ticks_of(name)
    idx = bodies()
    rows = rows_of(idx)
    return ticks, idx, rows, PerRobotRun(ticks, rows)


def derangement(B=BATCH):
    """A permutation p (new position i holds robot p[i]) under which no robot
    keeps its group slot (position mod 8 and mod 16 both change) and no 4- or
    8-robot block keeps its set of robots: robot b moves to position
    (5 b + 3) mod B (B a multiple of 16, gcd(5, B) = 1)."""
    assert B % 16 == 0
    new_pos = (5 * np.arange(B) + 3) % B
    p = np.empty(B, np.int64)
    p[new_pos] = np.arange(B)
    return p


# the rows the device must refuse (field, value), scattered into the mix
REFUSED = (("mass", np.nan), ("mass", 0.0), ("mu", -0.1), ("fz_max", np.inf), ("alpha", -1.0))
REFUSED_AT = (0, 7, 8, 29, 63)  # a block's first and last slot at both widths, the last robot


SERVO_MASS = (12.0, 14.0, 10.5, 9.0, 13.25, 11.0, 17.5, 15.75)   # per body of the mix, for F_sum


def servo_rows(B):
    """Masses and momenta mixed over B robots for the force block and the tick:
    robot b holds body b % 8 of the mix with SERVO_MASS[b % 8] and the momentum
    scaled by it (body 0: the constants, 12 and Momentum_sum)."""
    k = np.arange(B) % len(MIX)
    rows = rows_of(k)
    m = np.array(SERVO_MASS)[k]
    rows[:, 0] = m
    rows[:, 6:15] = O.GO1_INERTIA.reshape(9) * np.stack([m / 12.0, np.ones(B), np.ones(B), np.ones(B), 0.5 + m / 24.0,
                                                        np.ones(B), np.ones(B), np.ones(B), m / 12.0], 1)
    return rows


def block_as_force_inputs(d, F_sum, Force_L_R):
    """The force QP's inputs as the force block and the tick pass them
    (servo.cpp:1216-1228), from the block's inputs and its F_sum / Force_L_R."""
    return dict(com_des=d["body_p_des"], leg_des=d["foot_des"], F_force_des=Force_L_R, rfoot_des=d["rfoot_des"],
                lfoot_des=d["lfoot_des"], base_p=d["body_p_des"], feet_p=d["foot_des"], FT_total_des=F_sum,
                mode=d["gait_mode"], right_support=d["right_support"], y_coef=d["y_offset"])


def f_sum_numpy(rows, coma):
    """F_sum of include/qloco.h section 7 in its operation order, no fused
    multiply-add: numpy evaluates each product and sum in fp64 separately."""
    m = rows[:, 0]
    M = rows[:, 6:15].reshape(-1, 3, 3)
    out = np.zeros((len(rows), 6))
    out[:, 0] = m * coma[:, 0]
    out[:, 1] = m * coma[:, 1]
    out[:, 2] = m * 9.8 + m * coma[:, 2]
    for i in range(3):
        out[:, 3 + i] = (M[:, i, 0] * coma[:, 0] + M[:, i, 1] * coma[:, 1]) + M[:, i, 2] * coma[:, 2]
    return out


def force_lr_numpy(F_sum, com, rfoot, lfoot, rs):
    """F_lr_predict (servo.cpp:1097-1209) from F_sum, in servo_glue_kernel's
    operation order."""
    v = lfoot - rfoot
    c = com - rfoot
    dis = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    dot = (v[:, 0] * c[:, 0] + v[:, 1] * c[:, 1]) + v[:, 2] * c[:, 2]
    raw = dot / dis
    raw1 = np.where(1.0 < raw, 1.0, raw)
    k = np.where(raw1 < 0.0, 0.0, raw1)
    F = np.zeros((len(F_sum), 6))
    for j in range(3):
        a = F_sum[:, j] * k
        F[:, j] = np.where(rs == 0, F_sum[:, j], np.where(rs == 1, 0.0, a))
        F[:, 3 + j] = np.where(rs == 0, 0.0, np.where(rs == 1, F_sum[:, j], F_sum[:, j] - a))
    return F
