"""Input families for the Go1 force-distribution QP (force_qp_kernel and its
callers) and the restatement's results on them (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_oracle.py, which asserts each family's precondition on
the restatement alone (oracle/force_qp.c), and tests/test_qp_gpu.py, which
runs the same ticks through qp.ForceQP.  Every family is a short run of
ticks of cases.force_inputs (member state carried from tick to tick) with one
thing changed; a tick is (inputs, parameter overrides).

  baseline      force_inputs unchanged
  heavy         vertical demand x 4: legs reach fz_max
  lateral       + 80 N in x: friction rows active
  bad_position  tick 1: base_p[:, 0] NaN (b % 4 == 1) or +Inf (b % 4 == 3)
                -> Cholesky fails, grf_opt keeps its value
  zero_weights  tick 1: alpha = beta = gamma = 0 -> G = 0, fails on every robot
  alpha0        alpha = 0: G diagonal, closed form where the blend is feasible
  nan_demand    tick 0: NaN in one entry of FT_total_des on every 4th robot
                (the array force_inputs also passes as F_force_des)
  odd_flags     tick 1: mode in {0, 100, 104}, right_support in {-1, 3}
  hw_heavy, hw_lateral   heavy / lateral with the hardware copy's mass 14, mu 0.5

The failing ticks come second, after a healthy one, so that "grf_opt
unchanged" is a non-zero vector; a healthy third tick shows the carry.
"""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
from cases import force_inputs

OK, NOT_PD = 0, 5  # qloco_status
SEED, BATCH = 3, 64
FAMILIES = ("baseline", "heavy", "lateral", "bad_position", "zero_weights", "alpha0", "nan_demand",
            "odd_flags", "hw_heavy", "hw_lateral")
HW = dict(mass=14.0, mu=0.5)


def _inputs(rng, B):
    """force_inputs with every array its own (it passes one array as com_des
    and base_p, and one as F_force_des and FT_total_des)."""
    return {k: np.array(v) for k, v in force_inputs(rng, B).items()}


def heavy(d):
    d["F_force_des"][:, 2] *= 4.0
    d["FT_total_des"][:, 2] *= 4.0
    return d


def lateral(d):
    d["F_force_des"][:, 0] += 80.0
    d["FT_total_des"][:, 0] += 80.0
    return d


def bad_rows(B, kind="bad_position"):
    """Robots a failing tick hits: (NaN rows, +Inf rows) for bad_position,
    (NaN rows, none) for nan_demand."""
    b = np.arange(B)
    if kind == "nan_demand":
        return b[b % 4 == 0], b[:0]
    return b[b % 4 == 1], b[b % 4 == 3]


def bad_position(d, rows_nan=None, rows_inf=None):
    B = d["base_p"].shape[0]
    n, i = bad_rows(B)
    d["base_p"][n if rows_nan is None else rows_nan, 0] = np.nan
    d["base_p"][i if rows_inf is None else rows_inf, 0] = np.inf
    return d


def nan_demand(d, rows=None):
    """One entry (robot b: entry b % 6) of FT_total_des and, as in
    force_inputs where the two are one array, of F_force_des."""
    B = d["FT_total_des"].shape[0]
    rows = bad_rows(B, "nan_demand")[0] if rows is None else np.asarray(rows)
    d["FT_total_des"][rows, rows % 6] = np.nan
    d["F_force_des"][rows, rows % 6] = np.nan
    return d


def odd_flags(d):
    B = d["mode"].shape[0]
    b = np.arange(B)
    d["mode"] = np.array([0, 100, 104], np.int32)[b % 3]
    d["right_support"] = np.array([-1, 3], np.int32)[(b // 3) % 2]
    return d


def ticks_of(name, seed=SEED, B=BATCH, ticks=None):
    """[(inputs, parameter overrides)] of a family, ticks drawn in order from
    one generator (so tick t's healthy part is the same in every family)."""
    rng = np.random.default_rng(seed)
    hw = dict(HW) if name.startswith("hw_") else {}
    base = name[3:] if hw else name
    n = ticks or (3 if base in ("bad_position", "zero_weights", "nan_demand", "odd_flags") else 2)
    out = []
    for t in range(n):
        d, prm = _inputs(rng, B), dict(hw)
        if base == "heavy":
            heavy(d)
        elif base == "lateral":
            lateral(d)
        elif base == "bad_position" and t == 1:
            bad_position(d)
        elif base == "zero_weights" and t == 1:
            prm.update(alpha=0.0, beta=0.0, gamma=0.0)
        elif base == "alpha0":
            prm.update(alpha=0.0)
        elif base == "nan_demand" and t == 0:
            nan_demand(d)
        elif base == "odd_flags" and t == 1:
            odd_flags(d)
        elif base not in ("baseline", "bad_position", "zero_weights", "nan_demand", "odd_flags"):
            raise KeyError(name)
        out.append((d, prm))
    return out


def oracle_params(**over):
    prm = O.ForceParams()
    O.lib().qo_force_params_default(C.byref(prm))
    for k, v in over.items():
        setattr(prm, k, v)
    return prm


class OracleRun:
    """The restatement over a list of ticks, one Dynamiccclass per robot:
    per tick the dict grf_before, grf_opt, F_leg_guess, F_leg_ref (12 each),
    qp_solution, status, iters."""

    def __init__(self, ticks):
        L = O.lib()
        B = ticks[0][0]["mode"].shape[0]
        states = (O.DynState * B)()
        for s in states:
            L.qo_dyn_init(C.byref(s))
        self.ticks = []
        for d, over in ticks:
            prm = oracle_params(**over)
            r = {k: np.zeros((B, 12)) for k in ("grf_before", "grf_opt", "F_leg_guess", "F_leg_ref")}
            r.update({k: np.zeros(B, np.int32) for k in ("qp_solution", "status", "iters")})
            row = lambda k, b: np.ascontiguousarray(d[k][b], dtype=np.float64)
            for b in range(B):
                s = states[b]
                r["grf_before"][b] = s.grf_opt[:]
                L.qo_force_distribution(C.byref(s), O.P(row("com_des", b)), O.P(row("leg_des", b)),
                                        O.P(row("F_force_des", b)), int(d["mode"][b]),
                                        float(d["y_coef"][b]), O.P(row("rfoot_des", b)),
                                        O.P(row("lfoot_des", b)))
                fe = [np.ascontiguousarray(d["feet_p"][b, 3 * l:3 * l + 3], dtype=np.float64) for l in range(4)]
                est, eit = C.c_int(0), C.c_int(0)
                ok = L.qo_force_opt(C.byref(s), C.byref(prm), O.P(row("base_p", b)), *[O.P(f) for f in fe],
                                    O.P(row("FT_total_des", b)), int(d["mode"][b]),
                                    int(d["right_support"][b]), float(d["y_coef"][b]),
                                    C.byref(est), C.byref(eit))
                r["grf_opt"][b], r["F_leg_guess"][b], r["F_leg_ref"][b] = s.grf_opt[:], s.F_leg_guess[:], s.F_leg_ref[:]
                r["qp_solution"][b], r["status"][b], r["iters"][b] = ok, est.value, eit.value
            self.ticks.append(r)
        for s in states:
            L.qo_dyn_free(C.byref(s))


@functools.lru_cache(maxsize=None)
def family(name, seed=SEED, B=BATCH):
    """(ticks, OracleRun) of a family, computed once and shared; read-only."""
    t = ticks_of(name, seed, B)
    return t, OracleRun(t)


def pattern(mode, rs):
    """The swing-leg equality pattern of (mode, right_support), 0 = no rows."""
    return np.where(mode == 102, np.where(rs == 0, 1, np.where(rs == 1, 2, 0)),
                    np.where(mode == 101, np.where(rs == 0, 3, np.where(rs == 1, 4, 0)), 0))


ZERO_LEGS = {0: (), 1: (1, 2), 2: (0, 3), 3: (0, 2), 4: (1, 3)}  # dynmics_compute.cpp:310-350


def active_rows(grf, fz_max, mu, tol=1e-7):
    """Per robot: legs at fz_max, legs at fz = 0, friction rows at equality
    (|fx| or |fy| = mu fz with fz > tol), counted over the four legs."""
    g = grf.reshape(-1, 4, 3)
    fz = g[:, :, 2]
    top = np.sum(np.abs(fz - fz_max) <= tol, axis=1)
    zero = np.sum(np.abs(fz) <= tol, axis=1)
    fr = np.sum((np.abs(np.abs(g[:, :, :2]) - mu * fz[:, :, None]) <= tol) & (fz[:, :, None] > tol), axis=(1, 2))
    return top, zero, fr


def alpha0_closed_form(d, over, r):
    """alpha = 0: G = 2 (beta + gamma) I, so the QP is the projection of
    blend = (beta F_leg_guess + gamma grf_before) / (beta + gamma) onto the
    constraint set.  Where the blend, its swing legs zeroed (the equality
    rows fix single coordinates), satisfies every inequality, it is the
    solution; where it does not, the friction pyramid couples fx, fy and fz
    and there is no clip: those robots are left to parity.  Returns (x, rows
    where it applies)."""
    prm = oracle_params(**over)
    x = (prm.beta * r["F_leg_guess"] + prm.gamma * r["grf_before"]) / (prm.beta + prm.gamma)
    pat = pattern(d["mode"], d["right_support"])
    for b in range(x.shape[0]):
        for leg in ZERO_LEGS[int(pat[b])]:
            x[b, 3 * leg:3 * leg + 3] = 0.0
    g = x.reshape(-1, 4, 3)
    fz = g[:, :, 2]
    ok = np.all((fz >= 0) & (fz <= prm.fz_max) & (np.abs(g[:, :, 0]) <= prm.mu * fz) &
                (np.abs(g[:, :, 1]) <= prm.mu * fz), axis=1)
    return x, np.flatnonzero(ok)
