"""A1 single-step force QP (A1RobotControl::compute_grf, stance_leg_control_type
== 0; A1RobotControl.cpp:383-450, ctor :8-49) -- CPU tests: the oracle's build
against an independent numpy transcription of the reference lines, its OSQP
restatement against the exact optimum (EiQuadProg restatement), the committed
golden fixture, and the C ABI's defaults / argument checks (no device work).
Parity with the reference binary is unpinned (OsqpEigen / Eigen / ROS absent,
SURVEY.md §8c)."""
import ctypes as C
import os

import numpy as np
import pytest

import a1qp_cases as AC
import oracle_lib as O
from quadrupedal_loco_amd import _lib, a1qp

HERE = os.path.dirname(os.path.abspath(__file__))


def np_a1_build(s, ct, kp_l=(1000., 1000., 1000.), kd_l=(200., 70., 120.),
                kp_a=(650., 35., 1.), kd_a=(4.5, 4.5, 30.), mass=15.0,
                Q=(1., 1., 1., 400., 400., 100.), R_w=1e-3, mu=0.7, fmin=0.0, fmax=180.0):
    """Independent numpy restatement of A1RobotControl.cpp:330-419."""
    s = np.asarray(s, np.float64)
    pos, pos_d, eul, eul_d = s[0:3], s[3:6], s[6:9], s[9:12]
    lv, lv_d, av, av_d = s[12:15], s[15:18], s[18:21], s[21:24]
    R = s[24:33].reshape(3, 3).T
    Rz = s[33:42].reshape(3, 3).T
    feet = s[42:54].reshape(4, 3)
    ee = eul_d - eul
    if ee[2] > 3.1415926 * 1.5:
        ee[2] = eul_d[2] - 3.1415926 * 2 - eul[2]
    elif ee[2] < -3.1415926 * 1.5:
        ee[2] = eul_d[2] + 3.1415926 * 2 - eul[2]
    acc = np.zeros(6)
    acc[:3] = np.asarray(kp_l) * (pos_d - pos) + R @ (np.asarray(kd_l) * (lv_d - R.T @ lv))
    acc[3:] = np.asarray(kp_a) * ee + np.asarray(kd_a) * (av_d - R.T @ av)
    acc[2] += mass * 9.8
    inv = np.zeros((6, 12))
    for i in range(4):
        f = feet[i]
        S = np.array([[0, -f[2], f[1]], [f[2], 0, -f[0]], [-f[1], f[0], 0]])
        inv[0:3, 3 * i:3 * i + 3] = np.eye(3)
        inv[3:6, 3 * i:3 * i + 3] = Rz.T @ S
    H = R_w * np.eye(12) + inv.T @ np.diag(Q) @ inv
    g = -inv.T @ np.diag(Q) @ acc
    A = np.zeros((20, 12))
    l, u = np.zeros(20), np.zeros(20)
    for i in range(4):
        A[i, 2 + 3 * i] = 1
        r0 = 4 + 4 * i
        A[r0, 3 * i], A[r0, 2 + 3 * i] = 1, -mu
        A[r0 + 1, 3 * i], A[r0 + 1, 2 + 3 * i] = -1, -mu
        A[r0 + 2, 1 + 3 * i], A[r0 + 2, 2 + 3 * i] = 1, -mu
        A[r0 + 3, 1 + 3 * i], A[r0 + 3, 2 + 3 * i] = -1, -mu
        c = 1.0 if ct[i] else 0.0
        l[i], u[i] = c * fmin, c * fmax
        l[r0:r0 + 4] = -1e30
    return acc, H, g, A, l, u


def test_a1_oracle_build_matches_numpy_transcription():
    S, CT = a1qp.synth_states(5, 64)
    wrapped = 0
    for b in range(64):
        got = O.a1_build(S[b], CT[b])
        ref = np_a1_build(S[b], CT[b])
        for x, y in zip(got, ref):
            assert np.allclose(x, y, rtol=1e-12, atol=1e-9), b
        assert np.array_equal(got[1], got[1].T)   # OSQP reads triu(P): exactly symmetric
        wrapped += abs(S[b, 11] - S[b, 8]) > 3.1415926 * 1.5
    assert wrapped >= 8  # the yaw-error wrap of :333-337 is exercised


def test_a1_oracle_admm_reaches_exact_optimum():
    """OSQP-algorithm restatement vs the exact optimum of the same QP: inside
    the default-eps band, and converged at eps 1e-9."""
    S, CT = a1qp.synth_states(6, 48)
    for b in range(48):
        acc, H, g, A, l, u = O.a1_build(S[b], CT[b])
        xe = np.zeros(12)
        it = C.c_int()
        assert O.lib().qo_exact_solve(12, 20, O.P(np.asfortranarray(H).ravel("F")), O.P(g),
                                      O.P(np.asfortranarray(A).ravel("F")), O.P(l), O.P(u),
                                      O.P(xe), C.byref(it)) == 0
        fe = 0.5 * xe @ H @ xe + g @ xe
        sc = max(1.0, abs(fe))
        f, x, info = O.a1_compute_grf(S[b], CT[b])
        assert info.status == 0
        fo = 0.5 * x @ H @ x + g @ x
        assert -1e-2 * sc <= fo - fe <= 5e-2 * sc, (b, fo, fe)
        f9, x9, info9 = O.a1_compute_grf(S[b], CT[b], eps_abs=1e-9, eps_rel=1e-9, max_iter=50000)
        assert np.abs(x9 - xe).max() <= 1e-3 * max(1.0, np.abs(xe).max()), b
        # swing legs carry no force; body-frame forces are R^T x per leg
        for i in range(4):
            if not CT[b, i]:
                assert np.abs(x9[3 * i:3 * i + 3]).max() <= 1e-6
        R = S[b, 24:33].reshape(3, 3).T
        assert np.allclose(f9.reshape(4, 3), (R.T @ x9.reshape(4, 3).T).T, atol=1e-12)


def test_a1_golden_fixture():
    z = np.load(os.path.join(HERE, "golden", "a1_qp.npz"))
    for b in range(len(z["state"])):
        f, x, info = O.a1_compute_grf(z["state"][b], z["contacts"][b])
        assert np.array_equal(f, z["forces"][b]), b
        assert info.iters == z["iters"][b] and info.status == z["status"][b]


def test_a1_capi_defaults_and_argument_checks():
    p = a1qp.default_params()
    o = O.a1_params()
    for k in ("kp_linear", "kd_linear", "kp_angular", "kd_angular", "q_diag"):
        assert list(getattr(p, k)) == list(getattr(o, k)), k
    for k in ("robot_mass", "r", "mu", "f_min", "f_max"):
        assert getattr(p, k) == getattr(o, k), k
    assert (p.rho, p.sigma, p.alpha, p.eps_abs, p.eps_rel) == (0.1, 1e-6, 1.6, 1e-3, 1e-3)
    assert (p.max_iter, p.check_termination, p.scaling, p.adaptive_rho) == (4000, 25, 10, 1)
    L = _lib.lib()
    assert L.qloco_a1_qp_solve(None, 1, *([None] * 9)) == 100
    assert L.qloco_a1_qp_solve(C.byref(p), -1, *([None] * 9)) == 100
    assert L.qloco_a1_qp_solve(C.byref(p), 0, *([None] * 9)) == 0
    assert L.qloco_a1_qp_solve(C.byref(p), 4, *([None] * 9)) == 100
    bad = a1qp.default_params(max_iter=0)
    d = [C.c_void_p(16)] * 3
    assert L.qloco_a1_qp_solve(C.byref(bad), 4, *d, *([None] * 6)) == 100


# ---------------------------------------------------------------- off the defaults (tests/a1qp_cases.py)
NP_NAMES = dict(kp_linear="kp_l", kd_linear="kd_l", kp_angular="kp_a", kd_angular="kd_a",
                robot_mass="mass", q_diag="Q", r="R_w", mu="mu", f_min="fmin", f_max="fmax")
BODY_CASES = [k for k, ov in AC.CASES.items() if any(f in AC.BODY_FIELDS for f in ov)]


def test_a1qp_cases_cover_what_they_claim():
    """Preconditions of the case table, on the restatement alone: a solving
    case spreads over >= 3 iteration counts and adapts rho on some robot (so
    the termination check and the refactorisation both run at several
    iterations), the two max_iter exits end on and off a check iteration and
    split into both failure statuses, the never-checking solve runs to
    max_iter, and the edge contact patterns are in every batch."""
    assert BODY_CASES and set(BODY_CASES) < set(AC.CASES)
    for name in AC.CASES:
        S, CT, ov, ref, _ = AC.case(name)
        assert np.array_equal(CT[:len(AC.EDGE_CONTACTS)], AC.EDGE_CONTACTS)
        assert np.all(np.isfinite(ref["forces"])), name
        # the all-swing robot: f_z within eps of 0 and |f_x|, |f_y| <= mu f_z + eps at the first check
        assert ref["status"][0] == (AC.OK if AC.check_interval(ov) else AC.SOLVED_INACCURATE), name
        assert np.abs(ref["qp_solution"][0]).max() <= 3 * ov.get("eps_abs", 1e-3), name
        if name in AC.SOLVING:
            assert np.all(ref["status"] == AC.OK), name
            assert len(np.unique(ref["iters"])) >= 3, name
            if ov.get("adaptive_rho", 1):
                assert ref["rho_updates"].max() >= 1, name
    for name, mi in (("max_iter_30", 30), ("max_iter_60", 60), ("max_iter_100", 100),
                     ("max_iter_110", 110), ("no_check", 200)):
        ref = AC.case(name)[3]
        failed = ref["status"] != AC.OK
        assert failed.sum() >= 60 and np.all(ref["iters"][failed] == mi), name
        assert np.all(np.isin(ref["status"][failed], (AC.MAX_ITER, AC.SOLVED_INACCURATE))), name
    ref = AC.case("max_iter_110")[3]
    assert (ref["status"] == AC.MAX_ITER).sum() >= 8 and (ref["status"] == AC.SOLVED_INACCURATE).sum() >= 8
    assert ref["rho_updates"].max() == 1 and 110 % 25 != 0 and 100 % 25 == 0
    ref = AC.case("no_check")[3]
    assert np.all(ref["iters"] == 200) and ref["rho_updates"].min() >= 1   # interval 100
    # the Ruiz loop settles: 10 passes or 9 give the same bits and 4 or 3 differ by ~1e-10, so only
    # the short loops tell the number of passes (most robots move by far more than any tolerance)
    f = [AC.case(k)[3]["forces"] for k in ("scaling_0", "scaling_1", "scaling_2")]
    assert (np.abs(f[1] - f[0]).max(axis=1) > 1e-2).sum() >= 32
    assert (np.abs(f[2] - f[1]).max(axis=1) > 1e-2).sum() >= 32
    ref = AC.case("no_adaptive_rho")[3]
    assert np.all(ref["rho_updates"] == 0) and {AC.OK, AC.SOLVED_INACCURATE} <= set(ref["status"].tolist())
    assert ref["iters"].max() == 4000


def test_a1qp_case_tolerances_hold_their_conditions():
    """The widened force tolerance (a1qp_cases.force_tolerance) stays a check:
    at least half the robots of every case keep the plain 1e-7 and no robot
    gets more than 1e-2 relative."""
    for name in AC.CASES:
        _, _, _, ref, s_b = AC.case(name)
        _, rel = AC.force_tolerance(ref, s_b)
        assert (rel == 1e-7).sum() >= len(rel) / 2, (name, np.sort(s_b)[-8:])
        assert rel.max() <= 1e-2, (name, s_b.max())


@pytest.mark.parametrize("name", BODY_CASES)
def test_a1_oracle_build_matches_numpy_transcription_with_parameters(name):
    S, CT, ov, _, _ = AC.case(name)
    p, _ = AC.split(ov)
    kw = {NP_NAMES[k]: v for k, v in ov.items() if k in NP_NAMES}
    for b in range(len(S)):
        got = O.a1_build(S[b], CT[b], p)
        ref = np_a1_build(S[b], CT[b], **kw)
        for x, y in zip(got, ref):
            assert np.allclose(x, y, rtol=1e-12, atol=1e-9), (name, b)
        assert np.array_equal(got[1], got[1].T)


@pytest.mark.parametrize("name", ["f_min_20", "f_min_eq_f_max", "mu_0", "mu_0.2"])
def test_a1_oracle_admm_reaches_exact_optimum_with_parameters(name):
    """As test_a1_oracle_admm_reaches_exact_optimum at eps 1e-9, with a lower
    normal-force bound, the stance normal forces fixed (equality rows), no
    friction (f_x = f_y = 0) and a narrow pyramid."""
    S, CT = AC.inputs(6, 48)
    p, _ = AC.split(AC.CASES[name])
    for b in range(48):
        acc, H, g, A, l, u = O.a1_build(S[b], CT[b], p)
        xe, st, _ = O.exact_solve(H, g, A, l, u)
        assert st == 0, (name, b)
        f9, x9, info9 = O.a1_compute_grf(S[b], CT[b], p, eps_abs=1e-9, eps_rel=1e-9, max_iter=50000)
        assert info9.status == 0, (name, b)
        assert np.abs(x9 - xe).max() <= 1e-3 * max(1.0, np.abs(xe).max()), (name, b)
        for i in range(4):
            if not CT[b, i]:
                assert np.abs(x9[3 * i:3 * i + 3]).max() <= 1e-6
            elif name == "f_min_eq_f_max":
                assert abs(x9[3 * i + 2] - 40.0) <= 1e-6
            elif name == "f_min_20":
                assert x9[3 * i + 2] >= 20.0 - 1e-6
        R = S[b, 24:33].reshape(3, 3).T
        assert np.allclose(f9.reshape(4, 3), (R.T @ x9.reshape(4, 3).T).T, atol=1e-12)


NAN, INF = float("nan"), float("inf")
BAD_PARAMS = [
    dict(eps_abs=-1e-3), dict(eps_rel=-1e-3), dict(eps_abs=0.0, eps_rel=0.0),
    dict(alpha=0.0), dict(alpha=2.0), dict(alpha=-0.5), dict(adaptive_rho_interval=-1),
    dict(adaptive_rho_tolerance=0.5), dict(mu=-0.1), dict(f_min=181.0), dict(f_min=1.0, f_max=0.0),
    dict(r=-1e-3), dict(q_diag=(1.0, 1.0, 1.0, 400.0, -400.0, 100.0)),
    dict(rho=0.0), dict(sigma=0.0), dict(robot_mass=0.0), dict(scaling=-1), dict(check_termination=-1),
    dict(rho=NAN), dict(sigma=INF), dict(alpha=NAN), dict(eps_abs=NAN), dict(eps_rel=INF),
    dict(adaptive_rho_tolerance=INF), dict(robot_mass=NAN), dict(mu=NAN), dict(f_min=-INF),
    dict(f_max=INF), dict(r=NAN), dict(q_diag=(1.0, NAN, 1.0, 400.0, 400.0, 100.0)),
    dict(kp_linear=(INF, 1000.0, 1000.0)), dict(kd_linear=(200.0, NAN, 120.0)),
    dict(kp_angular=(650.0, 35.0, NAN)), dict(kd_angular=(-INF, 4.5, 30.0)),
]
EDGE_PARAMS = [
    dict(eps_abs=0.0), dict(eps_rel=0.0), dict(alpha=1.999), dict(alpha=1e-3),
    dict(adaptive_rho_tolerance=1.0), dict(mu=0.0), dict(f_min=180.0), dict(f_min=-5.0),
    dict(r=0.0), dict(q_diag=(0.0,) * 6), dict(check_termination=0), dict(scaling=0),
    dict(adaptive_rho_interval=1), dict(kp_linear=(-1.0, 0.0, 1.0)),
]


def test_a1_capi_parameter_rule():
    """qloco_a1_params_check (include/qloco.h section 9): what OSQP v0.6's
    validate_settings refuses, non-finite fields and an ill-posed body return
    QLOCO_ERR_ARG from the check, from qloco_a1_qp_solve before any device work
    (the pointers here are not device memory) and as ValueError from
    a1qp.A1QpBatch; the boundary values and every case of the table pass."""
    L = _lib.lib()
    d = [C.c_void_p(16)] * 3
    assert L.qloco_a1_params_check(None) == 100
    assert L.qloco_a1_params_check(C.byref(a1qp.default_params())) == 0
    for ov in BAD_PARAMS:
        p = a1qp.default_params(**ov)
        assert L.qloco_a1_params_check(C.byref(p)) == 100, ov
        assert L.qloco_last_error().decode().startswith("qloco_a1_params_check: "), ov
        assert L.qloco_a1_qp_solve(C.byref(p), 4, *d, *([None] * 6)) == 100, ov
        with pytest.raises(ValueError, match="qloco_a1_params_check"):
            a1qp.A1QpBatch(**ov)
        with pytest.raises(ValueError):
            a1qp.A1QpBatch(params=p)
        assert L.qloco_a1_qp_solve(C.byref(p), 0, *([None] * 9)) == 0   # an empty batch does nothing
    for ov in EDGE_PARAMS + list(AC.CASES.values()):
        assert L.qloco_a1_params_check(C.byref(a1qp.default_params(**ov))) == 0, ov
        a1qp.A1QpBatch(**ov)
