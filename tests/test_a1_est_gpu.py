"""GPU tests of the A1 state-estimation front end (csrc/qloco_a1est.hip):
A1 leg kinematics against the reference's own arithmetic
(golden/a1_kin_ref.npz) and the batched A1BasicEKF against the literal numpy
restatement (tests/a1_est_ref.py).

Tolerance for x and P.  The kernel factors S once (Cholesky) where the
reference solves twice with fullPivHouseholderQr, so parity is to rounding.
The spread between two summation orders of the same fp64 arithmetic was
measured on the CPU as max |literal - Cholesky formulation| over exactly the
inputs of the single-update and closed-sequence tests below, every tick
(`python tests/a1_est_ref.py`): 9.881e-14 for x entries, 3.675e-14 for P
entries.  The kernel's reduction order inside a lane group is a third order
of that arithmetic, so the bounds are 16 x the measured spreads.
"""
import os

import numpy as np
import pytest

import a1_est_ref as R
import host_exe
from quadrupedal_loco_amd import a1est

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

X_SPREAD = 9.881e-14    # measured, CPU, literal vs Cholesky formulation
P_SPREAD = 3.675e-14
X_TOL = 16 * X_SPREAD   # 1.581e-12
P_TOL = 16 * P_SPREAD   # 5.880e-13
EKF_KEYS = ("dt", "root_rot_mat", "imu_acc", "imu_ang_vel", "foot_pos_rel", "foot_vel_rel",
            "foot_force")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _tick(inp, t, dev):
    """update() arguments of tick t as device tensors."""
    d = {k: _t(inp[k][t], dev) for k in EKF_KEYS}
    d["movement_mode"] = _t(inp["movement_mode"].astype(np.int32), dev)
    return d


def _taken(P):
    """The drift-reduction branch (A1BasicEKF.cpp:143-147) leaves the cross
    blocks exactly zero; one filter step without it refills them."""
    return (P[:, 0:2, 2:] == 0).all((1, 2))


def _run(inp, dev, flat=True, x0=None, P0=None):
    """Closed loop on the GPU, as a1_est_ref.run_sequence: x, P, contacts, taken per tick."""
    T, B = inp["dt"].shape
    est = a1est.A1Estimator(B, dev, assume_flat_ground=1 if flat else 0)
    if x0 is None:
        est.init(_t(inp["root_rot_mat"][0], dev), _t(inp["foot_pos_rel"][0], dev))
    else:
        est.load_state(_t(x0, dev), _t(P0, dev))
    X, PP = np.zeros((T, B, 18)), np.zeros((T, B, 18, 18))
    CT, TK = np.zeros((T, B, 4), np.uint8), np.zeros((T, B), bool)
    for t in range(T):
        out = est.update(**_tick(inp, t, dev))
        x, P = est.state()
        X[t], PP[t] = x.cpu().numpy(), P.cpu().numpy()
        assert np.array_equal(out.root_pos.cpu().numpy(), X[t][:, 0:3])
        assert np.array_equal(out.root_lin_vel.cpu().numpy(), X[t][:, 3:6])
        CT[t], TK[t] = out.estimated_contacts.cpu().numpy(), _taken(PP[t])
    return X, PP, CT, TK


# ------------------------------------------------------------------ kinematics
def _special_quats(rng, B):
    """Random attitudes; yaw on both sides of +-pi; |t2| of quat_to_euler above
    1 (not normalised, as the callback passes them through)."""
    e = np.stack([rng.uniform(-0.4, 0.4, B), rng.uniform(-0.4, 0.4, B), rng.uniform(-np.pi, np.pi, B)], 1)
    e[0:6, 2] = (np.pi - 1e-9, -np.pi + 1e-9, np.pi - 1e-3, -np.pi + 1e-3, np.pi, -np.pi)
    cr, sr, cp, sp, cy, sy = (np.cos(e[:, 0] / 2), np.sin(e[:, 0] / 2), np.cos(e[:, 1] / 2),
                              np.sin(e[:, 1] / 2), np.cos(e[:, 2] / 2), np.sin(e[:, 2] / 2))
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                  cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], 1)
    q[6] = (0.7072, 0.0, 0.7072, 0.0)      # t2 = 1.0003 -> clamped to 1
    q[7] = (0.7072, 0.0, -0.7072, 0.0)     # t2 < -1 -> clamped to -1
    q[8] = (np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0)
    q[9] = (0.70710678, 0.001, 0.70710678, -0.001)
    return q


def test_a1_leg_kinematics_against_reference_arithmetic():
    dev = _dev()
    z = np.load(os.path.join(HERE, "golden", "a1_kin_ref.npz"))
    n = len(z["leg"])
    B = n // 4
    assert n == 404 and np.array_equal(z["leg"], np.arange(n) % 4)
    rng = np.random.default_rng(5)
    quat = _special_quats(rng, B)
    pos, vel = rng.uniform(-1, 1, (B, 3)), rng.normal(0, 0.5, (B, 3))
    out = a1est.A1LegKin().forward(_t(z["q"].reshape(B, 12), dev), _t(z["qd"].reshape(B, 12), dev),
                                   _t(quat, dev), _t(pos, dev), _t(vel, dev))
    torch.cuda.synchronize()
    g = {k: getattr(out, k).cpu().numpy() for k in out.__dataclass_fields__}
    e_pos = np.abs(g["foot_pos_rel"].reshape(n, 3) - z["pos"]).max()
    e_jac = np.abs(g["j_foot"].reshape(n, 9) - z["jac"]).max()
    e_vel = np.abs(g["foot_vel_rel"].reshape(n, 3) - z["vel"]).max()
    print("kin: pos %.3e jac %.3e vel %.3e" % (e_pos, e_jac, e_vel))
    assert e_pos <= 1e-12
    assert e_jac <= 1e-9
    assert e_vel <= 1e-9 * np.abs(z["qd"]).max()
    # stand-pose known answers: feet below the hips, mirrored left / right
    stand = g["foot_pos_rel"][0].reshape(4, 3)
    assert np.abs(stand[:, 0] - (0.1805, 0.1805, -0.1805, -0.1805)).max() <= 1e-12
    assert np.abs(stand[:, 1] - (0.1308, -0.1308, 0.1308, -0.1308)).max() <= 1e-12
    assert np.abs(stand[:, 2] + 0.21 * 2 * np.cos(0.72)).max() <= 1e-12
    # attitude outputs against the numpy restatements
    Rm = R.quat_to_rot(quat)
    eul = R.quat_to_euler(quat)
    assert abs(eul[6, 1] - np.pi / 2) == 0 and abs(eul[7, 1] + np.pi / 2) == 0   # clamped
    assert eul[0, 2] > 3.14 and eul[1, 2] < -3.14
    assert np.abs(g["root_rot_mat"].reshape(B, 3, 3).transpose(0, 2, 1) - Rm).max() <= 1e-14
    assert np.abs(g["root_euler"] - eul).max() <= 1e-14
    assert np.abs(g["root_rot_mat_z"].reshape(B, 3, 3).transpose(0, 2, 1) - R.rot_z(eul[:, 2])).max() <= 1e-14
    # frames: abs = R rel, world = abs + root (GazeboA1ROS.cpp:326-330)
    Rg = g["root_rot_mat"].reshape(B, 3, 3).transpose(0, 2, 1)
    for a, r in (("foot_pos_abs", "foot_pos_rel"), ("foot_vel_abs", "foot_vel_rel")):
        want = np.einsum("bij,blj->bli", Rg, g[r].reshape(B, 4, 3)).reshape(B, 12)
        scale = max(1.0, np.abs(want).max())
        assert np.abs(g[a] - want).max() <= 1e-15 * scale, a
    assert np.array_equal(g["foot_pos_world"], (g["foot_pos_abs"].reshape(B, 4, 3) + pos[:, None]).reshape(B, 12))
    assert np.array_equal(g["foot_vel_world"], (g["foot_vel_abs"].reshape(B, 4, 3) + vel[:, None]).reshape(B, 12))


# ------------------------------------------------------------------------ EKF
@pytest.mark.parametrize("B", R.SINGLE_BATCHES)
def test_a1_ekf_init_state(B):
    dev = _dev()
    inp, _, _ = R.single_update_case(B)
    est = a1est.A1Estimator(B, dev)
    assert not est.is_inited()
    est.init(_t(inp["root_rot_mat"][0], dev), _t(inp["foot_pos_rel"][0], dev))
    x, P = (a.cpu().numpy() for a in est.state())
    assert est.is_inited()
    for b in range(B):
        a = R._args(inp, 0, b)
        xr, Pr = R.init_state(a[2], a[5])
        assert np.array_equal(P[b], Pr), b
        assert np.abs(x[b] - xr).max() <= 1e-15, b


@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("B", R.SINGLE_BATCHES)
def test_a1_ekf_single_update_from_arbitrary_state(B, flat):
    dev = _dev()
    inp, x0, P0 = R.single_update_case(B)
    Xr, Pr, Cr, TKr, MGr = R.reference(str(B), flat)
    X, P, CT, TK = _run(inp, dev, flat, x0, P0)
    ex, ep = np.abs(X - Xr).max(), np.abs(P - Pr).max()
    print("single update B=%d flat=%d: x %.3e (bound %.3e)  P %.3e (bound %.3e)" % (B, flat, ex, X_TOL, ep, P_TOL))
    assert np.array_equal(CT, (Cr >= 0.5).astype(np.uint8))
    assert np.array_equal(P, P.transpose(0, 1, 3, 2))
    assert np.array_equal(TK, TKr)
    assert ex <= X_TOL and ep <= P_TOL
    if B > 3:   # the pinned forces: below 0, in (0, 100), exactly 50, above 100
        assert CT[0, 0].tolist() == [0, 1, 0, 1] and CT[0, 1].tolist() == [0, 1, 1, 1]
        assert CT[0, 2].tolist() == [0, 1, 1, 0] and CT[0, 3].tolist() == [1, 1, 1, 1]


def _compare_sequence(name, inp, ref, got):
    Xr, Pr, Cr, TKr, MGr = ref
    X, P, CT, TK = got
    # instance-ticks whose determinant sits within 1e-9 of the threshold may
    # take the other branch legitimately; they leave the comparison from there on
    excl = np.maximum.accumulate(np.abs(MGr) < 1e-9, axis=0)
    assert excl.mean() <= 0.01
    keep = ~excl
    ex, ep = np.abs(X - Xr)[keep].max(), np.abs(P - Pr)[keep].max()
    print("%s: x %.3e (bound %.3e)  P %.3e (bound %.3e)  excluded %d" % (name, ex, X_TOL, ep, P_TOL, excl.sum()))
    assert np.array_equal(CT, (Cr >= 0.5).astype(np.uint8))
    assert np.array_equal(P, P.transpose(0, 1, 3, 2))
    assert np.array_equal(TK[keep], TKr[keep])
    assert ex <= X_TOL and ep <= P_TOL


def test_a1_ekf_closed_sequence_golden():
    """golden/a1_ekf.npz: 8 robots x 48 ticks from init_state, x at every tick
    and P at the four checkpoints against the committed literal results."""
    dev = _dev()
    z = np.load(os.path.join(HERE, "golden", "a1_ekf.npz"))
    inp = {k: z[k] for k in z.files}
    X, P, CT, TK = _run(inp, dev)
    ck = z["checkpoints"]
    ex, ep = np.abs(X - z["x"]).max(), np.abs(P[ck] - z["P"]).max()
    print("golden sequence: x %.3e (bound %.3e)  P %.3e (bound %.3e)" % (ex, X_TOL, ep, P_TOL))
    assert np.abs(z["det_margin"]).min() >= 1e-9
    assert np.array_equal(CT, z["contacts"]) and np.array_equal(TK, z["drift_taken"])
    assert np.array_equal(P, P.transpose(0, 1, 3, 2))
    assert ex <= X_TOL and ep <= P_TOL


def test_a1_ekf_closed_sequence_both_drift_branches():
    """67 robots x 64 ticks at dt = 0.05 (a1_est_ref.SEQ_*): after tick 5 the
    literal restatement takes the drift-reduction branch 374 times and skips it
    3512 times, and its smallest |det - 1e-6| is 1.47e-9, so the reference
    alone excludes no instance-tick (seed chosen for that on the CPU; asserted
    again in tests/test_a1_est.py)."""
    dev = _dev()
    ref = R.reference("sequence")
    assert ref[3][6:].any() and (~ref[3][6:]).any()
    assert (np.abs(ref[4]) < 1e-9).sum() == 0
    inp = R.sequence_case()
    _compare_sequence("dt 0.05 sequence", inp, ref, _run(inp, dev))


def test_a1_ekf_batch_composition_independence():
    """Robot k computes the same bits alone and at positions 0, 66 and 1029 of
    a larger batch (first lane group, second group of a later workgroup, ragged
    tail); two identical runs are bit-identical."""
    dev = _dev()
    inp, x0, P0 = R.single_update_case(1030)
    inp = {k: v.copy() for k, v in inp.items()}
    x0, P0 = x0.copy(), P0.copy()
    k, spots = 517, (0, 66, 1029)
    for s in spots:
        for key in EKF_KEYS:
            inp[key][:, s] = inp[key][:, k]
        inp["movement_mode"][s] = inp["movement_mode"][k]
        x0[s], P0[s] = x0[k], P0[k]
    big = _run(inp, dev, True, x0, P0)
    again = _run(inp, dev, True, x0, P0)
    for a, b in zip(big, again):
        assert np.array_equal(a, b)
    one = {key: inp[key][:, k:k + 1] for key in EKF_KEYS}
    one["movement_mode"] = inp["movement_mode"][k:k + 1]
    solo = _run(one, dev, True, x0[k:k + 1], P0[k:k + 1])
    for s in spots + (k,):
        for a, b in zip(big, solo):
            assert np.array_equal(a[:, s], b[:, 0]), s


def test_a1_ekf_state_plumbing_and_workspace_isolation():
    dev = _dev()
    inp = R.sequence_case()
    B = inp["dt"].shape[1]
    a, b = a1est.A1Estimator(B, dev), a1est.A1Estimator(B, dev)
    a.init(_t(inp["root_rot_mat"][0], dev), _t(inp["foot_pos_rel"][0], dev))
    for t in range(3):
        a.update(**_tick(inp, t, dev))
    x, P = a.state()
    b.load_state(x, P)
    xb, Pb = b.state()
    assert torch.equal(x, xb) and torch.equal(P, Pb)
    # a third filter on other data between the two: workspaces do not interfere
    other = R.golden_case()
    c = a1est.A1Estimator(other["dt"].shape[1], dev)
    c.init(_t(other["root_rot_mat"][0], dev), _t(other["foot_pos_rel"][0], dev))
    c.update(**_tick(other, 0, dev))
    xc, Pc = (v.clone() for v in c.state())
    oa = a.update(**_tick(inp, 3, dev))
    ob = b.update(**_tick(inp, 3, dev))
    torch.cuda.synchronize()
    for u, v in zip(a.state() + (oa.root_pos, oa.root_lin_vel, oa.estimated_contacts),
                    b.state() + (ob.root_pos, ob.root_lin_vel, ob.estimated_contacts)):
        assert torch.equal(u, v)
    assert torch.equal(c.state()[0], xc) and torch.equal(c.state()[1], Pc)
    assert not torch.equal(a.state()[0], x)


def test_a1_ekf_update_replays_from_a_hip_graph():
    """One update captured on a single stream (no parallel branches), replayed
    three times with new inputs in static tensors: bit-identical to three
    eager calls (precedent: test_force_qp_grouped_launch_replays_from_a_hip_graph)."""
    dev = _dev()
    inp = R.sequence_case()
    B = inp["dt"].shape[1]
    eager, graphed = a1est.A1Estimator(B, dev), a1est.A1Estimator(B, dev)
    for e in (eager, graphed):
        e.init(_t(inp["root_rot_mat"][0], dev), _t(inp["foot_pos_rel"][0], dev))
    static = _tick(inp, 0, dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):  # warm-up on a throw-away filter
        w = a1est.A1Estimator(B, dev)
        w.load_state(*eager.state())
        w.update(**static)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        og = graphed.update(**static)
    for t in range(3):
        for key, v in _tick(inp, t, dev).items():
            static[key].copy_(v)
        g.replay()
        oe = eager.update(**_tick(inp, t, dev))
        torch.cuda.synchronize()
        assert torch.equal(og.root_pos, oe.root_pos) and torch.equal(og.root_lin_vel, oe.root_lin_vel)
        assert torch.equal(og.estimated_contacts, oe.estimated_contacts)
        for u, v in zip(graphed.state(), eager.state()):
            assert torch.equal(u, v), t


def test_a1_ekf_cpp_shim_matches_c_abi():
    _dev()
    print(host_exe.run("test_a1_est_host").stdout)
