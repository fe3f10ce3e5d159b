"""GPU tests of the A1 gait plan, swing-leg control, terrain pitch and joint
torques (csrc/qloco_a1ctrl.hip) against the literal restatement
(tests/a1_ctrl_ref.py).

Bit-identical to the restatement's first (reference) formulation: gait
counters, all three contact flags, the recent-contact filter state,
foot_pos_start, the Raibert targets, foot_pos_cur, the finite differences of
the current foot position, foot_forces_kin of stance legs, stance torques, the
hold-off and NaN-hold decisions, the terrain gate, clamp and sign decisions.
With the restatement's Bezier powers switched to repeated multiplication (what
the kernel computes) foot_forces_kin, foot_pos_target_last_time and the swing
torques are bit-identical too.

Bounded: four steps cannot be bit-identical (Bezier powers, swing torque
solve, terrain pseudo-inverse, terrain angle).  SPREAD holds the largest
difference between the restatement's two formulations of them, measured on the
CPU over exactly the inputs of the tests below (`python tests/a1_ctrl_ref.py`;
tests/test_a1_ctrl.py checks that the figures reproduce); the kernel is a
third formulation, so each bound is 16 x the measured spread.
"""
import os

import numpy as np
import pytest

import a1_ctrl_ref as R
import host_exe
from quadrupedal_loco_amd import a1ctrl

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SPREAD = dict(foot_forces_kin=5.684e-13, joint_torques=9.095e-13, surf_coef=3.490e-11,
              terrain_pitch_angle=1.243e-15, tgt_last=1.110e-16, te_sum=1.243e-13, te_ring=6.817e-14)
TOL = {k: 16 * v for k, v in SPREAD.items()}

EXACT_OUT = ("contacts", "plan_contacts", "early_contacts", "gait_counter", "foot_pos_target_rel",
             "foot_pos_target_abs", "foot_pos_target_world", "foot_pos_cur", "foot_pos_recent_contact")
# record slices no formulation can move
EXACT_REC = [(0, R.O_TGT_LAST), (R.O_TGT_REL, R.O_FKIN), (R.O_MPC, R.O_MPC + 1),
             (R.O_RC_FILL, R.O_TE_SUM), (R.O_RC_RING, R.O_TE_RING)]
worst = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _params(prm):
    if prm is None:
        return a1ctrl.default_params()
    return a1ctrl.default_params(**{k: v for k, v in prm.items() if v != R.default_params()[k]})


def _run(inp, dev, rec0=None, prm=None, order=("plan", "terrain", "torques"), ctrl=None):
    """The GPU twin of a1_ctrl_ref.run: same keys, same shapes."""
    T, B = inp["dt"].shape
    ctrl = ctrl or a1ctrl.A1GaitSwing(B, dev, params=_params(prm))
    if rec0 is not None:
        ctrl.set_state(_t(rec0, dev))
    d = {k: _t(inp[k], dev) for k in R.IN_KEYS}
    keep = {k: [] for k in R.OUT_KEYS + ("record",)}
    for t in range(T):
        for step in order:
            if step == "plan":
                o = ctrl.plan_swing(d["dt"][t], d["movement_mode"][t], d["root_pos"][t], d["root_lin_vel"][t],
                                    d["root_lin_vel_d"][t], d["root_rot_mat"][t], d["root_rot_mat_z"][t],
                                    d["foot_pos_abs"][t], d["foot_force"][t])
                for k in R.OUT_KEYS[:10]:
                    keep[k].append(getattr(o, k))
            elif step == "terrain":
                e = d["root_euler_d"][t].clone()
                o = ctrl.terrain(d["root_pos"][t], e)
                keep["terrain_pitch_angle"].append(o.terrain_pitch_angle)
                keep["surf_coef"].append(o.surf_coef)
                keep["root_euler_d"].append(e)
            else:
                keep["joint_torques"].append(ctrl.joint_torques(d["j_foot"][t], d["foot_forces_grf"][t]))
        keep["record"].append(ctrl.get_state())
    torch.cuda.synchronize()
    return {k: torch.stack(v).cpu().numpy() for k, v in keep.items() if v}


def _exact(name, key, got, want):
    assert np.array_equal(got, want, equal_nan=True), (name, key, np.argwhere(~((got == want) | (got != got)))[:4])


def _close(name, key, got, want, tol):
    e = R.spread(got, want)
    worst[key] = max(worst.get(key, 0.0), e)
    assert e <= tol, (name, key, e, tol)
    return e


def _compare(name, got, ref, prm=None, calls=("plan", "terrain", "torques")):
    """Everything against the first formulation: bits where no formulation can
    differ, 16 x the measured spread elsewhere."""
    prm = prm or R.default_params()
    rec, rrec = got["record"], ref["record"]
    fig = {}
    for a, b in EXACT_REC:
        _exact(name, "record[%d:%d]" % (a, b), rec[..., a:b], rrec[..., a:b])
    if "plan" in calls:
        for k in EXACT_OUT:
            _exact(name, k, got[k], ref[k])
        # a stance leg's target is exact (t = 0); its target velocity is too once the
        # previous tick's target was (the given state at tick 0, a stance tick later)
        stance = ref["gait_counter"] <= prm["counter_per_swing"]
        stance[1:] &= stance[:-1]
        stance = np.repeat(stance, 3, axis=-1)
        _exact(name, "foot_forces_kin (stance)", got["foot_forces_kin"][stance], ref["foot_forces_kin"][stance])
        fig["fkin"] = _close(name, "foot_forces_kin", got["foot_forces_kin"], ref["foot_forces_kin"], TOL["foot_forces_kin"])
        fig["tgt_last"] = _close(name, "tgt_last", rec[..., R.O_TGT_LAST:R.O_TGT_REL], rrec[..., R.O_TGT_LAST:R.O_TGT_REL], TOL["tgt_last"])
        _close(name, "foot_forces_kin", rec[..., R.O_FKIN:R.O_JT], rrec[..., R.O_FKIN:R.O_JT], TOL["foot_forces_kin"])
    if "torques" in calls:
        tau, rtau = got["joint_torques"], ref["joint_torques"]
        cont = np.repeat(rrec[..., R.O_CONT:R.O_CONT + 4] != 0, 3, axis=-1)
        held = np.repeat(rrec[..., R.O_MPC:R.O_MPC + 1] < prm["torque_holdoff_ticks"], 12, axis=-1)
        assert not tau[held].any()
        _exact(name, "joint_torques (stance)", tau[cont], rtau[cont])
        assert not np.isnan(tau).any()
        fig["tau"] = _close(name, "joint_torques", tau, rtau, TOL["joint_torques"])
        _exact(name, "record joint_torques", rec[..., R.O_JT:R.O_MPC], tau)
    if "terrain" in calls:
        fig["surf"] = _close(name, "surf_coef", got["surf_coef"], ref["surf_coef"], TOL["surf_coef"])
        ang, rang = got["terrain_pitch_angle"], ref["terrain_pitch_angle"]
        fig["angle"] = _close(name, "terrain_pitch_angle", ang, rang, TOL["terrain_pitch_angle"])
        _exact(name, "clamp", np.abs(ang) == 0.5, np.abs(rang) == 0.5)
        _exact(name, "gate", ang == 0.0, rang == 0.0)
        e, re_ = got["root_euler_d"], ref["root_euler_d"]
        _exact(name, "root_euler_d[0, 2]", e[..., [0, 2]], re_[..., [0, 2]])
        _exact(name, "sign", np.signbit(e[..., 1]), np.signbit(re_[..., 1]))
        _exact(name, "root_euler_d[1]", np.abs(e[..., 1]), np.abs(ang))
        _exact(name, "record terrain", rec[..., R.O_TERRAIN], ang)
        fig["te_sum"] = _close(name, "te_sum", rec[..., R.O_TE_SUM:R.O_TE_CORR + 1], rrec[..., R.O_TE_SUM:R.O_TE_CORR + 1], TOL["te_sum"])
        fig["te_ring"] = _close(name, "te_ring", rec[..., R.O_TE_RING:], rrec[..., R.O_TE_RING:], TOL["te_ring"])
    print(name, " ".join("%s %.3e" % kv for kv in fig.items()))


def _compare_kernel_form(name, got, ref):
    """Against the restatement with the kernel's Bezier powers: plan_swing and
    the torques bit for bit."""
    for k in EXACT_OUT + ("foot_forces_kin", "joint_torques"):
        _exact(name, k + " (kernel formulation)", got[k], ref[k])
    _exact(name, "record (kernel formulation)", got["record"][..., :R.O_TERRAIN], ref["record"][..., :R.O_TERRAIN])


# ----------------------------------------------------------------- single call
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("B", R.SINGLE_BATCHES)
def test_a1_ctrl_single_call_from_arbitrary_state(B, flip):
    dev = _dev()
    inp, r0 = R.single_case(B, flip)
    ref = R.reference(("single", B, flip))
    got = _run(inp, dev, r0)
    name = "single B=%d flip=%d" % (B, flip)
    _compare(name, got, ref)
    _compare_kernel_form(name, got, R.reference(("single", B, flip), "kernel"))
    # what the case is meant to reach
    mode = inp["movement_mode"][0]
    gc = ref["gait_counter"][0]
    if B >= 67:
        assert (mode == 0).any() and (mode == 1).any()
        assert (ref["early_contacts"] != 0).any() and (np.abs(ref["terrain_pitch_angle"]) == 0.5).any()
        assert (ref["terrain_pitch_angle"] == 0.0).any()
        assert not np.isfinite(got["foot_forces_kin"][0, 5]).all()        # dt = 0
        assert not got["joint_torques"][0, 5][np.repeat(got["contacts"][0, 5] == 0, 3)].any()
    if not flip:
        assert gc.reshape(-1)[0] == 120.0 and gc.reshape(-1)[1] == 122.0 and gc.reshape(-1)[3] == 0.0
        assert got["contacts"].reshape(-1)[:4].tolist() == [1, 0, 1, 1]     # at cps, past it, early, wrapped


def test_a1_ctrl_terrain_straight_after_reset():
    """The all-zero start state: W'W = diag(4, 0, 0), surf_coef (0, 0, -1), angle 0."""
    dev = _dev()
    inp = R.reset_case()
    got = _run(inp, dev, order=("terrain",))
    _compare("reset", got, R.reference(("reset",)), calls=("terrain",))
    assert np.array_equal(got["surf_coef"][0], [[0.0, 0.0, -1.0]] * 3)
    assert not got["terrain_pitch_angle"].any()
    assert np.array_equal(got["record"][0, :, R.O_TE_FILL], [1.0] * 3)


# ------------------------------------------------------------- closed sequence
@pytest.mark.parametrize("speed,B", [(8, 1), (8, 3), (8, 67), (2, 67)])
def test_a1_ctrl_closed_sequence(speed, B):
    """200 ticks from reset (a1_ctrl_ref.sequence_case): standstill, walking,
    standstill; early contacts; both sides of the terrain gate; the torque
    hold-off; a NaN ground force on one leg of robot 0."""
    dev = _dev()
    prm = R.sequence_params(speed)
    inp, ref = R.subset(R.sequence_case(speed), B), R.subset(R.reference(("sequence", speed)), B)
    got = _run(inp, dev, prm=prm)
    _compare("sequence speed=%d B=%d" % (speed, B), got, ref, prm)
    # the scenario happened
    assert ref["plan_contacts"][:R.SEQ_STAND].all() and ref["plan_contacts"][R.SEQ_STOP:].all()
    assert np.array_equal(ref["gait_counter"][R.SEQ_STOP:], np.broadcast_to([0.0, 120.0, 120.0, 0.0], (20, B, 4)))
    assert not ref["plan_contacts"][R.SEQ_STAND:R.SEQ_STOP].all()
    assert not got["joint_torques"][:9].any() and got["joint_torques"][9].any()
    t0, t1 = R.NAN_TICKS
    sl = slice(3 * R.NAN_LEG, 3 * R.NAN_LEG + 3)
    stance = got["contacts"][t0:t1, R.NAN_ROBOT, R.NAN_LEG] != 0
    assert stance.any()
    assert not got["joint_torques"][t0:t1, R.NAN_ROBOT, sl][stance].any()      # held at the zeroed value
    if B == 67:
        full = R.reference(("sequence", speed))
        assert (full["early_contacts"] != 0).any()
        ang = full["terrain_pitch_angle"]
        assert (ang[:20, 1] == 0.0).all() and (ang[40:, 1] != 0.0).all()       # gate opens
        assert (ang[:90, 2] != 0.0).all() and (ang[110:, 2] == 0.0).all()       # gate closes
        rec = full["record"]
        assert (rec[-1, :, R.O_RC_FILL:R.O_RC_FILL + 4] == 60).all() and (rec[-1, 0, R.O_TE_FILL] == 100)
    if B == 67 and speed == 8:
        # the NaN stays with its robot: every other robot's outputs and
        # workspace bits are those of a run without it
        clean = {k: v.copy() for k, v in inp.items()}
        clean["foot_forces_grf"][t0:t1, R.NAN_ROBOT] = 1.0
        other = _run(clean, dev, prm=prm)
        for k in got:
            assert np.array_equal(got[k][:, 1:], other[k][:, 1:], equal_nan=True), k
        assert not np.array_equal(got["joint_torques"][:, 0], other["joint_torques"][:, 0])


# ------------------------------------------------------------------- plumbing
def test_a1_ctrl_batch_position_independence():
    """A robot computes the same outputs and workspace bits at batch 1 and at
    positions 0, 40 and 66 of batch 67 (first lanes, mid-wave, ragged tail)."""
    dev = _dev()
    inp, r0 = R.single_case(67)
    inp = {k: v.copy() for k, v in inp.items()}
    r0 = r0.copy()
    k, spots = 23, (0, 40, 66)
    for s in spots:
        for key in R.IN_KEYS:
            inp[key][:, s] = inp[key][:, k]
        r0[s] = r0[k]
    big = _run(inp, dev, r0)
    solo = _run({key: inp[key][:, k:k + 1] for key in R.IN_KEYS}, dev, r0[k:k + 1])
    for s in spots + (k,):
        for key in big:
            assert np.array_equal(big[key][:, s], solo[key][:, 0], equal_nan=True), (key, s)


def test_a1_ctrl_workspace_isolation_and_state_round_trip():
    dev = _dev()
    inp, r0 = R.single_case(67)
    a, b = a1ctrl.A1GaitSwing(67, dev), a1ctrl.A1GaitSwing(67, dev)
    fresh = b.get_state().clone()
    want = np.zeros((67, R.REC))
    want[:, 0:4] = (0, 120, 120, 0)
    assert np.array_equal(fresh.cpu().numpy(), want)                     # reset values
    a.set_state(_t(r0, dev))
    assert np.array_equal(a.get_state().cpu().numpy(), r0)               # round trip, every field
    _run(inp, dev, ctrl=a)
    assert torch.equal(b.get_state(), fresh)                             # b untouched
    assert not np.array_equal(a.get_state().cpu().numpy(), r0)
    b.set_state(a.get_state())
    assert np.array_equal(a.get_state().cpu().numpy(), b.get_state().cpu().numpy(), equal_nan=True)   # dt = 0 robot
    a.reset()
    assert torch.equal(a.get_state(), fresh) and not torch.equal(b.get_state(), fresh)


TICK_KEYS = ("dt", "movement_mode", "joint_pos", "joint_vel", "root_quat", "imu_acc", "imu_ang_vel",
             "foot_force", "root_lin_vel_d", "root_euler_d", "foot_forces_grf")


def test_a1_tick_chain_replays_from_a_hip_graph():
    """An A1Tick chain without the solver (kinematics, plan + swing, EKF,
    terrain, torques from given forces), captured on one stream -- a linear
    chain, no parallel branches -- replays bit for bit."""
    dev = _dev()
    B = 67
    inp = a1ctrl.synth_inputs(41, B, 5)
    tick = lambda t: {k: _t(inp[k][t], dev) for k in TICK_KEYS}
    eager, graphed = a1ctrl.A1Tick(B, dev), a1ctrl.A1Tick(B, dev)
    static = tick(0)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):      # warm-up: initialises the filter and the buffers
        graphed.step(**static)
    eager.step(**tick(0))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        og = graphed.step(**static)
    for t in range(1, 5):
        for key, v in tick(t).items():
            static[key].copy_(v)
        g.replay()
        oe = eager.step(**tick(t))
        torch.cuda.synchronize()
        assert torch.equal(og.joint_torques, oe.joint_torques) and torch.equal(og.swing.contacts, oe.swing.contacts)
        assert torch.equal(og.state, oe.state) and torch.equal(og.terrain.terrain_pitch_angle, oe.terrain.terrain_pitch_angle)
        assert torch.equal(og.est.root_pos, oe.est.root_pos)
        assert torch.equal(graphed.ctrl.get_state(), eager.ctrl.get_state()), t
        for u, v in zip(graphed.est.state(), eager.est.state()):
            assert torch.equal(u, v), t
    assert torch.isfinite(og.joint_torques).all()


def test_a1_tick_with_the_qp_solver_runs_device_resident():
    """The whole tick with the section 9 QP as the solver: finite torques after
    the hold-off, contacts wired from plan_swing into the solver."""
    from quadrupedal_loco_amd import a1qp
    dev = _dev()
    B = 3
    inp = a1ctrl.synth_inputs(43, B, 12)
    qp = a1qp.A1QpBatch()
    solver = lambda state, contacts: qp.solve(state, contacts, stats=False).forces
    tk = a1ctrl.A1Tick(B, dev, solver=solver)
    for t in range(12):
        o = tk.step(**{k: _t(inp[k][t], dev) for k in TICK_KEYS if k != "foot_forces_grf"})
    torch.cuda.synchronize()
    assert torch.isfinite(o.joint_torques).all() and o.joint_torques.abs().max() > 0
    assert o.forces.shape == (B, 12)


def test_a1_tick_forces_are_the_qp_solution_of_its_own_state():
    """The tick's forces are what the section 9 QP returns on the record and
    the contacts the tick itself assembled (bit for bit, against a direct
    call), and they are the restatement's solution of that QP at the
    tolerance of tests/test_a1qp_gpu.py."""
    import a1qp_cases as AC
    from quadrupedal_loco_amd import a1qp
    dev = _dev()
    B = 3
    inp = a1ctrl.synth_inputs(43, B, 12)
    qp = a1qp.A1QpBatch()
    tk = a1ctrl.A1Tick(B, dev, solver=lambda state, contacts: qp.solve(state, contacts, stats=False).forces)
    for t in range(12):
        o = tk.step(**{k: _t(inp[k][t], dev) for k in TICK_KEYS if k != "foot_forces_grf"})
    torch.cuda.synchronize()
    direct = a1qp.A1QpBatch().solve(o.state, o.swing.contacts)
    torch.cuda.synchronize()
    assert o.forces.shape == (B, 12) and torch.equal(o.forces, direct.forces)
    S, CT = o.state.cpu().numpy(), o.swing.contacts.cpu().numpy()
    assert np.all(np.isfinite(S)) and CT.any()
    ref = AC.oracle_run(S, CT, {})
    tol, _ = AC.force_tolerance(ref, AC.sensitivity(S, CT, {}, ref))
    f, it = o.forces.cpu().numpy(), direct.iters.cpu().numpy()
    assert np.array_equal(direct.status.cpu().numpy(), ref["status"])
    assert np.all(np.abs(it - ref["iters"]) <= 25)
    d = np.abs(f - ref["forces"]).max(axis=1)
    print("a1 tick forces vs restatement: iters", it, ref["iters"], "|df|", d, "tol", tol)
    assert np.all(d <= np.where(it == ref["iters"], tol, 0.5)), (d, tol)


def test_a1_ctrl_cpp_shim_matches_c_abi():
    _dev()
    print(host_exe.run("test_a1_ctrl_host").stdout)
