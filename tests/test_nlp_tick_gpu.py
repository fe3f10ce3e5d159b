"""GPU tests of the batched planner tick (quadrupedal_loco_amd/nlp.py
PlannerTick, csrc/qloco_nlp_tick.hip) against the restatement
tests/nlp_tick_ref.py.

Bit-exact: right_support, the statuses, the integer members of the second
record, everything the step-timing kernel returns through qloco_nlp_tick
against a StepTimingPlanner run, the slots of com_traj NLPStepTimingBatch
already filled, everything between batch sizes, the get / set round trip and
the C++ shim against the Python path.

Bounded: the kernel is a third formulation beside the restatement's A and B
(A's order for the 7 x 7 system and the polynomials with correctly rounded
powers, pivoted LU for the 4 x 4 system, the device library's SQP), so each key is bounded at 16 x the A - B spread of nlp_tick_ref.SPREAD_TEACHER /
SPREAD_FREE (`python tests/nlp_tick_ref.py`; tests/test_nlp_tick.py checks that
they reproduce).  The keys the 4 x 4 system reaches are bounded per robot-tick
at 16 x max(pooled median, that tick's own A - B difference), see
nlp_tick_ref.PER_TICK_KEYS.  No robot and no tick is left out.
"""
import os

import numpy as np
import pytest

import host_exe
import nlp_ref as R
import nlp_tick_ref as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from quadrupedal_loco_amd import nlp, rt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _need_gpu():
    _dev()


def _t(a, dtype=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if dtype is None else a.astype(dtype)).to(_dev())


def _params(prm):
    return nlp.default_params(**{k: prm[k] for k in R.PARAM_ORDER})


def _planner(a):
    sqp = a["sqp"]
    return nlp.PlannerTick(len(sqp["steplength"]), _dev(), params=_params(sqp["params"]),
                           steplength=_t(sqp["steplength"]), stepwidth=_t(sqp["stepwidth"]),
                           stepheight=_t(a["stepheight"]))


def _tick(pl, a, t):
    sqp, inp = a["sqp"], a["sqp"]["inputs"]
    o = pl.tick(_t(sqp["t_int"][t]), _t(inp["est"][t]), _t(inp["rfoot"][t]), _t(inp["lfoot"][t]),
                stop_walking=_t(a["stop"][t]))
    torch.cuda.synchronize()
    s = o.step_timing
    return dict(com_traj=o.com_traj.cpu().numpy(), rlfoot=o.rlfoot_traj.cpu().numpy(),
                right_support=o.right_support.cpu().numpy(), status=o.status.cpu().numpy(),
                vari=s.vari_ini.cpu().numpy(), sched=s.sched.cpu().numpy(), step=s.step.cpu().numpy(),
                com=s.com.cpu().numpy(), pass_status=s.pass_status.cpu().numpy(), pass_iters=s.pass_iters.cpu().numpy())


INT_REC = [0, 2, 4]                     # _bjx1, _t_end_footstep, the last tick index


def _check(got, rec2, a, own, t, spreads, fig, what, worst):
    """One tick of every robot against formulation A."""
    for k in ("right_support", "status"):
        assert np.array_equal(got[k], a[k][t]), (what, t, k, got[k], a[k][t])
    assert np.array_equal(got["sched"], a["sqp"]["sched"][t]), (what, t)
    assert np.array_equal(rec2[:, INT_REC], a["rec2_out"][t][:, INT_REC]), (what, t)
    assert np.array_equal(rec2[:, 5:86], a["rec2_out"][t][:, 5:86]), (what, t)       # _footz_ref, lift heights, _tx0
    g = K.keyed(dict(com_traj=got["com_traj"], rlfoot=got["rlfoot"], rec2_out=rec2))
    w = K.keyed(dict(com_traj=a["com_traj"][t], rlfoot=a["rlfoot"][t], rec2_out=a["rec2_out"][t]))
    for k in g:
        assert np.array_equal(np.isfinite(g[k]), np.isfinite(w[k])), (what, t, k)
        d = np.where(np.isfinite(w[k]), np.abs(g[k] - w[k]), 0.0).max(axis=-1)
        bound = K.bound(spreads, k, own[k][t])
        fig[k] = max(fig.get(k, 0.0), float(d.max()))
        ratio = d / np.maximum(bound, 1e-300)
        worst[k] = max(worst.get(k, 0.0), float(np.where(bound > 0, ratio, np.where(d > 0, np.inf, 0.0)).max()))
    return g


def _report(name, mode, fig, worst):
    print(name, mode, "largest difference per key:", " ".join("%s %.3e" % kv for kv in fig.items()))
    print(name, mode, "largest difference / bound per key:", " ".join("%s %.3f" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (name, mode, k, v, fig[k])


@pytest.mark.parametrize("name", ["flat", "stepped", "stop"])
def test_teacher_forced_ticks(name):
    """Both records are set from the restatement before every tick."""
    a, _, own = K.pair(name, "teacher")
    T, B = a["status"].shape
    pl = _planner(a)
    fig, worst = {}, {}
    for t in range(T):
        pl.set_state(_t(a["sqp"]["record_in"][t]))
        pl.set_tick_state(_t(a["rec2_in"][t]))
        got = _tick(pl, a, t)
        _check(got, pl.get_tick_state().cpu().numpy(), a, own, t, K.SPREAD_TEACHER, fig, (name, "teacher"), worst)
    _report(name, "teacher-forced", fig, worst)


@pytest.mark.parametrize("name", ["flat", "stepped", "stop", "end"])
def test_free_running_rollout(name):
    """Nothing re-seeded: both records start from qloco_nlp_tick_init and only
    the pushes touch the first."""
    a, _, own = K.pair(name, "free")
    T, B = a["status"].shape
    pl = _planner(a)
    assert np.array_equal(pl.get_state().cpu().numpy(), a["sqp"]["record_in"][0])    # Initialize, bit for bit
    assert np.array_equal(pl.get_tick_state().cpu().numpy(), a["rec2_in"][0])
    fig, worst = {}, {}
    fa, fb = R.SLICES["feed"]
    push = a["sqp"]["inputs"]["push"]
    for t in range(T):
        if push[t].any():
            s = pl.get_state()
            s[:, fa:fb] += _t(push[t])
            pl.set_state(s)
        got = _tick(pl, a, t)
        _check(got, pl.get_tick_state().cpu().numpy(), a, own, t, K.SPREAD_FREE, fig, (name, "free"), worst)
    if name == "end":
        assert (got["right_support"] == 2).all() and not got["rlfoot"][:, 6:].any()
    _report(name, "free-running", fig, worst)


def test_pass_through_and_filled_slots():
    """What the step-timing kernel returns through qloco_nlp_tick, and its
    record afterwards, are the bits of a StepTimingPlanner run on the same
    inputs; the slots of com_traj NLPStepTimingBatch filled are unchanged."""
    a = K.rollout("stepped", K.A)
    T, B = a["status"].shape
    sqp = a["sqp"]
    full = _planner(a)
    alone = nlp.StepTimingPlanner(B, _dev(), params=_params(sqp["params"]), steplength=_t(sqp["steplength"]),
                                  stepwidth=_t(sqp["stepwidth"]))
    inp = sqp["inputs"]
    for t in range(24, 60):
        for pl in (full, alone):
            pl.set_state(_t(sqp["record_in"][t]))
        got = _tick(full, a, t)
        o = alone.tick(_t(sqp["t_int"][t]), _t(inp["est"][t]), _t(inp["rfoot"][t]), _t(inp["lfoot"][t]))
        torch.cuda.synchronize()
        want = dict(vari=o.vari_ini, sched=o.sched, step=o.step, com=o.com, pass_status=o.pass_status,
                    pass_iters=o.pass_iters, status=o.status)
        for k, v in want.items():
            assert np.array_equal(got[k], v.cpu().numpy()), (t, k)
        rec = full.get_state().cpu().numpy()
        assert np.array_equal(rec, alone.get_state().cpu().numpy()), t
        # NLPStepTimingBatch's slots (include/qloco.hpp): the CoM samples, _bjxx, the next two footholds, the step
        c, com, bj = got["com_traj"], got["com"], got["sched"][:, 2]
        fx, fy = rec[:, slice(*R.SLICES["footx_ref"])], rec[:, slice(*R.SLICES["footy_ref"])]
        rows = np.arange(B)
        assert np.array_equal(c[:, [0, 1, 3, 4, 6, 7]], com[:, 0:6])
        assert np.array_equal(c[:, [21, 22]], com[:, 10:12]) and np.array_equal(c[:, [24, 25]], com[:, 16:18])
        assert np.array_equal(c[:, 27], bj.astype(np.float64))
        assert np.array_equal(c[:, 28], fx[rows, bj]) and np.array_equal(c[:, 29], fx[rows, bj + 1])
        assert np.array_equal(c[:, 30], fy[rows, bj]) and np.array_equal(c[:, 31], fy[rows, bj + 1])
        z = np.zeros((B, R.NS))                          # :180, accumulated as the shim does
        for k in range(1, R.NS):
            z[:, k] = z[:, k - 1] + a["stepheight"]
        assert np.array_equal(c[:, 32], z[rows, bj]) and np.array_equal(c[:, 33], z[rows, bj + 1])
        assert np.array_equal(c[:, 34], got["sched"][:, 0] - 1.0) and np.array_equal(c[:, 35:38], got["step"])


def test_right_support_equals_support_phase():
    """right_support is qloco_support_phase's flag on the same ts / tx / t_int /
    t_end_footstep, on every tick of case 1."""
    a = K.rollout("flat", K.A)
    T, B = a["status"].shape
    pl = _planner(a)
    t_end = _t(np.full(B, R.t_end_footstep(), np.int32))
    fa, fb = R.SLICES["feed"]
    push = a["sqp"]["inputs"]["push"]
    for t in range(T):
        if push[t].any():
            s = pl.get_state()
            s[:, fa:fb] += _t(push[t])
            pl.set_state(s)
        got = _tick(pl, a, t)
        bjxx, bjx1, rs = rt.support_phase(pl.ts, pl.tx, _t(a["sqp"]["t_int"][t]), t_end)
        torch.cuda.synchronize()
        assert np.array_equal(got["right_support"], rs.cpu().numpy()), t
        assert np.array_equal(got["sched"][:, 2], bjxx.cpu().numpy()) and np.array_equal(got["sched"][:, 3], bjx1.cpu().numpy())


def _short_run(B, ticks=40, nan_robot=None, gw=1):
    prev = nlp.set_tick_group_width(gw)
    try:
        return _short_run_form(B, ticks, nan_robot)
    finally:
        nlp.set_tick_group_width(prev)


def _short_run_form(B, ticks, nan_robot):
    a = K.rollout("stepped", K.A)                        # only its inputs are used, tiled to 131 robots
    sqp = a["sqp"]
    idx = np.arange(131) % sqp["t_int"].shape[1]
    sl, sw = R.robot_inputs(31, 131)
    sh = a["stepheight"][idx]
    inp = R.tick_inputs(31, 131, ticks)
    pl = nlp.PlannerTick(B, _dev(), steplength=_t(sl[:B]), stepwidth=_t(sw[:B]), stepheight=_t(sh[:B]))
    outs = []
    for t in range(ticks):
        if nan_robot is not None and t == 30:
            s = pl.get_state()
            s[nan_robot, R.SLICES["feed"][0]] = float("nan")
            pl.set_state(s)
        o = pl.tick(_t(np.full(B, t + 1, np.int32)), _t(inp["est"][t, :B]), _t(inp["rfoot"][t, :B]),
                    _t(inp["lfoot"][t, :B]))
        torch.cuda.synchronize()
        outs.append(dict(com_traj=o.com_traj.cpu().numpy(), rlfoot=o.rlfoot_traj.cpu().numpy(),
                         right_support=o.right_support.cpu().numpy(), status=o.status.cpu().numpy(),
                         vari=o.step_timing.vari_ini.cpu().numpy()))
    return outs, pl.get_state().cpu().numpy(), pl.get_tick_state().cpu().numpy()


def test_batch_independence_and_nan_isolation():
    """Robot r's outputs and both records are the same bits at B = 1, 17, 67
    and 131 and in both kernel forms (40 ticks on stepped ground: one step
    boundary, the 7 x 7 system from tick 28 on, a swing); a robot with a NaN feed
    state reports QLOCO_NAN and its neighbours do not notice."""
    base, brec, brec2 = _short_run(131)
    for B, gw in ((1, 1), (17, 1), (67, 1), (1, 8), (17, 8), (67, 8), (131, 8)):    # both kernel forms
        outs, rec, rec2 = _short_run(B, gw=gw)
        assert np.array_equal(rec, brec[:B]) and np.array_equal(rec2, brec2[:B]), (B, gw)
        for t, o in enumerate(outs):
            for k, v in o.items():
                assert np.array_equal(v, base[t][k][:B], equal_nan=True), (B, gw, t, k)
    bad = 5
    outs, rec, rec2 = _short_run(67, nan_robot=bad)
    others = np.arange(67) != bad
    assert np.array_equal(rec[others], brec[:67][others]) and np.array_equal(rec2[others], brec2[:67][others])
    for t, o in enumerate(outs):
        for k, v in o.items():
            assert np.array_equal(v[others], base[t][k][:67][others]), (t, k)
        if t >= 30:
            assert o["status"][bad] == R.NAN and np.isnan(o["com_traj"][bad][[0, 9, 11]]).all(), (t, o["status"][bad])
        else:
            assert o["status"][bad] == R.OK


def test_outside_the_plan_leaves_both_records_untouched():
    a = K.rollout("stop", K.A)
    B = a["status"].shape[1]
    pl = _planner(a)
    pl.set_state(_t(a["sqp"]["record_out"][-1]))
    pl.set_tick_state(_t(a["rec2_out"][-1]))
    ti = np.full(B, 27 * 40, np.int32)
    ti[0] = a["sqp"]["t_int"][-1, 0] + 1                 # one robot still inside the plan
    ti[1] = 0                                            # i < 1
    z6 = torch.zeros((B, 6), dtype=torch.float64, device=_dev())
    z2 = torch.zeros((B, 2), dtype=torch.float64, device=_dev())
    o = pl.tick(_t(ti), z6, z2, z2)
    torch.cuda.synchronize()
    st = o.status.cpu().numpy()
    assert st[0] == 0 and st[1] == R.BAD and (st[2:] == nlp.FINISHED).all(), st
    r1, r2 = pl.get_state().cpu().numpy(), pl.get_tick_state().cpu().numpy()
    assert np.array_equal(r1[1:], a["sqp"]["record_out"][-1][1:]) and np.array_equal(r2[1:], a["rec2_out"][-1][1:])
    assert not np.array_equal(r2[0], a["rec2_out"][-1][0])
    assert np.isnan(o.com_traj.cpu().numpy()[1:]).all() and np.isnan(o.rlfoot_traj.cpu().numpy()[1:]).all()
    assert (o.right_support.cpu().numpy()[1:] == 2).all()
    assert np.isfinite(o.com_traj.cpu().numpy()[0]).all() and np.isfinite(o.rlfoot_traj.cpu().numpy()[0]).all()


def test_tick_state_round_trip():
    rng = np.random.default_rng(4)
    B = 67
    s = rng.normal(size=(B, nlp.TICK_STATE))
    pl = nlp.PlannerTick(B, _dev())
    before = pl.get_state().cpu().numpy()
    pl.set_tick_state(_t(s))
    assert np.array_equal(pl.get_tick_state().cpu().numpy(), s)
    assert np.array_equal(pl.get_state().cpu().numpy(), before)          # the first record is another workspace


def test_cpp_shim_matches_python_path():
    """qloco::NLPClassBatch for B = 1 over the first 12 ticks on stepped
    ground: the 38-vector, the 18-vector and right_support are the Python
    path's bits."""
    _dev()
    ticks, sh = 12, 0.02
    inp = R.tick_inputs(41, 1, ticks)
    r = host_exe.run("test_nlp_tick_host", [ticks, repr(sh)], input="\n".join(
        " ".join(repr(float(x)) for x in np.concatenate([inp["est"][t, 0], inp["rfoot"][t, 0], inp["lfoot"][t, 0]]))
        for t in range(ticks)))
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("T ")]
    assert len(rows) == ticks
    pl = nlp.PlannerTick(1, _dev(), steplength=0.075, stepwidth=2 * 0.12675, stepheight=sh)
    for t in range(ticks):
        row = rows[t]
        assert row[39] == "|" and row[58] == "|", row
        c = np.array([float.fromhex(x) for x in row[1:39]])
        f = np.array([float.fromhex(x) for x in row[40:58]])
        o = pl.tick(_t(np.full(1, t + 1, np.int32)), _t(inp["est"][t]), _t(inp["rfoot"][t]), _t(inp["lfoot"][t]))
        torch.cuda.synchronize()
        assert np.array_equal(c, o.com_traj.cpu().numpy()[0]), (t, c, o.com_traj.cpu().numpy()[0])
        assert np.array_equal(f, o.rlfoot_traj.cpu().numpy()[0]), t
        assert int(row[59]) == int(o.right_support.cpu().numpy()[0]), t
