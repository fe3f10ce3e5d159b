"""GPU tests of the batched step-timing SQP (quadrupedal_loco_amd/nlp.py,
csrc/qloco_nlp.hip) against the restatement tests/nlp_ref.py.

Bit-exact: the integer outputs (_periond_i, _k_yu, _bjxx, _bjx1), the per-pass
codes (solved / infeasible / skipped) and iteration counts, the record after
qloco_nlp_init, everything between batch sizes and group widths.

Bounded: the transcendental steps (cosh / sinh / log of the device library)
cannot be bit-identical with libm.  SPREAD_TEACHER / SPREAD_FREE hold the
largest difference between the restatement's two formulations of them
(SPREAD_BLEND: over the feedback-blend case, which this file adds to the two
windows), measured on the CPU over exactly the inputs of the tests below
(`python tests/nlp_ref.py`; tests/test_nlp.py checks that the figures
reproduce); the kernel is a third formulation, so each bound is 16 x the
measured spread of that key (the convention of tests/test_a1_ctrl_gpu.py).
"""
import os

import numpy as np
import pytest

import host_exe
import nlp_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from quadrupedal_loco_amd import nlp, rt  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")

# python tests/nlp_ref.py
SPREAD_TEACHER = dict(
    vari=7.105e-15, step=2.220e-16, com=3.553e-15, rec_ts=2.220e-16, rec_tx=3.553e-15, rec_td=5.551e-17,
    rec_Lxx_ref=1.388e-17, rec_Lyy_ref=5.551e-17, rec_footx_ref=1.388e-17, rec_footy_ref=5.551e-17,
    rec_COMx_is=0.0, rec_COMvx_is=3.469e-17, rec_COMy_is=0.0, rec_COMvy_is=1.332e-15, rec_vari=7.105e-15,
    rec_feed=2.665e-15, rec_endref=1.421e-14)
SPREAD_BLEND = dict(
    vari=1.865e-14, step=6.661e-16, com=1.332e-15, rec_ts=6.661e-16, rec_tx=3.553e-15, rec_td=1.388e-16,
    rec_Lxx_ref=1.665e-16, rec_Lyy_ref=1.110e-16, rec_footx_ref=1.665e-16, rec_footy_ref=1.110e-16,
    rec_COMx_is=0.0, rec_COMvx_is=3.469e-17, rec_COMy_is=0.0, rec_COMvy_is=5.690e-16, rec_vari=1.865e-14,
    rec_feed=6.661e-16, rec_endref=1.332e-15)
SPREAD_FREE = dict(
    vari=3.908e-14, step=5.829e-15, com=1.172e-13, rec_ts=7.772e-16, rec_tx=3.553e-15, rec_td=1.388e-16,
    rec_Lxx_ref=2.776e-17, rec_Lyy_ref=5.829e-15, rec_footx_ref=2.776e-17, rec_footy_ref=5.829e-15,
    rec_COMx_is=1.388e-17, rec_COMvx_is=1.596e-16, rec_COMy_is=2.942e-15, rec_COMvy_is=1.643e-14,
    rec_vari=3.908e-14, rec_feed=9.059e-14, rec_endref=6.750e-14)


def _params(prm):
    return nlp.default_params(**{k: prm[k] for k in R.PARAM_ORDER})


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) if dtype is None else \
        torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(_dev())


def _tick(pl, ref, t, sel=slice(None)):
    inp = ref["inputs"]
    o = pl.tick(_t(ref["t_int"][t, sel]), _t(inp["est"][t, sel]), _t(inp["rfoot"][t, sel]), _t(inp["lfoot"][t, sel]))
    torch.cuda.synchronize()
    return dict(vari=o.vari_ini.cpu().numpy(), sched=o.sched.cpu().numpy(), step=o.step.cpu().numpy(),
                com=o.com.cpu().numpy(), pass_status=o.pass_status.cpu().numpy(),
                pass_iters=o.pass_iters.cpu().numpy(), status=o.status.cpu().numpy())


def _values(got, rec):
    d = {k: got[k] for k in R.OUT_KEYS}
    for k in R.REC_KEYS:
        a, b = R.SLICES[k]
        d["rec_" + k] = rec[:, a:b]
    return d


def _ref_values(ref, t):
    d = {k: ref[k][t] for k in R.OUT_KEYS}
    for k in R.REC_KEYS:
        a, b = R.SLICES[k]
        d["rec_" + k] = ref["record_out"][t][:, a:b]
    return d


def _check_values(got, want, spreads, rows, fig, what):
    for k, g in got.items():
        w = want[k]
        d = np.abs(g[rows] - w[rows])
        assert np.isfinite(g[rows]).all() and np.isfinite(w[rows]).all(), (what, k)
        m = float(d.max()) if d.size else 0.0
        fig[k] = max(fig.get(k, 0.0), m)
        assert m <= 16 * spreads[k], (what, k, m, spreads[k])


def _ints_equal(got, ref, t):
    return ((got["sched"] == ref["sched"][t]).all(1) & (got["pass_status"] == ref["pass_status"][t]).all(1)
            & (got["pass_iters"] == ref["pass_iters"][t]).all(1) & (got["status"] == ref["status"][t]))


def _teacher(ref, name, spreads=None):
    spreads = SPREAD_TEACHER if spreads is None else spreads
    T, B = ref["t_int"].shape
    pl = nlp.StepTimingPlanner(B, _dev(), params=_params(ref["params"]))
    fig = {}
    rows = np.ones(B, bool)
    for t in range(T):
        pl.set_state(_t(ref["record_in"][t]))
        got = _tick(pl, ref, t)
        for k in ("sched", "pass_status", "pass_iters", "status"):
            assert np.array_equal(got[k], ref[k][t]), (name, t, k, got[k], ref[k][t])
        _check_values(_values(got, pl.get_state().cpu().numpy()), _ref_values(ref, t), spreads, rows, fig,
                      (name, t))
    print(name, "teacher-forced, largest difference per key:", " ".join("%s %.3e" % kv for kv in fig.items()))


def test_teacher_forced_ticks():
    """67 robots (16 groups of a wave and a partial one at four lanes per
    robot), 90 ticks from i = 1, the device record set from the restatement's
    before every tick."""
    _teacher(R.rollout(**dict(R.cases())["main"]), "main")


def test_feedback_blend():
    """_lamda_* = 0.02 / 0.002 across the first step boundary, teacher-forced:
    estimated_state and both foot-location feedbacks reach the feed state."""
    ref = R.rollout(**dict(R.cases())["blend"])
    assert ref["params"]["lamda_comx"] == 0.02 and len(set(ref["sched"][:, 0, 0])) == 2
    _teacher(ref, "blend", SPREAD_BLEND)


def test_free_running_rollout():
    """The same inputs, nothing re-seeded: the record starts from
    qloco_nlp_init and only the pushes touch it."""
    ref = R.rollout(**dict(R.cases())["main"])
    T, B = ref["t_int"].shape
    pl = nlp.StepTimingPlanner(B, _dev(), params=_params(ref["params"]), steplength=_t(ref["steplength"]),
                               stepwidth=_t(ref["stepwidth"]))
    assert np.array_equal(pl.get_state().cpu().numpy(), ref["record_in"][0])    # Initialize, bit for bit
    alive = np.ones(B, bool)
    dropped_solves = 0
    fig = {}
    a, b = R.SLICES["feed"]
    for t in range(T):
        if ref["inputs"]["push"][t].any():
            s = pl.get_state()
            s[:, a:b] += _t(ref["inputs"]["push"][t])
            pl.set_state(s)
        got = _tick(pl, ref, t)
        same = _ints_equal(got, ref, t)
        newly = alive & ~same
        dropped_solves += int(newly.sum()) * 3 * (T - t)
        alive &= same
        rec = pl.get_state().cpu().numpy()
        _check_values(_values(got, rec), _ref_values(ref, t), SPREAD_FREE, alive, fig, ("free", t))
        assert np.isfinite(got["vari"]).all() and np.isfinite(rec).all(), t      # dropped robots stay finite
    print("free-running, largest difference per key:", " ".join("%s %.3e" % kv for kv in fig.items()),
          "| robots dropped:", int((~alive).sum()))
    assert dropped_solves <= 0.01 * 3 * T * B, dropped_solves


def test_late_window_and_plan_end():
    """Steps 15-16, where _steplength changes sign, teacher-forced; then a
    robot past its last step: "plan finished", NaN outputs, record untouched."""
    ref = R.rollout(**dict(R.cases())["late"])
    _teacher(ref, "late")
    T, B = ref["t_int"].shape
    pl = nlp.StepTimingPlanner(B, _dev(), params=_params(ref["params"]))
    rec = ref["record_out"][-1]
    pl.set_state(_t(rec))
    ti = np.full(B, 27 * 40, np.int32)
    ti[0] = ref["t_int"][-1, 0] + 1                      # one robot still inside the plan
    ti[1] = 0                                            # i < 1
    z6, z2 = torch.zeros((B, 6), dtype=torch.float64, device=_dev()), torch.zeros((B, 2), dtype=torch.float64, device=_dev())
    o = pl.tick(_t(ti), z6, z2, z2)
    torch.cuda.synchronize()
    st = o.status.cpu().numpy()
    assert st[0] == 0 and st[1] == R.BAD and (st[2:] == nlp.FINISHED).all(), st
    after = pl.get_state().cpu().numpy()
    assert np.array_equal(after[1:], rec[1:]) and not np.array_equal(after[0], rec[0])
    assert np.isnan(o.vari_ini.cpu().numpy()[1:]).all() and np.isnan(o.com.cpu().numpy()[1:]).all()
    assert (o.pass_status.cpu().numpy()[1:] == nlp.SKIPPED).all()
    assert (o.sched.cpu().numpy()[2:, 0] == 27).all()


def _short_run(B, ticks=12, nan_robot=None, gw=4):
    sl, sw = R.robot_inputs(31, 131)
    inp = R.tick_inputs(31, 131, ticks)
    prev = nlp.set_group_width(gw)
    try:
        pl = nlp.StepTimingPlanner(B, _dev(), steplength=_t(sl[:B]), stepwidth=_t(sw[:B]))
        outs = []
        for t in range(ticks):
            if nan_robot is not None and t == 3:
                s = pl.get_state()
                s[nan_robot, R.SLICES["feed"][0]] = float("nan")
                pl.set_state(s)
            ref = dict(t_int=np.full((ticks, B), 1, np.int32) + np.arange(ticks, dtype=np.int32)[:, None],
                       inputs={k: v[:, :B] for k, v in inp.items()})
            outs.append(_tick(pl, ref, t))
        rec = pl.get_state().cpu().numpy()
    finally:
        nlp.set_group_width(prev)
    return outs, rec


def test_batch_independence_and_nan_isolation():
    """Robot r's outputs and record are the same bits at B = 1, 17, 67, 131
    and at every group width; a robot with a NaN feed state reports it and its
    neighbours do not notice."""
    base, brec = _short_run(131)
    for B, gw in ((1, 4), (17, 4), (67, 4), (67, 8), (17, 16)):
        outs, rec = _short_run(B, gw=gw)
        assert np.array_equal(rec, brec[:B]), (B, gw)
        for t, o in enumerate(outs):
            for k, v in o.items():
                assert np.array_equal(v, base[t][k][:B]), (B, gw, t, k)
    bad = 5
    outs, rec = _short_run(67, nan_robot=bad)
    others = np.arange(67) != bad
    assert np.array_equal(rec[others], brec[:67][others])
    for t, o in enumerate(outs):
        for k, v in o.items():
            assert np.array_equal(v[others], base[t][k][:67][others]), (t, k)
        if t >= 3:
            # the NaN went into _comx_feed: the x half of the CoM samples (comx, comvx, comax)
            assert o["status"][bad] == R.NAN and np.isnan(o["com"][bad][0::2]).all(), (t, o["status"][bad])
    assert np.isnan(rec[bad]).any()


def test_get_set_round_trip_and_lockstep():
    rng = np.random.default_rng(3)
    B = 67
    s = rng.normal(size=(B, nlp.STATE))
    a, b = nlp.StepTimingPlanner(B, _dev()), nlp.StepTimingPlanner(B, _dev())
    a.set_state(_t(s))
    assert np.array_equal(a.get_state().cpu().numpy(), s)
    # the (B, 27) views are the record's first two fields
    assert np.array_equal(a.ts.cpu().numpy(), s[:, 0:27]) and np.array_equal(a.tx.cpu().numpy(), s[:, 27:54])
    assert set(nlp.STATE_FIELDS) == set(R.SLICES) and all(nlp.STATE_FIELDS[k] == R.SLICES[k] for k in R.SLICES)
    ref = R.rollout(**dict(R.cases())["main"])
    a.set_state(_t(ref["record_in"][30]))
    b.set_state(a.get_state())
    for t in range(30, 36):
        oa, ob = _tick(a, ref, t), _tick(b, ref, t)
        for k in oa:
            assert np.array_equal(oa[k], ob[k], equal_nan=True), (t, k)
        assert np.array_equal(a.get_state().cpu().numpy(), b.get_state().cpu().numpy())


def test_tick_chains_into_support_phase():
    """tick, then qloco_support_phase on the planner's ts / tx views (no copy):
    the flags equal the oracle's on the restatement's schedule wherever the
    restatement is clear of every decision boundary (tests/test_nlp.py checks
    the selection)."""
    ref = R.rollout(**dict(R.cases())["main"])
    T, B = ref["t_int"].shape
    pl = nlp.StepTimingPlanner(B, _dev(), params=_params(ref["params"]))
    mask = R.chain_mask(ref)
    t_end = np.full(B, R.t_end_footstep(), np.int32)
    checked = 0
    for t in range(0, T, 3):
        pl.set_state(_t(ref["record_in"][t]))
        _tick(pl, ref, t)
        ti = _t(ref["t_int"][t])
        bjxx, bjx1, rs = rt.support_phase(pl.ts, pl.tx, ti, _t(t_end))
        torch.cuda.synchronize()
        a, b = R.SLICES["ts"], R.SLICES["tx"]
        want = O.support_phase(ref["record_out"][t][:, a[0]:a[1]], ref["record_out"][t][:, b[0]:b[1]],
                               ref["t_int"][t], t_end)
        m = mask[t]
        for g, w in zip((bjxx, bjx1, rs), want):
            assert np.array_equal(g.cpu().numpy()[m], np.asarray(w)[m]), t
        checked += int(m.sum())
    assert checked >= 0.9 * B * len(range(0, T, 3))


def test_cpp_shim_matches_python_path(tmp_path):
    """qloco::NLPStepTimingBatch::step_timing_opti_loop for B = 1: the filled
    slots of the 38-vector are the Python path's bits, the listed ones NaN."""
    _dev()
    ticks = 40
    sl, sw = 0.075, 2 * 0.12675
    inp = R.tick_inputs(41, 1, ticks)
    r = host_exe.run("test_nlp_host", [ticks], input="\n".join(
        " ".join(repr(float(x)) for x in np.concatenate([inp["est"][t, 0], inp["rfoot"][t, 0], inp["lfoot"][t, 0]]))
        for t in range(ticks)))
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("T ")]
    assert len(rows) == ticks
    got = np.array([[float.fromhex(x) if x not in ("nan", "-nan") else np.nan for x in row[1:]] for row in rows])
    pl = nlp.StepTimingPlanner(1, _dev(), steplength=sl, stepwidth=sw)
    nan_slots = [2, 5, 8] + list(range(9, 21)) + [23, 26]
    for t in range(ticks):
        ref = dict(t_int=np.full((ticks, 1), 1, np.int32) + np.arange(ticks, dtype=np.int32)[:, None], inputs=inp)
        o = _tick(pl, ref, t)
        rec = pl.get_state().cpu().numpy()[0]
        fx, fy = rec[slice(*R.SLICES["footx_ref"])], rec[slice(*R.SLICES["footy_ref"])]
        com, bj = o["com"][0], int(o["sched"][0, 2])
        want = np.full(38, np.nan)
        want[[0, 1, 3, 4, 6, 7]] = com[0:6]
        want[[21, 22]] = com[10:12]
        want[[24, 25]] = com[16:18]
        want[27] = bj
        want[28:32] = fx[bj], fx[bj + 1], fy[bj], fy[bj + 1]
        want[32:34] = 0.0                                  # _footz_ref with stepheight 0
        want[34] = o["sched"][0, 0] - 1
        want[35:38] = o["step"][0]
        assert np.isnan(got[t][nan_slots]).all(), t
        assert np.array_equal(got[t], want, equal_nan=True), (t, got[t], want)
