"""GPU tests of the batched planner node tick (quadrupedal_loco_amd/nlp.py
PlannerNode, csrc/qloco_nlp_node.hip) against the restatement
tests/nlp_node_ref.py.

Teacher-forced on the device's own planner tick: after every node tick the
inner tick's outputs and both planner records are read back and the row is
rebuilt from them by formulation A.  Bit-exact: every slot that is a copy (0..14
and 27..99 of a walking row, all of a not-started, over-time or stopped row,
all but the three polynomial slots of a squat row), the branch, the counters,
the inner tick against a standalone PlannerTick, both row-store forms, every
batch size against every other, the get / set round trip, the consumers'
outputs when chained, the C++ shim against the Python path.  Bounded: squat
slots 2, 38, 41 and slots 15..26, at 16 x max(the pooled A - B spread of the key,
nlp_node_ref.SPREAD, that robot-tick's own A - B difference).  No robot and no
tick is left out.
"""
import copy
import os

import numpy as np
import pytest

import go1_servo_ref as G
import host_exe
import nlp_node_ref as N
import nlp_ref as R
import nlp_tick_ref as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from quadrupedal_loco_amd import go1servo, nlp, rt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 17, 67, 131)
LEAD = N.LEAD                           # one tick not started, 40 of squat
HW = 0.12675


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


# ---- robots by identity: a robot's inputs depend on its id alone, not on the batch it rides in
IDS = np.arange(131)
STEPLENGTH = 0.04 + 0.05 * ((IDS * 37) % 101) / 101
STEPWIDTH = 2 * HW * (0.9 + 0.2 * ((IDS * 53) % 97) / 97)
# Flat ground only for the five robots 42, 45, .. 54 of the parity test.  A robot on flat ground stands still
# through its first step: its ZMP samples there are zeros and rounding noise, _Co of the first double support
# is noise over noise and NaN where that is 0 / 0 (nlp_node_ref.SEEDS).  The parity test takes whatever
# comes, on both sides; the tests that compare runs with each other keep to stepped ground.
FLAT = (IDS % 3 == 0) & (IDS >= 40) & (IDS < 57)
STEPHEIGHT = np.where(FLAT, 0.0, np.array([1.0, 1.0, -1.0])[IDS % 3] * (0.01 + 0.02 * ((IDS * 29) % 89) / 89))
N_MAX = LEAD + 90


def _noise(g):
    """(N_MAX, 25) of robot g: [1:19] a state estimate the node must not pass
    on, [19:22] / [22:25] the left / right foot feedback."""
    rng = np.random.default_rng(7000 + int(g))
    m = rng.normal(0.0, 0.02, (N_MAX, 25))
    m[:, 19:22] = [0.0, HW, 0.0] + rng.normal(0, 0.002, (N_MAX, 3))
    m[:, 22:25] = [0.0, -HW, 0.0] + rng.normal(0, 0.002, (N_MAX, 3))
    return m


NOISE = {}


def _msg(ids, n, start):
    """The /rt2nrt/state rows of tick n; start: per-robot msg[0]."""
    for g in ids:
        if g not in NOISE:
            NOISE[g] = _noise(g)
    m = np.stack([NOISE[g][n] for g in ids])
    m[:, 0] = start
    return m


def _node(ids, **prm):
    ids = np.asarray(ids)
    return nlp.PlannerNode(len(ids), _dev(), params=nlp.default_params(**prm) if prm else None,
                           steplength=_t(STEPLENGTH[ids]), stepwidth=_t(STEPWIDTH[ids]),
                           stepheight=_t(STEPHEIGHT[ids]))


def _read(node, out):
    torch.cuda.synchronize()
    s = {k: v.cpu().numpy().copy() for k, v in node.scratch().items()}
    return dict(row=out.gait_msg.cpu().numpy().copy(), sched=out.sched.cpu().numpy().copy(),
                status=out.status.cpu().numpy().copy(), scratch=s, rec14=node.get_state().cpu().numpy(),
                rec15=node.get_tick_state().cpu().numpy(), rec17=node.get_node_state().cpu().numpy())


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


class Checker:
    """Formulation A beside a device node, robot by robot: its state runs free,
    fed with the device's planner tick."""

    def __init__(self, node, prm=None):
        self.p = prm or R.params()
        self.tp, self.npar = dict(K.TICK_DEFAULTS), dict(N.NODE_DEFAULTS)
        self.B = node.batch
        self.st = [N.NodeState(self.p) for _ in range(self.B)]
        self.rec14 = node.get_state().cpu().numpy()
        self.rec15 = node.get_tick_state().cpu().numpy()
        self.fig, self.worst, self.census = {}, {}, {}
        self.rows = None

    def tick(self, msg, got, what):
        td = slice(*R.SLICES["td"])
        sc = got["scratch"]
        rows = np.zeros((self.B, 100))
        for b in range(self.B):
            st = self.st[b]
            branch, w1, ti = N.pre(st, msg[b, 0], self.p, self.npar)
            assert got["sched"][b, :3].tolist() == [branch, w1, ti] and sc["t_int"][b] == ti, (what, b, got["sched"][b])
            assert got["sched"][b, 5] == st.count and sc["branch"][b] == branch, (what, b)
            self.census[branch] = self.census.get(branch, 0) + 1
            kw = {}
            if branch == N.WALKING:
                b0, td1 = int(self.rec15[b, 0]), float(self.rec14[b][td][1])
                assert sc["prev"][b].tolist() == [b0, td1], (what, b)
                kw = dict(tick=dict(com_traj=sc["com_traj"][b], rlfoot=sc["rlfoot_traj"][b],
                                    right_support=sc["right_support"][b], sched=sc["sched"][b],
                                    status=sc["status"][b]),
                          rec14=got["rec14"][b], rec15=got["rec15"][b], b0=b0, td1=td1)
                assert _same(sc["rfoot_feedback"][b], msg[b, 22:24]) and _same(sc["lfoot_feedback"][b], msg[b, 19:21])
            else:
                # a robot that does not walk leaves both planner records as they were
                assert _same(got["rec14"][b], self.rec14[b]) and _same(got["rec15"][b], self.rec15[b]), (what, b)
            before = copy.deepcopy(st) if branch in (N.SQUAT, N.WALKING) else None
            row, info = N.post(st, branch, w1, N.A, self.p, self.tp, self.npar, **kw)
            rows[b] = row
            g = got["row"][b]
            assert np.isfinite(g[[k for k in range(100) if not 87 <= k <= 92]]).all() or info["status"] != R.OK, (what, b)
            assert got["status"][b] == info["status"] == got["sched"][b, 4], (what, b, got["status"][b], info)
            assert got["sched"][b, 3] == int(row[27]) and got["sched"][b, 6] == info["ntd"], (what, b)
            assert got["sched"][b, 7] == info["kend"], (what, b, got["sched"][b], info)
            bounded = {}
            if branch == N.SQUAT:
                bounded = {k: [s] for k, s in N.SQUAT_SLOTS.items()}
            elif branch == N.WALKING:
                bounded = dict(force=list(N.FORCE_SLOTS), moment=list(N.MOMENT_SLOTS))
            loose = [s for v in bounded.values() for s in v]
            exact = [k for k in range(100) if k not in loose]
            assert _same(g[exact], row[exact]), (what, b, branch, [k for k in exact if not _same(g[k], row[k])])
            if bounded:
                rowb, _ = N.post(before, branch, w1, N.B, self.p, self.tp, self.npar, **kw)
                for key, slots in bounded.items():
                    assert np.array_equal(np.isfinite(g[slots]), np.isfinite(row[slots])), (what, b, key)
                    fin = np.isfinite(row[slots])
                    d = float(np.where(fin, np.abs(g[slots] - row[slots]), 0.0).max())
                    own = float(np.where(fin & np.isfinite(rowb[slots]), np.abs(row[slots] - rowb[slots]), 0.0).max())
                    self.fig[key] = max(self.fig.get(key, 0.0), d)
                    self.worst[key] = max(self.worst.get(key, 0.0), d / float(N.bound(key, own)))
            # the node record: the counters and the row it carries
            r17 = got["rec17"][b]
            assert r17[:4].tolist() == [st.count, float(st.latch), st.restart, st.mpc_stop], (what, b, r17[:4])
            assert _same(r17[154:254], g), (what, b)
        self.rec14, self.rec15, self.rows = got["rec14"], got["rec15"], rows

    def report(self, what):
        print(what, "largest difference per key:", " ".join("%s %.3e" % kv for kv in self.fig.items()))
        print(what, "largest difference / bound per key:", " ".join("%s %.4f" % kv for kv in self.worst.items()))
        for k, v in self.worst.items():
            assert v <= 1.0, (what, k, v, self.fig[k])


def test_teacher_forced_row_parity():
    """17 robots on flat and stepped ground, started together: one tick not
    started, the squat, 90 walking ticks across three step boundaries."""
    ids = np.arange(40, 57)
    node = _node(ids)
    chk = Checker(node)
    for n in range(LEAD + 90):
        msg = _msg(ids, n, 0.0 if n == 0 else 1.0)
        chk.tick(msg, _read(node, node.tick(_t(msg))), ("parity", n))
    assert chk.census == {N.NOT_STARTED: 17, N.SQUAT: 40 * 17, N.WALKING: 90 * 17}
    assert set(chk.worst) == set(N.KEYS)
    chk.report("teacher-forced row parity, B = 17:")


def test_inner_tick_is_the_standalone_tick():
    """The node's inner tick against a PlannerTick of its own given the node's
    t_int, zeros for estimated_state and the message's foot feedback -- with the
    feedback blend switched on, so that estimated_state and the feedback reach
    the result: outputs and both records, bit for bit."""
    ids = np.arange(17)
    lam = dict(lamda_comx=0.02, lamda_comvx=0.002, lamda_comy=0.02, lamda_comvy=0.002)
    node = _node(ids, **lam)
    alone = nlp.PlannerTick(17, _dev(), params=nlp.default_params(**lam), steplength=_t(STEPLENGTH[ids]),
                            stepwidth=_t(STEPWIDTH[ids]), stepheight=_t(STEPHEIGHT[ids]))
    wrong = nlp.PlannerTick(17, _dev(), params=nlp.default_params(**lam), steplength=_t(STEPLENGTH[ids]),
                            stepwidth=_t(STEPWIDTH[ids]), stepheight=_t(STEPHEIGHT[ids]))
    differs = False
    for n in range(LEAD + 34):
        start = np.where(ids % 4 == 3, 0.0, 1.0) if n > 0 else 0.0     # every fourth robot never starts
        msg = _msg(ids, n, start)
        node.tick(_t(msg))
        torch.cuda.synchronize()
        sc = {k: v.cpu().numpy().copy() for k, v in node.scratch().items()}
        ti = _t(sc["t_int"])
        o = alone.tick(ti, _t(np.zeros((17, 6))), _t(msg[:, 22:24]), _t(msg[:, 19:21]))
        torch.cuda.synchronize()
        want = dict(com_traj=o.com_traj, rlfoot_traj=o.rlfoot_traj, right_support=o.right_support, status=o.status,
                    sched=o.step_timing.sched, vari_ini=o.step_timing.vari_ini, com=o.step_timing.com)
        for k, v in want.items():
            assert _same(sc[k], v.cpu().numpy()), (n, k)
        assert _same(node.get_state().cpu().numpy(), alone.get_state().cpu().numpy()), n
        assert _same(node.get_tick_state().cpu().numpy(), alone.get_tick_state().cpu().numpy()), n
        walking = sc["t_int"] >= 1
        assert (sc["status"][~walking] == 4).all() and (sc["status"][walking] == 0).all(), n    # QLOCO_BAD_SIZE
        # the callback's estimate instead of the member's zeros gives another tick
        w = wrong.tick(ti, _t(msg[:, 1:7]), _t(msg[:, 22:24]), _t(msg[:, 19:21]))
        differs = differs or not _same(w.com_traj.cpu().numpy(), sc["com_traj"])
    assert differs and walking.sum() == 13


def test_start_gating():
    """Robots of one batch start at different ticks, one is never started and
    one is started by a single message: each count advances with its own
    messages only, a robot that does not walk leaves the planner records
    byte-identical (Checker), and no NaN of its scratch reaches its row."""
    ids = np.arange(100, 117)
    first = ids % 6                      # the tick of the first msg[0] > 0; 5: never
    node = _node(ids)
    chk = Checker(node)
    counts = np.zeros(17)
    for n in range(LEAD + 6):
        start = np.where((first < 5) & (n >= first), 1.0 + n, -1.0)
        start[3] = 2.0 if n == 4 else 0.0                           # one message, then silence: the latch holds
        counts += start > 0
        msg = _msg(ids, n, start)
        got = _read(node, node.tick(_t(msg)))
        chk.tick(msg, got, ("gating", n))
        assert np.isfinite(got["row"]).all(), n
        assert np.isnan(got["scratch"]["com_traj"][got["scratch"]["t_int"] == 0]).all(), n
        assert got["rec17"][:, 0].tolist() == counts.tolist(), n
    # started at tick f, a robot has counted LEAD + 6 - f > 40 messages by now
    assert got["sched"][:, 0].tolist() == [N.SQUAT if b == 3 else N.NOT_STARTED if f == 5 else N.WALKING
                                           for b, f in enumerate(first.tolist())]
    assert got["sched"][3, 1] == 1 and chk.census[N.WALKING] > 0


def _rollout(ids, ticks, form=None, poison=None, states=None, first_tick=0):
    """Rows, statuses and the three records after `ticks` ticks, all started at tick 1."""
    node = _node(ids)
    if states is not None:
        node.set_state(_t(states[0]))
        node.set_tick_state(_t(states[1]))
        node.set_node_state(_t(states[2]))
    prev = nlp.set_node_form(form) if form is not None else None
    rows, status = [], []
    try:
        for n in range(first_tick, first_tick + ticks):
            if poison is not None:
                poison(node, n)
            o = node.tick(_t(_msg(ids, n, 0.0 if n == 0 else 1.0)))
            rows.append(o.gait_msg.clone())
            status.append(o.status.clone())
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            nlp.set_node_form(prev)
    recs = [node.get_state().cpu().numpy(), node.get_tick_state().cpu().numpy(), node.get_node_state().cpu().numpy()]
    return torch.stack(rows).cpu().numpy(), torch.stack(status).cpu().numpy(), recs


def test_nan_isolation():
    """One robot's planner record and another's node record are made
    non-finite through set_state: both report QLOCO_NAN, every other robot's
    rows are the clean run's bits."""
    ids = np.arange(20, 37)
    T = LEAD + 34                        # into the double support of step 2, where the ring is read

    def poison(node, n):
        if n == LEAD + 4:
            s = node.get_state()
            s[5, slice(*R.SLICES["feed"])] = float("nan")
            node.set_state(s)
        if n == LEAD + 27:
            s = node.get_node_state()
            s[9, 10 + 1:154:3] = float("nan")                       # every _zmpx_real the ring holds
            node.set_node_state(s)

    clean, st0, _ = _rollout(ids, T)
    dirty, st1, _ = _rollout(ids, T, poison=poison)
    others = [b for b in range(17) if b not in (5, 9)]
    assert (st0 == 0).all() and np.isfinite(clean).all()
    assert _same(clean[:, others], dirty[:, others]) and (st1[:, others] == 0).all()
    assert (st1[LEAD + 4:, 5] == 3).all() and (st1[:LEAD + 4, 5] == 0).all()
    assert _same(clean[:LEAD + 27, 9], dirty[:LEAD + 27, 9]) and (st1[LEAD + 27:LEAD + 29, 9] == 3).all()
    assert np.isnan(dirty[LEAD + 27, 9, 15:27]).any() and np.isfinite(dirty[LEAD + 27, 9, :15]).all()


def test_form_and_shape_invariance():
    """Both row-store forms give the same rows and records at every batch size,
    and a robot's rows depend neither on the batch size nor on its place."""
    T = LEAD + 34
    full, st, recs = _rollout(IDS, T, form=0)
    assert (st == 0).all()
    for B, ids in ((131, IDS), (1, np.array([100])), (17, np.arange(76, 59, -1)), (67, np.arange(64, 131))):
        assert B in BATCHES and len(ids) == B
        for form in (0, 1):
            if B == 131 and form == 0:
                continue
            rows, st_b, recs_b = _rollout(ids, T, form=form)
            assert _same(rows, full[:, ids]), (B, form)
            assert (st_b == 0).all()
            for a, b in zip(recs_b, recs):
                assert _same(a, b[ids]), (B, form)


def test_state_round_trip():
    """get_state / set_state of all three records at a mid-step tick, then 8
    more ticks: the uninterrupted run's bits."""
    ids = np.arange(17)
    T = LEAD + 45
    whole, _, recs_whole = _rollout(ids, T + 8)
    _, _, recs = _rollout(ids, T)
    assert (recs[2][:, 154 + 99] != 2).any()                        # some robot is in single support
    tail, _, recs_tail = _rollout(ids, 8, states=recs, first_tick=T)
    assert _same(tail, whole[T:])
    for a, b in zip(recs_tail, recs_whole):
        assert _same(a, b)


def test_over_time_row_on_the_device():
    """A node record with advanced counters reaches _walkdtime_max on its next
    tick: mpc_stop = 2, right_support = 2, then the row is re-emitted."""
    ids = np.arange(17)
    node = _node(ids)
    chk = Checker(node)
    s = node.get_node_state()
    s[:, 0], s[:, 1] = 40 + 671, 1.0
    s[:, 154 + 99] = 1.0
    node.set_node_state(s)
    for st in chk.st:
        st.count, st.latch = 40 + 671, True
        st.row[99] = 1.0
    for n in range(3):
        msg = _msg(ids, n, 1.0)
        got = _read(node, node.tick(_t(msg)))
        chk.tick(msg, got, ("over time", n))
        assert (got["row"][:, 97] == 2).all() and (got["row"][:, 99] == 2).all()
        assert (got["sched"][:, 0] == (N.OVER_TIME if n == 0 else N.STOPPED)).all()


def test_chaining_with_no_host_step():
    """After the squat the device gait_msg goes straight into the rt node and
    the servo tick: their outputs are those of the restated row.  Then a fresh
    planner node and a fresh rt node close the loop on the device: the rt
    node's /rt2nrt/state buffer is the planner node's input, whose msg[0] > 0
    starts it."""
    ids = np.arange(17)
    B = 17
    node = _node(ids)
    chk = Checker(node)
    for n in range(LEAD + 3):
        msg = _msg(ids, n, 0.0 if n == 0 else 1.0)
        out = node.tick(_t(msg))
        chk.tick(msg, _read(node, out), ("chain", n))
    restated = _t(chk.rows)
    assert (chk.rows[:, 99] == 2).all() and (out.sched[:, 0] == N.WALKING).all()
    ctrl = np.zeros((B, 25))
    ctrl[:, 0] = 1.0
    ctrl[:, 19:25] = [0.0, HW, 0.0, 0.0, -HW, 0.0]
    ctrl = _t(ctrl)
    rt_a, rt_b = rt.RtNodeBatch(B, _dev()), rt.RtNodeBatch(B, _dev())
    for k in range(3):
        a = [x.clone() for x in rt_a.tick(out.gait_msg, ctrl)]
        b = [x.clone() for x in rt_b.tick(restated, ctrl)]
        for x, y in zip(a, b):
            assert _same(x.cpu().numpy(), y.cpu().numpy()), ("rt", k)
    assert (a[1][:, 0] > 0).all()
    inp = go1servo.synth_inputs(G.SEED, B, G.TICKS)
    sv_a = go1servo.Go1ServoTick(B, _dev(), **G.TEST_PARAMS)
    sv_b = go1servo.Go1ServoTick(B, _dev(), **G.TEST_PARAMS)
    mode, yoff = _t(inp["gait_mode"]), _t(inp["y_offset"])
    for t in range(12):                                             # through the stand-up into the gait branch
        ra = sv_a.step(_t(inp["q_mea"][t]), _t(inp["quat"][t]), out.gait_msg, mode, yoff)
        rb = sv_b.step(_t(inp["q_mea"][t]), _t(inp["quat"][t]), restated, mode, yoff)
        for k in ("q_cmd", "ctrl_msg", "tau", "grf_opt"):
            assert _same(getattr(ra, k).cpu().numpy(), getattr(rb, k).cpu().numpy()), ("servo", t, k)
    assert not ra.homing
    # one closed planner -> rt -> planner iteration after the other, device buffers only
    node2, rt2 = _node(ids), rt.RtNodeBatch(B, _dev())
    chk2 = Checker(node2)
    nrt = rt2.nrt
    branches = []
    for n in range(5):
        msg = nrt.cpu().numpy().copy()
        out2 = node2.tick(nrt)
        chk2.tick(msg, _read(node2, out2), ("loop", n))
        branches.append(int(out2.sched[0, 0]))
        _, nrt, _, _ = rt2.tick(out2.gait_msg, ctrl)
    assert branches == [N.NOT_STARTED, N.NOT_STARTED, N.SQUAT, N.SQUAT, N.SQUAT]
    assert int(node2.get_node_state()[0, 0]) == 3


def test_stream_order():
    """Two ticks issued back to back on a side stream, nothing between them,
    against two synchronised ticks."""
    ids = np.arange(17)
    T = LEAD + 30
    _, _, recs = _rollout(ids, T)
    m0, m1 = _t(_msg(ids, T, 1.0)), _t(_msg(ids, T + 1, 1.0))

    def fresh():
        nd = _node(ids)
        nd.set_state(_t(recs[0]))
        nd.set_tick_state(_t(recs[1]))
        nd.set_node_state(_t(recs[2]))
        torch.cuda.synchronize()
        return nd

    a = fresh()
    ra0 = a.tick(m0).gait_msg.clone()
    torch.cuda.synchronize()
    ra1 = a.tick(m1).gait_msg.clone()
    torch.cuda.synchronize()
    b = fresh()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        o0, o1 = b.tick(m0, stream=side.cuda_stream), None
        o1 = b.tick(m1, stream=side.cuda_stream)
    side.synchronize()
    assert not _same(ra0.cpu().numpy(), ra1.cpu().numpy())
    assert _same(o0.gait_msg.cpu().numpy(), ra0.cpu().numpy()) and _same(o1.gait_msg.cpu().numpy(), ra1.cpu().numpy())
    for x, y in ((a.get_state(), b.get_state()), (a.get_tick_state(), b.get_tick_state()),
                 (a.get_node_state(), b.get_node_state())):
        assert _same(x.cpu().numpy(), y.cpu().numpy())


def test_cpp_shim_matches_python_path():
    """qloco::NLPRTControlBatch for B = 1 through one not-started tick, the
    squat and 12 walking ticks on stepped ground: every row is the Python
    path's bits."""
    ticks, sh = LEAD + 12, 0.02
    ids = [7]
    msgs = [_msg(ids, n, 0.0 if n == 0 else 1.0)[0] for n in range(ticks)]
    r = host_exe.run("test_nlp_node_host", [ticks, repr(sh)], input="\n".join(
        " ".join(repr(float(x)) for x in m) for m in msgs))
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("T ")]
    assert len(rows) == ticks
    node = nlp.PlannerNode(1, _dev(), steplength=0.075, stepwidth=2 * HW, stepheight=sh)
    for n in range(ticks):
        o = node.tick(_t(msgs[n][None, :]))
        torch.cuda.synchronize()
        got = np.array([float.fromhex(x) for x in rows[n][1:101]])
        assert _same(got, o.gait_msg.cpu().numpy()[0]), n
