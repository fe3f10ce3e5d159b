"""GPU tests of the per-robot bodies of the Go1 force QP, the servo force block
and the servo tick (qloco_force_qp_solve_body, qloco_servo_force_block_body,
qloco_go1_servo_tick_body; include/qloco.h sections 3, 7, 16).

The QP runs the eight-body mix of tests/force_body_cases.py: force_cases' 64
robots on `baseline`, `heavy` and `lateral`, member state carried, at both
group widths, grouped and not.  Device against device everything is compared
byte for byte; against the restatement (qo_force_opt per robot with the
robot's own parameters) the bounds are those of tests/test_qp_gpu.py's
test_force_qp_family_parity and tests/test_servo_gpu.py, unchanged: F_leg_guess,
F_leg_ref, qp_solution, status and iterations equal, grf_opt within 1e-9
relative / 1e-8 N and bit-identical on >= 90 % of the solved robots.  The mix
run of a (family, launch) is computed once and shared.
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import force_body_cases as BC  # noqa: E402
import force_cases as FC  # noqa: E402
import host_exe  # noqa: E402

from quadrupedal_loco_amd import build, go1servo, qp  # noqa: E402
from quadrupedal_loco_amd._lib import lib  # noqa: E402
from quadrupedal_loco_amd.go1servo import STATE_FIELDS as F  # noqa: E402

OUT = BC.KEYS                                         # outputs; F_leg_ref and grf_opt are the state arrays
LAUNCHES = [(False, 8), (True, 8), (False, 16), (True, 16)]  # (grouped, group width)
B = BC.BATCH


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


class _group_width:
    def __init__(self, gw):
        self.gw = gw

    def __enter__(self):
        self.prev = lib().qloco_force_set_group_width(self.gw)
        assert self.prev in (8, 16)

    def __exit__(self, *exc):
        lib().qloco_force_set_group_width(self.prev)


def _step(solver, d, body=None):
    """One ForceQP.step: the outputs and, grouped, the carried iteration counts, as numpy."""
    out = solver.step(**{k: _t(v) for k, v in d.items()}, body=body)
    torch.cuda.synchronize()
    g = {k: out[k].cpu().numpy().copy() for k in OUT}
    if solver.order_ws is not None:
        g["prev_it"] = solver.order_ws[:solver.batch].cpu().numpy().copy()
    return g


def _same(a, b, rows_a, rows_b, what):
    for k in a:
        assert a[k][rows_a].tobytes() == b[k][rows_b].tobytes(), (what, k)


@functools.lru_cache(maxsize=None)
def _mix_run(name, grouped, gw, ticks=None):
    """The mix through qp.ForceQP.step(body=): a list of per-tick outputs (read-only)."""
    tk = FC.ticks_of(name, ticks=ticks)
    rows = _t(BC.rows_of(BC.bodies()))
    solver = qp.ForceQP(batch=B, device=_dev(), grouped=grouped)
    with _group_width(gw):
        return [_step(solver, d, rows) for d, _ in tk]


# ---- rows that hold the params' values are the call without rows ----------------------------

@pytest.mark.parametrize("hw", [False, True])
@pytest.mark.parametrize("grouped,gw", LAUNCHES)
def test_qp_rows_holding_the_params_equal_no_rows(hw, grouped, gw):
    dev = _dev()
    a = qp.ForceQP(batch=B, device=dev, grouped=grouped, hw=hw)
    b = qp.ForceQP(batch=B, device=dev, grouped=grouped, hw=hw)
    rows = qp.force_body_rows(B, params=b.params)
    assert rows[0, 0] == (14.0 if hw else 12.0) and rows[0, 5] == (0.5 if hw else 0.25)
    # with rows prm is only the stand-in of refused robots: garbage there must not matter
    b.params.alpha, b.params.mu, b.params.fz_max = 1.0, 9.0, 1.0
    with _group_width(gw):
        for t, (d, _) in enumerate(FC.ticks_of("hw_lateral" if hw else "lateral")):
            _same(_step(a, d), _step(b, d, _t(rows)), slice(None), slice(None), (hw, grouped, gw, t))


def test_block_and_tick_rows_holding_the_defaults_equal_no_rows():
    dev = _dev()
    n = 32
    a, b = qp.ServoForceBlock(n, dev), qp.ServoForceBlock(n, dev)
    rows = _t(qp.force_body_rows(n))
    for t in range(3):
        d = {k: _t(v) for k, v in qp.synth_servo_inputs(7, n, t).items()}
        oa, ob = a.step(**d), b.step(**d, body=rows)
        torch.cuda.synchronize()
        for k in oa:
            assert torch.equal(oa[k], ob[k]), (t, k)
        assert torch.equal(a.ws, b.ws), t              # every member, the grouping state included
    n, T = 16, 7
    inp = go1servo.synth_inputs(11, n, T)
    ta = go1servo.Go1ServoTick(n, dev, gait_data=True, **TICK_PARAMS)
    tb = go1servo.Go1ServoTick(n, dev, gait_data=True, **TICK_PARAMS)
    rows = _t(qp.force_body_rows(n))
    for t in range(T):
        args = (_t(inp["q_mea"][t]), _t(inp["quat"][t]), _t(inp["gait_msg"][t]), _t(inp["gait_mode"]), _t(inp["y_offset"]))
        ra, rb = ta.step(*args), tb.step(*args, body=rows)
        torch.cuda.synchronize()
        assert ra.homing == (t < TICK_HOM)
        for k, v in ta.out.items():
            assert torch.equal(v, tb.out[k]), (t, k)
        assert torch.equal(ta.get_state(), tb.get_state()), t


# ---- the mix against one uniform no-rows call per body --------------------------------------

@pytest.mark.parametrize("grouped,gw", LAUNCHES)
@pytest.mark.parametrize("name", BC.FAMILIES)
def test_qp_mix_equals_one_uniform_call_per_body(name, grouped, gw):
    dev = _dev()
    tk = FC.ticks_of(name)
    idx = BC.bodies()
    mix = _mix_run(name, grouped, gw)
    changed = 0
    with _group_width(gw):
        for k in range(len(BC.MIX)):
            uni = qp.ForceQP(batch=B, device=dev, grouped=grouped, **BC.overrides(k))
            mine = np.flatnonzero(idx == k)
            for t, (d, _) in enumerate(tk):
                g = _step(uni, d)
                _same(mix[t], g, mine, mine, (name, grouped, gw, "body", k, "tick", t))
                if k == 0:
                    others = np.flatnonzero(idx != 0)
                    changed += int(np.sum(np.any(mix[t]["grf_opt"][others] != g["grf_opt"][others], axis=1)))
    assert changed >= len(tk) * 28, changed            # the rows are read: most other bodies differ from the default


@pytest.mark.parametrize("grouped,gw", LAUNCHES)
@pytest.mark.parametrize("name", BC.FAMILIES)
def test_qp_mix_parity_with_the_restatement(name, grouped, gw):
    """The bounds of test_force_qp_family_parity (tests/test_qp_gpu.py)."""
    _, _, _, run = BC.mix(name)
    mix = _mix_run(name, grouped, gw)
    exact = solved = 0
    for t, (g, r) in enumerate(zip(mix, run.ticks)):
        what = (name, grouped, gw, t)
        for k in ("F_leg_guess", "F_leg_ref"):
            assert np.array_equal(g[k], r[k], equal_nan=True), (what, k)
        for k in ("qp_solution", "status", "iters"):
            assert np.array_equal(g[k], r[k]), (what, k, g[k], r[k])
        err = np.abs(g["grf_opt"] - r["grf_opt"]).max()
        print("%s tick %d: max |grf_opt - restatement| = %.3g N" % (what, t, err))
        assert np.allclose(g["grf_opt"], r["grf_opt"], rtol=1e-9, atol=1e-8), what
        ok = (r["status"] == FC.OK) & (r["qp_solution"] == 1)
        exact += int(np.sum(np.all(g["grf_opt"][ok] == r["grf_opt"][ok], axis=1)))
        solved += int(ok.sum())
        if grouped:
            assert np.array_equal(g["prev_it"], r["iters"]), what
    print("%s grouped=%s gw=%d: grf_opt bit-identical on %d of %d solved" % (name, grouped, gw, exact, solved))
    assert solved >= 64 and exact >= 0.9 * solved, (name, exact, solved)


@pytest.mark.parametrize("grouped,gw", LAUNCHES)
def test_qp_mix_permuted_keeps_every_robots_bytes(grouped, gw):
    dev = _dev()
    p = BC.derangement()
    new_pos = np.argsort(p)
    w = 64 // gw                                       # robots per block
    assert np.all(new_pos % w != np.arange(B) % w)     # no robot keeps its group slot
    blocks = {frozenset(range(w * k, w * k + w)) for k in range(B // w)}
    assert all(frozenset(p[w * k:w * k + w].tolist()) not in blocks for k in range(B // w))
    name = "lateral"
    mix = _mix_run(name, grouped, gw)
    rows = _t(BC.rows_of(BC.bodies())[p])
    solver = qp.ForceQP(batch=B, device=dev, grouped=grouped)
    with _group_width(gw):
        for t, (d, _) in enumerate(FC.ticks_of(name)):
            g = _step(solver, {k: v[p] for k, v in d.items()}, rows)
            _same(g, mix[t], slice(None), p, (grouped, gw, t))


@pytest.mark.parametrize("n", [1, 3, 7, 9, 17])
def test_qp_tails_and_padded_buffers(n):
    """The first n robots of the mix alone: outputs as in the full batch; rows
    n .. n + 5 of every buffer (the body rows and the grouping workspace
    included) keep their sentinel."""
    dev = _dev()
    name, pad = "heavy", 5
    tk = FC.ticks_of(name)
    rows_np = np.full((n + pad, 16), np.nan)           # NaN rows past n: never read, nothing refused
    rows_np[:n] = BC.rows_of(BC.bodies())[:n]
    rows = _t(rows_np)
    for grouped, gw in LAUNCHES:
        mix = _mix_run(name, grouped, gw)
        solver = qp.ForceQP(batch=n, device=dev, grouped=grouped)
        f64 = lambda: torch.full((n + pad, 12), -777.25, dtype=torch.float64, device=dev)
        i32 = lambda: torch.full((n + pad,), -777, dtype=torch.int32, device=dev)
        solver.F_leg_ref, solver.grf_opt, solver.F_leg_guess = f64(), f64(), f64()
        solver.F_leg_ref[:n] = 0.0
        solver.grf_opt[:n] = 0.0
        solver.qp_solution, solver.status, solver.iters = i32(), i32(), i32()
        if grouped:
            ws = torch.full((2 * n + 160 + pad,), -777, dtype=torch.int32, device=dev)
            ws[:2 * n + 160] = 0
            solver.order_ws = ws
        with _group_width(gw):
            for t, (d, _) in enumerate(tk):
                out = solver.step(**{k: _t(np.concatenate([v[:n], v[:pad]])) for k, v in d.items()}, body=rows[:n])
                torch.cuda.synchronize()
                for k in OUT:
                    got = out[k].cpu().numpy()
                    assert got[:n].tobytes() == mix[t][k][:n].tobytes(), (n, grouped, gw, t, k)
                    assert np.all(got[n:] == (-777.25 if got.dtype == np.float64 else -777)), (n, grouped, gw, t, k)
                if grouped:
                    assert torch.all(solver.order_ws[2 * n + 160:] == -777)
                    assert np.array_equal(solver.order_ws[:n].cpu().numpy(), mix[t]["iters"][:n])
        assert torch.equal(rows.isnan(), _t(np.isnan(rows_np)))


# ---- refused rows ---------------------------------------------------------------------------

@pytest.mark.parametrize("grouped,gw", LAUNCHES)
def test_qp_refused_rows(grouped, gw):
    """NaN mass, mass 0, negative mu, +Inf fz_max and negative alpha scattered
    into the mix at tick 1 of 3: those robots are refused as include/qloco.h
    section 3 says, their members unchanged bit for bit; everyone else equals
    the run without them byte for byte; with the rows corrected at tick 2 they
    solve again, from where they stood (the restatement skipping tick 1 for
    them, the existing bounds)."""
    dev = _dev()
    name = "lateral"
    tk = FC.ticks_of(name, ticks=3)
    clean = _mix_run(name, grouped, gw, ticks=3)
    good = BC.rows_of(BC.bodies())
    bad = good.copy()
    at = np.array(BC.REFUSED_AT)
    for b, (field, v) in zip(at, BC.REFUSED):
        bad[b, qp.FORCE_BODY_COLUMNS[field][0]] = v
    refused = np.zeros(B, bool)
    refused[at] = True
    others = np.flatnonzero(~refused)
    solver = qp.ForceQP(batch=B, device=dev, grouped=grouped)
    orc = BC.PerRobotOracle(good)
    with _group_width(gw):
        g0 = _step(solver, tk[0][0], _t(good))
        orc.step(tk[0][0])
        _same(g0, clean[0], slice(None), slice(None), "tick 0")
        assert np.all(np.abs(g0["grf_opt"][at]).max(axis=1) > 1.0)   # "unchanged" is a non-zero vector
        g1 = _step(solver, tk[1][0], _t(bad))
        orc.step(tk[1][0], skip=refused)
        _same(g1, clean[1], others, others, "tick 1, everyone else")
        assert np.all(g1["status"][at] == BC.ERR_ARG) and np.all(g1["qp_solution"][at] == 0)
        assert np.all(g1["iters"][at] == 0) and np.all(np.isnan(g1["F_leg_guess"][at]))
        for k in ("F_leg_ref", "grf_opt") + (("prev_it",) if grouped else ()):
            assert g1[k][at].tobytes() == g0[k][at].tobytes(), k
            assert np.all(np.isfinite(g1[k])), k       # nothing non-finite in the resident state
        g2 = _step(solver, tk[2][0], _t(good))
        r2 = orc.step(tk[2][0])
        orc.close()
    _same(g2, clean[2], others, others, "tick 2, everyone else")
    assert np.all(g2["status"][at] == FC.OK) and np.all(g2["qp_solution"][at] == 1) and np.all(g2["iters"][at] > 0)
    for k in ("F_leg_guess", "F_leg_ref"):
        assert np.array_equal(g2[k], r2[k]), k
    for k in ("qp_solution", "status", "iters"):
        assert np.array_equal(g2[k], r2[k]), k
    assert np.allclose(g2["grf_opt"], r2["grf_opt"], rtol=1e-9, atol=1e-8)
    assert np.any(g2["grf_opt"][at] != clean[2]["grf_opt"][at])     # they did skip a tick


# ---- HIP graph -------------------------------------------------------------------------------

def test_qp_body_call_replays_from_a_hip_graph():
    """qloco_force_qp_solve_body (memset + count + scatter + the rows kernel on
    one stream: a linear chain) captured once after one eager call and replayed
    over three ticks of new inputs equals the eager call bit for bit, member
    and grouping state carried by both."""
    dev = _dev()
    tk = FC.ticks_of("lateral", ticks=3)
    ins = [{k: _t(v) for k, v in d.items()} for d, _ in tk]
    static = {k: v.clone() for k, v in ins[0].items()}
    rows = _t(BC.rows_of(BC.bodies()))
    eager = qp.ForceQP(batch=B, device=dev)
    graphed = qp.ForceQP(batch=B, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):                         # the eager call: constants uploaded
        qp.ForceQP(batch=B, device=dev).step(**static, body=rows)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        og = graphed.step(**static, body=rows)
    for t in range(3):
        for k, v in ins[t].items():
            static[k].copy_(v)
        g.replay()
        oe = eager.step(**ins[t], body=rows)
        torch.cuda.synchronize()
        for k in OUT:
            assert torch.equal(og[k], oe[k]), (t, k)
        assert torch.equal(graphed.order_ws[:B], eager.order_ws[:B]), t
        assert np.array_equal(og["grf_opt"].cpu().numpy(), _mix_run("lateral", True, 8, ticks=3)[t]["grf_opt"])


# ---- the force block -------------------------------------------------------------------------

def _oracle_parity(orc, d, g, what, skip=None):
    """grf_opt of the block / the tick against qo_force_opt fed the device's
    F_sum / Force_L_R and the row's parameters: the bounds of
    tests/test_servo_gpu.py.  Returns (bit-identical, compared) robots."""
    r = orc.step(BC.block_as_force_inputs(d, g["F_sum"], g["Force_L_R"]), skip=skip)
    sel = np.ones(len(g["status"]), bool) if skip is None else ~skip
    assert np.array_equal(g["status"][sel], r["status"][sel]), what
    assert np.array_equal(g["qp_solution"][sel], r["qp_solution"][sel]), what
    assert np.allclose(g["grf_opt"][sel], r["grf_opt"][sel], rtol=1e-9, atol=1e-8), what
    return int(np.sum(np.all(g["grf_opt"][sel] == r["grf_opt"][sel], axis=1))), int(sel.sum())


def test_force_block_rows():
    dev = _dev()
    n, T = 32, 3
    rows = BC.servo_rows(n)
    body = np.arange(n) % 8
    blk = qp.ServoForceBlock(n, dev)
    plain = qp.ServoForceBlock(n, dev)
    uni = [qp.ServoForceBlock(n, dev) for _ in range(8)]
    uni_rows = [_t(np.tile(rows[k], (n, 1))) for k in range(8)]
    orc = BC.PerRobotOracle(rows)
    exact = total = differ = 0
    for t in range(T):
        d = qp.synth_servo_inputs(7, n, t)
        dd = {k: _t(v) for k, v in d.items()}
        g = {k: v.cpu().numpy().copy() for k, v in blk.step(**dd, body=_t(rows)).items()}
        p = {k: v.cpu().numpy().copy() for k, v in plain.step(**dd).items()}
        fs = BC.f_sum_numpy(rows, d["coma_des"])
        assert g["F_sum"].tobytes() == fs.tobytes(), t
        flr = BC.force_lr_numpy(fs, d["com_des"], d["rfoot_des"], d["lfoot_des"], d["right_support"])
        assert g["Force_L_R"].tobytes() == flr.tobytes(), t
        for k in range(8):
            u = {key: v.cpu().numpy() for key, v in uni[k].step(**dd, body=uni_rows[k]).items()}
            mine = np.flatnonzero(body == k)
            for key in g:
                assert g[key][mine].tobytes() == u[key][mine].tobytes(), (t, k, key)
        zero = np.flatnonzero(body == 0)                # 12 and Momentum_sum: the call without rows
        for key in g:
            assert g[key][zero].tobytes() == p[key][zero].tobytes(), (t, key)
        differ += int(np.sum(np.any(g["grf_opt"][body != 0] != p["grf_opt"][body != 0], axis=1)))
        assert np.all(g["status"] == FC.OK) and np.all(np.isfinite(g["tau"]))
        e, c = _oracle_parity(orc, d, g, t)
        exact, total = exact + e, total + c
    orc.close()
    assert differ >= T * 20, differ
    assert exact >= 0.9 * total, (exact, total)


def test_force_block_refused_row():
    dev = _dev()
    n = 32
    rows = BC.servo_rows(n)
    bad = rows.copy()
    bad[9, 0] = np.nan
    bad[17, 5] = -0.1
    at = [9, 17]
    others = np.setdiff1d(np.arange(n), at)
    a, b = qp.ServoForceBlock(n, dev), qp.ServoForceBlock(n, dev)
    for t in range(3):
        dd = {k: _t(v) for k, v in qp.synth_servo_inputs(7, n, t).items()}
        ga = {k: v.cpu().numpy().copy() for k, v in a.step(**dd, body=_t(rows)).items()}
        before = b.ws.clone()
        gb = {k: v.cpu().numpy().copy() for k, v in b.step(**dd, body=_t(bad if t == 1 else rows)).items()}
        for k in ga:
            assert ga[k][others].tobytes() == gb[k][others].tobytes(), (t, k)
        if t == 1:
            assert np.all(gb["status"][at] == BC.ERR_ARG) and np.all(gb["qp_solution"][at] == 0)
            assert np.all(np.isnan(gb["tau"][at])) and np.all(np.isnan(gb["grf_opt"][at]))
            # the workspace copies of F_leg_ref and grf_opt (its first two arrays) did not move
            al = lambda x: (x + 255) & ~255
            for off in (0, al(8 * 12 * n)):
                now = b.ws[off:off + 96 * n].view(torch.float64).view(n, 12)
                was = before[off:off + 96 * n].view(torch.float64).view(n, 12)
                assert torch.equal(now[at], was[at]) and bool(torch.all(now[at].abs().max(dim=1).values > 1.0))
            # nothing non-finite in the workspace's members: its doubles are six arrays of 12 per
            # robot (F_leg_ref, grf_opt, F_leg_guess, then the relative feet) and two of 6; the third
            # is the QP's F_leg_guess output (NaN for a refused robot, rewritten by every call)
            w12, w6 = al(8 * 12 * n), al(8 * 6 * n)
            dbl = b.ws[:6 * w12 + 2 * w6].view(torch.float64)
            keep = torch.ones_like(dbl, dtype=torch.bool)
            keep[2 * w12 // 8:3 * w12 // 8] = False
            assert bool(torch.isfinite(dbl[keep]).all())
            assert bool(dbl[2 * w12 // 8:3 * w12 // 8].view(-1, 12)[at].isnan().all())
        if t == 2:
            assert np.all(gb["status"][at] == FC.OK) and np.all(np.isfinite(gb["tau"][at])) and np.all(np.isfinite(gb["grf_opt"][at]))


# ---- the servo tick --------------------------------------------------------------------------

TICK_PARAMS = dict(stand_duration=0.0025, t_walk_start=0.01)   # ticks 0..2 stand up, the targets move from count 2
TICK_HOM = 3
TICK_KEYS = ("q_cmd", "ctrl_msg", "tau", "grf_opt", "F_sum", "Force_L_R", "swing", "qp_solution", "status")


def _tick(tk, inp, t, body=None):
    r = tk.step(_t(inp["q_mea"][t]), _t(inp["quat"][t]), _t(inp["gait_msg"][t]), _t(inp["gait_mode"]),
                _t(inp["y_offset"]), body=body)
    torch.cuda.synchronize()
    g = {k: getattr(r, k).cpu().numpy().copy() for k in TICK_KEYS + ("coma_des", "com_des", "rfoot_des", "lfoot_des",
                                                                      "body_p_des", "foot_des")}
    g["state"] = tk.get_state().cpu().numpy()
    return g


def test_servo_tick_rows():
    """B = 16, three stand-up ticks and four of the gait branch.  Standing up
    the rows are not read (even rows the rule refuses change nothing).  Then
    F_sum and Force_L_R are the numpy evaluation of include/qloco.h section 7
    on the tick's own filtered references, every robot equals the tick whose
    rows are all its row, grf_opt matches qo_force_opt with the row's
    parameters; on the last tick a refused row leaves that robot's member state
    finite and unmoved and its tau / grf_opt NaN."""
    dev = _dev()
    n, T = 16, 7
    inp = go1servo.synth_inputs(11, n, T)
    rows = BC.servo_rows(n)
    body = np.arange(n) % 8
    junk = rows.copy()
    junk[5, 0] = np.nan
    junk[6, 5] = -1.0
    bad = rows.copy()
    bad[5, 5] = -0.1
    tk = go1servo.Go1ServoTick(n, dev, **TICK_PARAMS)
    plain = go1servo.Go1ServoTick(n, dev, **TICK_PARAMS)
    uni = [go1servo.Go1ServoTick(n, dev, **TICK_PARAMS) for _ in range(8)]
    uni_rows = [_t(np.tile(rows[k], (n, 1))) for k in range(8)]
    orc = BC.PerRobotOracle(rows)
    exact = total = differ = 0
    for t in range(T):
        last = t == T - 1
        before = tk.get_state().cpu().numpy()
        g = _tick(tk, inp, t, _t(junk if t < TICK_HOM else bad if last else rows))
        p = _tick(plain, inp, t)
        us = [_tick(uni[k], inp, t, uni_rows[k]) for k in range(8)]
        if t < TICK_HOM:                                # standing up: no QP, no row read, nothing refused
            for k in g:
                assert g[k].tobytes() == p[k].tobytes(), (t, k)
            continue
        skip = np.zeros(n, bool)
        skip[5] = last
        sel = np.flatnonzero(~skip)
        fs = BC.f_sum_numpy(rows, g["coma_des"])
        assert g["F_sum"][sel].tobytes() == fs[sel].tobytes(), t
        rs = inp["gait_msg"][t][:, 99].astype(np.int32)
        flr = BC.force_lr_numpy(fs, g["com_des"], g["rfoot_des"], g["lfoot_des"], rs)
        assert g["Force_L_R"][sel].tobytes() == flr[sel].tobytes(), t
        for k in range(8):
            mine = np.flatnonzero((body == k) & ~skip)
            for key in g:
                assert g[key][mine].tobytes() == us[k][key][mine].tobytes(), (t, k, key)
        zero = np.flatnonzero(body == 0)
        for key in g:
            assert g[key][zero].tobytes() == p[key][zero].tobytes(), (t, key)
        differ += int(np.sum(np.any(g["grf_opt"][sel][body[sel] != 0] != p["grf_opt"][sel][body[sel] != 0], axis=1)))
        d = dict(body_p_des=g["body_p_des"], foot_des=g["foot_des"], rfoot_des=g["rfoot_des"], lfoot_des=g["lfoot_des"],
                 gait_mode=inp["gait_mode"], right_support=rs, y_offset=inp["y_offset"])
        e, c = _oracle_parity(orc, d, g, t, skip=skip if last else None)
        exact, total = exact + e, total + c
        assert np.all(g["status"][sel] == FC.OK), t
        if last:
            assert g["status"][5] == BC.ERR_ARG and g["qp_solution"][5] == 0
            assert np.all(np.isnan(g["tau"][5])) and np.all(np.isnan(g["grf_opt"][5]))
            assert np.all(np.isfinite(g["state"]))      # the refused robot's member state included
            for key in ("F_leg_ref", "grf_opt"):
                sl = slice(*F[key])
                assert g["state"][5, sl].tobytes() == before[5, sl].tobytes(), key
            assert np.abs(before[5, slice(*F["grf_opt"])]).max() > 1.0   # (mode 103 keeps F_leg_ref at 0)
            assert g["q_cmd"][5].tobytes() == us[5]["q_cmd"][5].tobytes()   # the rest of its tick ran
    orc.close()
    assert differ >= (T - TICK_HOM) * 10, differ
    assert exact >= 0.9 * total, (exact, total)


# ---- the C++ classes -------------------------------------------------------------------------

def test_cpp_set_bodies():
    """tests/cpp/test_force_body_host.cpp: set_bodies of Dynamiccclass,
    ServoForceBlock and Go1ServoBatch, and nullptr back to the params."""
    _dev()
    assert os.path.exists(build.build_host_exe("test_force_body_host"))
    host_exe.run("test_force_body_host")
