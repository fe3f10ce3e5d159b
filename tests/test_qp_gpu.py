"""GPU parity tests for the small-QP paths (EiQuadProg / force QP / body MPC).

Checker: the oracle's double-precision restatement (oracle/eiquadprog.c,
force_qp.c, body_mpc.c).  The GPU kernels run the same fp64 operation
sequence (no FMA contraction, one lane per dot product in index order), so
the stated tolerance is tight: status and iteration count equal, results
within 1e-9 relative (bit-identical in the common case -- the fraction is
asserted >= 90 %); schedule integers (Indexfind, bjx1/bjx2/t_yu) bit-exact.

The Goldfarb-Idnani kernels (gi_kernel: n, p <= 16, m <= 64, four QPs per
wave; gi_wide_kernel above that) are tested on the input families of
tests/qp_cases.py; tests/test_oracle.py asserts each family's preconditions
on the restatement alone, 64 instances per shape (branch counts from an
instrumented scratch copy of the restatement, not in the repository):

  A  feasible Gaussian (8,0,48) (12,3,24) (16,4,64, 2 zero CE) (16,0,64):
     64 / 64 / 63 / 64 OK (one INFEASIBLE), mean iterations 11.0 / 8.0 /
     15.4 / 17.2, 35-174 partial steps per shape; no h == 0, no ties.
  B  box, n = 1, 4, 16 | 17, 32, 64: 64/64 OK; h == 0 skips in the
     add-constraint sweep 0 / 66 / 3,059 | 3,246 / 13,074 / 57,289;
     restatement against clip(-g0 / diag G, lo, hi): 8.9e-16 / 2.7e-15 /
     3.1e-15 | 1.8e-15 / 2.2e-15 / 2.8e-15; the kernels are held to 16 x
     the restatement's error on the same inputs, computed in the test.
  C  coupled ties (4,8) (8,24) (16,64) | (17,65) (32,96): 64/64 OK; an exact
     tie in the most-violated scan on 14 / 19 / 38 | 32 / 58 instances; a
     restatement whose scan keeps the LAST tied index changes the status or
     iteration count on 3 / 7 / 13 | 19 / 33 of them, so the iteration
     equality exposes a wrong tie rule; 2-6,431 h == 0 skips.  The solutions
     are not dyadic (x has > 20 fractional bits on 318 of 320 instances), so
     there is no exactness to use: parity only.
  D  mixed statuses in one wave (8,0,24), B = 67: NOT_PD 17, INFEASIBLE 17,
     OK 33 (17 with an active set, 16 slack with one iteration).
  E  equality only (16,16,0) (4,2,0) | (20,17,0): 64/64 OK, one iteration;
     restatement against the KKT solution, relative to max(1, |x|max):
     7.9e-14 / 5.1e-16 | 8.2e-15; the kernels are held to 16 x the
     restatement's error on the same inputs, computed in the test.
  more live equality columns than variables (4,6,4) | (20,24,8): DEGENERATE
     with 0 iterations on every instance.

No family reaches the degenerate-restore branch (add_constraint false after
a full step: iaexcl, snapshot restore, goto l2); see DESIGN.md §4f.

The kernels that run the same core inside a larger kernel (force_qp_kernel,
body_mpc_kernel) are tested on the families of tests/force_cases.py and
tests/body_cases.py -- legs at fz_max, active friction rows, failed
factorisations (NOT_PD: grf_opt / _V_ini keep their values), NaN fallbacks,
flags outside the gait table, bounds of the body QP; census in the tests'
docstrings and in DESIGN.md §4.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import body_cases as BC  # noqa: E402
import force_cases as FC  # noqa: E402
import oracle_lib as O  # noqa: E402
import qp_cases as Q  # noqa: E402
from cases import force_inputs  # noqa: E402
from qp_cases import oracle_eqp, random_feasible_qp, random_qp  # noqa: E402

from quadrupedal_loco_amd import qp  # noqa: E402


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("n,p,m,zero_ce", [(4, 0, 8, 0), (8, 0, 48, 0), (12, 12, 24, 6),
                                           (12, 3, 24, 0), (16, 4, 64, 2)])
def test_eiquadprog_matches_restatement(n, p, m, zero_ce):
    """Parity on the INFEASIBLE path, not a solution test: unconstrained
    Gaussian offsets are mostly infeasible at these shapes.  The oracle's
    census over the 64 instances, OK / INFEASIBLE: (4, 0, 8) 51 / 13,
    (8, 0, 48) 0 / 64, (12, 12, 24) 2 / 62, (12, 3, 24) 28 / 36,
    (16, 4, 64) 0 / 64 -- so x and f are compared on few instances or none,
    status and iterations on all.  Solved instances: the family tests below."""
    dev = _dev()
    rng = np.random.default_rng(n * 100 + p * 10 + m)
    B = 64
    probs = [random_qp(rng, n, p, m, zero_ce) for _ in range(B)]
    stack = lambda k: np.stack([np.asfortranarray(pr[k]).ravel(order="F") for pr in probs])
    res = qp.eiquadprog_solve(*(torch.from_numpy(stack(k)).to(dev) for k in range(6)),
                              n=n, p=p, m=m)
    torch.cuda.synchronize()
    x = res["x"].cpu().numpy()
    f = res["f"].cpu().numpy()
    st = res["status"].cpu().numpy()
    it = res["iters"].cpu().numpy()
    exact = 0
    for b in range(B):
        xo, fo, sto, ito = oracle_eqp(*probs[b])
        assert st[b] == sto, (b, st[b], sto)
        assert it[b] == ito, (b, it[b], ito)
        if sto == 0:
            assert np.allclose(x[b], xo, rtol=1e-9, atol=1e-9), (b, x[b], xo)
            assert np.isclose(f[b], fo, rtol=1e-9, atol=1e-9)
            exact += int(np.array_equal(x[b], xo))
    ok = int(np.sum(st == 0))
    assert exact >= 0.9 * ok, (exact, ok)


@pytest.mark.parametrize("n,p,m,zero_ce", [(60, 10, 300, 3), (30, 0, 120, 0), (17, 17, 65, 4),
                                           (64, 64, 320, 8), (40, 6, 200, 0)])
def test_eiquadprog_wide_matches_restatement(n, p, m, zero_ce):
    """The reference's QPBaseClass capacity (nVars <= 60, nIneq <= 300,
    QPBaseClass.h:49-51) through qloco_eiquadprog_solve's size dispatch: one
    QP per wavefront (qloco_gi_wide.hip), zero CE columns included (the
    me = p / A(i) quirks).  Status and active-set iterations equal to the
    restatement; x within 1e-9 relative (the triangular solves are column
    sweeps, so results agree to rounding, not bit for bit), f within 1e-9."""
    dev = _dev()
    rng = np.random.default_rng(n * 1000 + p * 10 + m)
    B = 24
    probs = [random_feasible_qp(rng, n, p, m, zero_ce) for _ in range(B)]
    stack = lambda k: np.stack([np.asfortranarray(pr[k]).ravel(order="F") for pr in probs])
    res = qp.eiquadprog_solve(*(torch.from_numpy(stack(k)).to(dev) for k in range(6)),
                              n=n, p=p, m=m)
    torch.cuda.synchronize()
    x = res["x"].cpu().numpy()
    f = res["f"].cpu().numpy()
    st = res["status"].cpu().numpy()
    it = res["iters"].cpu().numpy()
    solved = 0
    for b in range(B):
        xo, fo, sto, ito = oracle_eqp(*probs[b])
        assert st[b] == sto, (b, st[b], sto)
        assert it[b] == ito, (b, it[b], ito)
        if sto == 0:
            solved += 1
            sc = max(1.0, np.abs(xo).max())
            assert np.abs(x[b] - xo).max() <= 1e-9 * sc, (b, np.abs(x[b] - xo).max())
            assert abs(f[b] - fo) <= 1e-9 * max(1.0, abs(fo)), (b, f[b], fo)
    # p = n with skipped zero CE columns drives EiQuadProg's index quirks into
    # infeasible reports on some instances (the restatement does the same)
    assert solved >= (4 if p >= n else B // 2), solved
    assert np.mean(it) > 2  # the active set did work


@pytest.mark.parametrize("hw,grouped", [(False, False), (True, True), (True, False)])
def test_force_qp_matches_restatement_over_ticks(hw, grouped):
    """force_distribution + force_opt over three ticks of member state against
    the oracle (dynmics_compute.cpp:141-445), bit-exact in >= 90 % of
    instances and within 1e-9 otherwise -- with the sim's constants (mass 12,
    mu 0.25) and with the hardware copy's (unitree_legged_real: mass =
    gait::mass = 14, mu = 0.5, called at torque_mode.cpp:1364-1367), through
    the plain and the grouped launch.  Status, qp_solution and iterations
    equal on every robot and tick.  These inputs (seed 7) all solve OK with
    no leg at fz_max; the other kinds are test_force_qp_family_parity's."""
    dev = _dev()
    rng = np.random.default_rng(7)
    B, ticks = 96, 3
    prm = O.ForceParams()
    O.lib().qo_force_params_default(C.byref(prm))
    if hw:
        prm.mass, prm.mu = 14.0, 0.5
    states = []
    for b in range(B):
        s = O.DynState()
        O.lib().qo_dyn_init(C.byref(s))
        states.append(s)
    solver = qp.ForceQP(batch=B, device=dev, grouped=grouped, hw=hw)
    assert (solver.params.mass, solver.params.mu) == ((14.0, 0.5) if hw else (12.0, 0.25))
    exact, total = 0, 0
    for tick in range(ticks):
        inp = force_inputs(rng, B)
        out = solver.step(**{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
                             for k, v in inp.items()})
        torch.cuda.synchronize()
        g = out["grf_opt"].cpu().numpy()
        guess = out["F_leg_guess"].cpu().numpy()
        qps = out["qp_solution"].cpu().numpy()
        st = out["status"].cpu().numpy()
        its = out["iters"].cpu().numpy()
        for b in range(B):
            d = lambda k, b=b: np.ascontiguousarray(inp[k][b], dtype=np.float64)
            O.lib().qo_force_distribution(C.byref(states[b]), O.P(d("com_des")), O.P(d("leg_des")),
                                          O.P(d("F_force_des")), int(inp["mode"][b]),
                                          float(inp["y_coef"][b]), O.P(d("rfoot_des")),
                                          O.P(d("lfoot_des")))
            fe = inp["feet_p"][b].reshape(4, 3)
            est, eit = C.c_int(0), C.c_int(0)
            ok = O.lib().qo_force_opt(C.byref(states[b]), C.byref(prm), O.P(d("base_p")),
                                      O.P(np.ascontiguousarray(fe[0])), O.P(np.ascontiguousarray(fe[1])),
                                      O.P(np.ascontiguousarray(fe[2])), O.P(np.ascontiguousarray(fe[3])),
                                      O.P(d("FT_total_des")), int(inp["mode"][b]),
                                      int(inp["right_support"][b]), float(inp["y_coef"][b]),
                                      C.byref(est), C.byref(eit))
            ref = np.array(states[b].grf_opt[:])
            assert np.array_equal(guess[b], np.array(states[b].F_leg_guess[:])), b
            assert qps[b] == ok and st[b] == est.value, (b, qps[b], ok, st[b], est.value)
            assert its[b] == eit.value, (tick, b, its[b], eit.value)
            assert np.allclose(g[b], ref, rtol=1e-9, atol=1e-8), (tick, b, g[b], ref)
            exact += int(np.array_equal(g[b], ref))
            total += 1
    assert exact >= 0.9 * total, (exact, total)
    for s in states:
        O.lib().qo_dyn_free(C.byref(s))


@pytest.mark.parametrize("grouped", [True, False])
def test_force_qp_group_width_is_bit_identical(grouped):
    """Eight 8-lane groups per wave (the default) and four 16-lane groups run
    the same per-element operations in the same order (qloco_gi_core.hpp):
    every output equal bit for bit over four ticks, member state carried,
    B = 1001 (a partial last wavefront at both widths)."""
    from quadrupedal_loco_amd._lib import lib
    dev = _dev()
    L = lib()
    rng = np.random.default_rng(12)
    B, ticks = 1001, 4
    a = qp.ForceQP(batch=B, device=dev, grouped=grouped)
    b = qp.ForceQP(batch=B, device=dev, grouped=grouped)
    prev = L.qloco_force_set_group_width(8)
    try:
        for tick in range(ticks):
            inp = force_inputs(rng, B)
            d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items()}
            assert L.qloco_force_set_group_width(8) in (8, 16)
            oa = a.step(**d)
            torch.cuda.synchronize()
            assert L.qloco_force_set_group_width(16) == 8
            ob = b.step(**d)
            torch.cuda.synchronize()
            for k in ("grf_opt", "F_leg_guess", "F_leg_ref", "qp_solution", "status", "iters"):
                assert torch.equal(oa[k], ob[k]), (tick, k)
        assert L.qloco_force_set_group_width(4) == 100  # QLOCO_ERR_ARG, width unchanged
        assert L.qloco_force_set_group_width(16) == 16
    finally:
        L.qloco_force_set_group_width(prev)


def test_force_qp_grouped_launch_replays_from_a_hip_graph():
    """The grouped force-QP call (memset + count + scatter + force kernel,
    INTEGRATION.md §2) allocates nothing and keeps its state in caller
    buffers, so it can be captured once and replayed every servo tick: a
    captured ForceQP.step fed new inputs through static tensors gives the
    eager call's outputs bit for bit over four ticks, member state and
    grouping state carried by both."""
    dev = _dev()
    rng = np.random.default_rng(13)
    B, ticks = 1001, 4
    ticks_in = [{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in force_inputs(rng, B).items()}
                for _ in range(ticks)]
    static = {k: v.clone() for k, v in ticks_in[0].items()}
    eager = qp.ForceQP(batch=B, device=dev)
    graphed = qp.ForceQP(batch=B, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):  # warm-up on a throw-away instance: constants uploaded
        qp.ForceQP(batch=B, device=dev).step(**static)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        og = graphed.step(**static)
    for tick in range(ticks):
        for k, v in ticks_in[tick].items():
            static[k].copy_(v)
        g.replay()
        oe = eager.step(**ticks_in[tick])
        torch.cuda.synchronize()
        for k in ("grf_opt", "F_leg_guess", "F_leg_ref", "qp_solution", "status", "iters"):
            assert torch.equal(og[k], oe[k]), (tick, k)
        # the carried iteration counts (the list's order inside a class is immaterial)
        assert torch.equal(graphed.order_ws[:B], eager.order_ws[:B]), tick


def _assert_grouping_state(solver, prev, inp, iters, what):
    """The grouped solver's workspace after a call: order_ws[:B] carries this
    call's iteration counts to the next, and order_ws[B:2B] -- the list the
    call ran -- is a permutation of the robots in (pattern, min(previous
    iterations, 15)) order; `prev` is order_ws[:B] from before the call."""
    B = solver.batch
    assert torch.equal(solver.order_ws[:B], iters), what  # carried for the next call
    lst = solver.order_ws[B:2 * B].cpu().numpy()
    assert np.array_equal(np.sort(lst), np.arange(B)), what
    m, rs = inp["mode"][lst], inp["right_support"][lst]
    pat = np.where(m == 102, np.where(rs == 0, 1, np.where(rs == 1, 2, 0)),
                   np.where(m == 101, np.where(rs == 0, 3, np.where(rs == 1, 4, 0)), 0))
    key = pat * 16 + np.minimum(prev.cpu().numpy()[lst], 15)
    assert np.all(np.diff(key) >= 0), what


def test_force_qp_grouped_launch_is_bit_identical():
    """qloco_force_qp_solve_ordered groups the robots by swing-leg pattern and
    previous iteration count before the launch; every robot's
    arithmetic is unchanged, so grf_opt / F_leg_ref / status / iterations equal
    the ungrouped launch's bit for bit, tick after tick (the member state and
    the grouping state both carried).  B = 1001: a partial last wavefront.
    The workspace's list is a permutation in (pattern, previous iterations)
    order."""
    dev = _dev()
    rng = np.random.default_rng(11)
    B, ticks = 1001, 4
    grouped = qp.ForceQP(batch=B, device=dev)
    plain = qp.ForceQP(batch=B, device=dev, grouped=False)
    assert grouped.order_ws.numel() == 2 * B + 160
    for tick in range(ticks):
        inp = force_inputs(rng, B)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items()}
        prev = grouped.order_ws[:B].clone()
        og = grouped.step(**d)
        op = plain.step(**d)
        torch.cuda.synchronize()
        for k in ("grf_opt", "F_leg_guess", "F_leg_ref", "qp_solution", "status", "iters"):
            assert torch.equal(og[k], op[k]), (tick, k)
        _assert_grouping_state(grouped, prev, inp, op["iters"], tick)


# ---- the force block on the families of tests/force_cases.py ----------------

FORCE_OUT = ("grf_opt", "F_leg_guess", "F_leg_ref", "qp_solution", "status", "iters")
FORCE_LAUNCHES = [(False, 8), (True, 8), (False, 16), (True, 16)]  # (grouped, group width)


def _force_dev(d, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def _force_set_params(solver, over):
    """The tick's constants: the solver's own (sim or hardware copy) with the
    family's overrides (alpha, beta, gamma) -- equal to the restatement's."""
    prm = FC.oracle_params(**over)
    for k in ("alpha", "beta", "gamma", "fz_max"):
        setattr(solver.params, k, getattr(prm, k))
    assert (solver.params.mass, solver.params.mu) == (prm.mass, prm.mu)


def _force_step(solver, d, dev):
    out = solver.step(**_force_dev(d, dev))
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in FORCE_OUT}


class _group_width:
    def __init__(self, gw):
        self.gw = gw

    def __enter__(self):
        from quadrupedal_loco_amd._lib import lib
        self.prev = lib().qloco_force_set_group_width(self.gw)
        assert self.prev in (8, 16)

    def __exit__(self, *exc):
        from quadrupedal_loco_amd._lib import lib
        lib().qloco_force_set_group_width(self.prev)


@pytest.mark.parametrize("grouped,gw", FORCE_LAUNCHES)
@pytest.mark.parametrize("name", FC.FAMILIES)
def test_force_qp_family_parity(name, grouped, gw):
    """qp.ForceQP on every family of tests/force_cases.py (B = 64, two or
    three ticks, member state carried) against the restatement, through the
    plain and the grouped launch at both group widths.  The census the CPU
    tests assert on the restatement (tests/test_oracle.py, seed 3):
      baseline      all OK; double support at >= 4 iterations on 12 / 26 robots
      heavy         all OK; a leg at fz_max on 47 / 55; 1-5 iterations
      lateral       all OK; friction rows active on 64 / 64; up to 9 iterations
      bad_position  tick 1: NOT_PD, 0 iterations on 32 (16 NaN, 16 +Inf), 32 OK
      zero_weights  tick 1: NOT_PD on 64
      alpha0        all OK; closed form on 43 / 30 robots, restatement 1.42e-14 N
      nan_demand    tick 0: qp_solution 0 on 16, NaN grf_opt on 12; 12 / 2 stay
      odd_flags     tick 1: pattern 0 on 64, F_leg_ref carried, all OK
      hw_heavy / hw_lateral   as heavy / lateral with mass 14, mu 0.5
    Per robot and tick: F_leg_guess, F_leg_ref, qp_solution, status and
    iterations equal (NaN by position); grf_opt within 1e-9 relative / 1e-8 N,
    equal by position on the fallback rows, and bit-identical on >= 90 % of
    this family's solved robots.  On NOT_PD robots grf_opt is bit-equal to its
    value before the call (the definition in include/qloco.h); a healthy batch
    of the same size is launched just before every such tick, so the LDS the
    failing groups find is other robots' data and not zeros.  alpha0: the
    kernel within 16 x the restatement's own error of the closed form.
    Grouped: the workspace's list stays a permutation in class order, also on
    the tick after the NOT_PD robots left 0 iterations in it."""
    dev = _dev()
    ticks, run = FC.family(name)
    B = FC.BATCH
    hw = name.startswith("hw_")
    solver = qp.ForceQP(batch=B, device=dev, grouped=grouped, hw=hw)
    primer = qp.ForceQP(batch=B, device=dev, grouped=grouped)
    prime_in = _force_dev(FC.ticks_of("heavy", B=B)[0][0], dev)
    exact = solved = 0
    with _group_width(gw):
        for t, ((d, over), r) in enumerate(zip(ticks, run.ticks)):
            _force_set_params(solver, over)
            before = solver.grf_opt.cpu().numpy().copy()
            prev = solver.order_ws[:B].clone() if grouped else None
            bad = r["status"] == FC.NOT_PD
            if bad.any():
                primer.step(**prime_in)
            g = _force_step(solver, d, dev)
            what = (name, grouped, gw, t)
            for k in ("F_leg_guess", "F_leg_ref"):
                assert np.array_equal(g[k], r[k], equal_nan=True), (what, k)
            for k in ("qp_solution", "status", "iters"):
                assert np.array_equal(g[k], r[k]), (what, k, g[k], r[k])
            fb =r["qp_solution"] == 0
            assert np.array_equal(g["grf_opt"][fb], r["grf_opt"][fb], equal_nan=True), what
            assert np.array_equal(np.isnan(g["grf_opt"]), np.isnan(r["grf_opt"])), what
            assert np.allclose(g["grf_opt"][~fb], r["grf_opt"][~fb], rtol=1e-9, atol=1e-8), what
            assert g["grf_opt"][bad].tobytes() == before[bad].tobytes(), (what, g["grf_opt"][bad], before[bad])
            if bad.any():
                assert np.all(np.abs(before[bad]).max(axis=1) > 1.0), what
            ok = (r["status"] == FC.OK) & ~fb
            exact += int(np.sum(np.all(g["grf_opt"][ok] == r["grf_opt"][ok], axis=1)))
            solved += int(ok.sum())
            if name == "alpha0":
                x, rows = FC.alpha0_closed_form(d, over, r)
                err_ref = np.abs(r["grf_opt"][rows] - x[rows]).max()
                err = np.abs(g["grf_opt"][rows] - x[rows]).max()
                print("alpha0 tick %d: %d robots, |grf - closed form| %.3g (restatement %.3g, bound %.3g)" % (
                    t, len(rows), err, err_ref, 16 * err_ref))
                assert len(rows) >= 30 and err <= 16 * err_ref, (what, err, err_ref)
            if grouped:
                _assert_grouping_state(solver, prev, d, solver.iters, what)
    print("%s grouped=%s gw=%d: grf_opt bit-identical on %d of %d solved" % (name, grouped, gw, exact, solved))
    assert solved >= 64 and exact >= 0.9 * solved, (name, exact, solved)


@pytest.mark.parametrize("grouped,gw", FORCE_LAUNCHES)
def test_force_qp_bad_robots_do_not_disturb_their_neighbours(grouped, gw):
    """B = 67 `heavy` robots over three ticks; on ticks 1 and 2 the robots at
    positions 0, 7, 8 and 66 -- a group boundary of a wave at both widths and
    the partial last block -- get a NaN base_p[0], a NaN demand, a +Inf
    base_p[0] and a NaN demand.  The bad robots end NOT_PD with grf_opt kept
    (0, 8) or in the F_leg_guess fallback (7, 66); every other robot's outputs
    equal, bit for bit, those of the same batch with the four left healthy."""
    dev = _dev()
    B = 67
    ticks = FC.ticks_of("heavy", B=B, ticks=3)
    poisoned = []
    for t, (d, over) in enumerate(ticks):
        d = {k: v.copy() for k, v in d.items()}
        if t >= 1:
            FC.bad_position(d, rows_nan=[0], rows_inf=[8])
            FC.nan_demand(d, rows=[7, 66])
        poisoned.append((d, over))
    healthy = np.setdiff1d(np.arange(B), [0, 7, 8, 66])
    a = qp.ForceQP(batch=B, device=dev, grouped=grouped)
    b = qp.ForceQP(batch=B, device=dev, grouped=grouped)
    with _group_width(gw):
        for t in range(3):
            before = b.grf_opt.cpu().numpy().copy()
            ga = _force_step(a, ticks[t][0], dev)
            gb = _force_step(b, poisoned[t][0], dev)
            for k in FORCE_OUT:
                assert ga[k][healthy].tobytes() == gb[k][healthy].tobytes(), (grouped, gw, t, k)
            assert np.all(ga["status"] == FC.OK) and np.all(ga["qp_solution"] == 1)
            if t >= 1:
                assert gb["status"][[0, 8]].tolist() == [FC.NOT_PD, FC.NOT_PD] and np.all(gb["iters"][[0, 8]] == 0)
                assert gb["grf_opt"][[0, 8]].tobytes() == before[[0, 8]].tobytes()
                assert np.all(np.abs(before[[0, 8]]).max(axis=1) > 1.0)
                assert np.all(gb["qp_solution"][[7, 66]] == 0)
                assert np.array_equal(gb["grf_opt"][[7, 66]], gb["F_leg_guess"][[7, 66]], equal_nan=True)


def test_hw_torque_ff_bit_exact():
    """The hardware loop's feed-forward after force_opt (unitree_legged_real
    torque_mode.cpp:1370-1384: stand-up ramp blend of grf_opt with the
    stand-up GRF, tau = -J^T F, no gravity compensation) against the oracle's
    restatement, bit for bit, over the ramp (dynamic_count 0 .. 700: rate 0,
    partial, 1, clamped)."""
    dev = _dev()
    rng = np.random.default_rng(5)
    B = 1003
    J = rng.normal(0, 0.3, (B, 4, 9))
    g = rng.normal(0, 40, (B, 12))
    base = rng.normal(0, 30, (B, 12))
    cnt = rng.integers(0, 700, B).astype(np.int32)
    cnt[:4] = [0, 1, 500, 501]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tau = qp.hw_torque_ff(d(J), d(g), d(base), d(cnt)).cpu().numpy()
    for b in range(B):
        ref = np.zeros(12)
        O.lib().qo_hw_torque_ff(O.P(np.ascontiguousarray(J[b])), O.P(g[b].copy()), O.P(base[b].copy()),
                                int(cnt[b]), O.P(ref))
        assert np.array_equal(tau[b], ref), (b, tau[b], ref)
    with pytest.raises(ValueError):
        qp.hw_torque_ff(d(J), d(g), d(base), d(cnt.astype(np.int64)))


def test_body_mpc_matches_restatement_over_a_gait():
    dev = _dev()
    rng = np.random.default_rng(11)
    B = 16
    solver = qp.BodyMPC(batch=B, device=dev)
    ostates = []
    for b in range(B):
        s = O.BodyState()
        O.lib().qo_body_init(C.byref(s))
        ostates.append(s)
    for i in list(range(96, 180)) + list(range(1905, 1925)):
        zmp = rng.normal(0, 0.02, (B, 2, 5))
        ang = rng.normal(0, 0.02, (B, 2, 5))
        rf = rng.normal(0, 0.05, (B, 2, 5))
        lf = rng.normal(0, 0.05, (B, 2, 5))
        acc = rng.normal(0, 0.5, (B, 3, 5))
        bs = rng.normal(0, 0.05, (B, 4))
        cm = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1).reshape(a.shape[0], -1))
        ins = dict(i=np.full(B, i, np.int32), bodyangle_state=bs, zmp_ref=cm(zmp),
                   angle_ref=cm(ang), rfoot_ref=cm(rf), lfoot_ref=cm(lf), comacc_ref=cm(acc))
        out = solver.step(**{k: torch.from_numpy(v).to(dev) for k, v in ins.items()})
        torch.cuda.synchronize()
        traj = out["com_traj"].cpu().numpy()
        status = out["status"].cpu().numpy()
        state = solver.state.cpu().numpy()
        for b in range(B):
            ct = np.zeros(14)
            est = C.c_int(0)
            O.lib().qo_body_theta_mpc(C.byref(ostates[b]), i, O.P(np.ascontiguousarray(bs[b])),
                                      O.P(ins["zmp_ref"][b].copy()), O.P(ins["angle_ref"][b].copy()),
                                      O.P(ins["rfoot_ref"][b].copy()), O.P(ins["lfoot_ref"][b].copy()),
                                      O.P(ins["comacc_ref"][b].copy()), O.P(np.zeros(9)), O.P(ct),
                                      C.byref(est))
            assert np.allclose(traj[b], ct, rtol=1e-9, atol=1e-12), (i, b, traj[b], ct)
            assert status[b] == est.value, (i, b, status[b], est.value)
            if i >= 100:
                o = ostates[b]
                assert (int(state[b, 26]), int(state[b, 27]), int(state[b, 28])) == \
                    (o.bjx1, o.bjx2, o.t_yu), (i, b)
    for s in ostates:
        O.lib().qo_body_free(C.byref(s))


@pytest.mark.parametrize("name", BC.FAMILIES)
def test_body_mpc_family_parity(name):
    """qp.BodyMPC on the families of tests/body_cases.py (B = 16, i = 96 ..
    139: 640 acting calls) against the restatement; the census the CPU tests
    assert (tests/test_oracle.py):
      nan_reference     all OK; the !ok fallback and a NaN com_traj row on 160
      tilted_reference  all OK; more than one active-set iteration on 640 of
                        640 calls (up to 17), the post-solve clamps taken 8
                        times (counted in an instrumented scratch copy of the
                        restatement); a theta at its bound on 428 rows, the
                        torque on 380
      nan_accel         NOT_PD on 12 calls (G holds the NaN), OK on 628
    Every call: status equal, com_traj NaN in the same positions and within
    1e-9 relative / 1e-12 elsewhere, the carried _V_ini likewise, the
    schedule integers equal.  On NOT_PD calls _V_ini entries 1-3 and 5-7
    (0 and 4 are rewritten after the solve) are bit-equal to their values
    before the call -- non-zero, and a batch of other robots is launched just
    before, so the LDS the failing groups find is not zeros."""
    dev = _dev()
    steps, run = BC.family(name)
    B = BC.BATCH
    solver = qp.BodyMPC(batch=B, device=dev)
    primer = qp.BodyMPC(batch=B, device=dev)
    prime_in = {k: torch.from_numpy(v).to(dev) for k, v in BC.steps_of("tilted_reference", steps=(120,))[0][1].items()}
    keep = [5, 6, 7, 9, 10, 11]  # state columns of _V_ini entries 1-3, 5-7
    for (i, ins), r in zip(steps, run.steps):
        before = solver.state.cpu().numpy().copy()
        bad = r["status"] == BC.NOT_PD
        if bad.any():
            primer.step(**prime_in)
        out = solver.step(**{k: torch.from_numpy(v).to(dev) for k, v in ins.items()})
        torch.cuda.synchronize()
        traj, status = out["com_traj"].cpu().numpy(), out["status"].cpu().numpy()
        state = solver.state.cpu().numpy()
        assert np.array_equal(status, r["status"]), (name, i, status, r["status"])
        assert np.array_equal(np.isnan(traj), np.isnan(r["com_traj"])), (name, i)
        assert np.allclose(traj, r["com_traj"], rtol=1e-9, atol=1e-12, equal_nan=True), (name, i)
        if i >= 100:
            assert np.array_equal(state[:, 26:29].astype(np.int32), r["sched"]), (name, i)
            assert np.array_equal(state[:, 29].astype(np.int32), r["qp_solution"]), (name, i)
            assert np.array_equal(np.isnan(state[:, 4:12]), np.isnan(r["V_after"])), (name, i)
            # angular accelerations, up to 1389 rad/s^2; theta = .. + 5e-5 V, so
            # com_traj's 1e-12 absolute is 2e-8 here: 1e-9 is the tighter one
            assert np.allclose(state[:, 4:12], r["V_after"], rtol=1e-9, atol=1e-9, equal_nan=True), (name, i)
        assert state[bad][:, keep].tobytes() == before[bad][:, keep].tobytes(), (name, i)
        if bad.any():
            assert np.all(np.abs(before[bad][:, keep]).max(axis=1) > 0), (name, i)


def test_indexfind_bit_exact():
    dev = _dev()
    s = O.BodyState()
    O.lib().qo_body_init(C.byref(s))
    tx = np.array(s.tx[:])
    t = np.concatenate([np.linspace(0, tx[-1] - 1e-9, 2001), tx[:-1], np.nextafter(tx[:-1], -1),
                        np.arange(0, 1880) * 0.01])
    j = qp.indexfind(torch.from_numpy(t).to(dev)).cpu().numpy()
    ref = np.array([O.lib().qo_body_indexfind(C.byref(s), float(v)) for v in t])
    assert np.array_equal(j, ref)
    O.lib().qo_body_free(C.byref(s))


# ---- Goldfarb-Idnani kernels on the families of tests/qp_cases.py ----------

def _is_fast(n, p, m):
    """qloco_eiquadprog_solve's dispatch: gi_kernel, else gi_wide_kernel."""
    return n <= 16 and p <= 16 and m <= 64


def _gpu_solve(dev, probs, rows=None, **kw):
    """qp.eiquadprog_solve over a list of problems -> numpy dict."""
    G, _, CE, _, CI, _ = probs[0]
    n, p, m = G.shape[0], CE.shape[1], CI.shape[1]
    sel = probs if rows is None else [probs[b] for b in rows]
    res = qp.eiquadprog_solve(*(torch.from_numpy(Q.stack(sel, k)).to(dev) for k in range(6)),
                              n=n, p=p, m=m, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _assert_parity(res, sol, fast, what):
    """Status and iterations equal to the restatement on every instance; on
    its OK instances x and f within 1e-9 relative, and (four-per-wave kernel)
    x bit-identical on >= 90 % of them."""
    assert np.array_equal(res["status"], sol.status), (what, res["status"], sol.status)
    assert np.array_equal(res["iters"], sol.iters), (what, res["iters"], sol.iters)
    ok = np.flatnonzero(sol.status == Q.OK)
    exact = 0
    for b in ok:
        xo, fo = sol.x[b], sol.f[b]
        err = np.abs(res["x"][b] - xo).max()
        assert err <= 1e-9 * max(1.0, np.abs(xo).max()), (what, b, err)
        assert abs(res["f"][b] - fo) <= 1e-9 * max(1.0, abs(fo)), (what, b, res["f"][b], fo)
        exact += int(np.array_equal(res["x"][b], xo))
    print("%s: OK %d of %d, x bit-identical on %d" % (what, len(ok), len(sol.status), exact))
    if fast:
        assert exact >= 0.9 * len(ok), (what, exact, len(ok))
    return len(ok)


@pytest.mark.parametrize("n,p,m,zero_ce", Q.FAMILY_A)
def test_gi_parity_feasible_gaussian(n, p, m, zero_ce):
    """Family A at the four-per-wave kernel's shapes (its capacity (16, *,
    64) and the body-QP shape (8, 0, 48) included): at least 3/4 of the 64
    instances are OK in the restatement (tests/test_oracle.py), and on those
    x and f are compared."""
    probs, sol = Q.family_a(n, p, m, zero_ce)
    solved = _assert_parity(_gpu_solve(_dev(), probs), sol, _is_fast(n, p, m), ("A", n, p, m))
    assert solved == int(np.sum(sol.status == Q.OK)) >= 48


@pytest.mark.parametrize("n", Q.FAMILY_B)
def test_gi_parity_and_closed_form_box(n):
    """Family B (n <= 16: gi_kernel, above: gi_wide_kernel): parity with the
    restatement, which solves all 64 and takes 66 to 57,289 h == 0 skips of
    the add-constraint Givens sweep per shape (n >= 4); and
    x = clip(-g0 / diag G, lo, hi) within 16 x the restatement's own error
    against that closed form on these same inputs, computed here from its
    results (measured 8.88e-16 / 2.66e-15 / 3.11e-15 | 1.78e-15 / 2.22e-15 /
    2.78e-15 at n = 1, 4, 16 | 17, 32, 64)."""
    probs, sol, xc = Q.family_b(n)
    res = _gpu_solve(_dev(), probs)
    assert _assert_parity(res, sol, _is_fast(n, 0, 2 * n), ("B", n)) == 64
    err_ref = np.abs(sol.x - xc).max()
    err = np.abs(res["x"] - xc).max()
    print("box n = %d: max |x - closed form| %.3g (restatement %.3g, bound %.3g)" % (n, err, err_ref, 16 * err_ref))
    assert err <= 16 * err_ref, (n, err, err_ref)


@pytest.mark.parametrize("n,m", Q.FAMILY_C)
def test_gi_parity_coupled_ties(n, m):
    """Family C: exact ties in the most-violated-constraint scan on 14 / 19 /
    38 / 32 / 58 of the 64 instances at (4,8) (8,24) (16,64) (17,65) (32,96).
    A restatement whose scan keeps the last tied index instead of the first
    changes status or iteration count on 3 / 7 / 13 / 19 / 33 instances, so
    the iteration equality asserted here fails for a butterfly with the
    wrong tie rule (ov == bv && oi < bi)."""
    probs, sol = Q.family_c(n, m)
    assert _assert_parity(_gpu_solve(_dev(), probs), sol, _is_fast(n, 0, m), ("C", n, m)) == 64


@pytest.mark.parametrize("n,p", Q.FAMILY_E)
def test_gi_closed_form_equality_only(n, p):
    """Family E: no inequalities, full-rank CE; one iteration, and x equals
    the KKT solution (numpy float64, refined on a longdouble residual)
    within 16 x the restatement's own error on these same inputs, computed
    here from its results, both relative to max(1, |x|max) (measured
    7.86e-14 / 5.07e-16 / 8.15e-15)."""
    probs, sol, xk = Q.family_e(n, p)
    res = _gpu_solve(_dev(), probs)
    assert _assert_parity(res, sol, _is_fast(n, p, 0), ("E", n, p)) == 64
    assert np.all(res["iters"] == 1)
    scale = np.maximum(1.0, np.abs(xk).max(axis=1))
    err_ref = (np.abs(sol.x - xk).max(axis=1) / scale).max()
    err = (np.abs(res["x"] - xk).max(axis=1) / scale).max()
    print("equality (%d, %d): max relative error %.3g (restatement %.3g, bound %.3g)" % (n, p, err, err_ref, 16 * err_ref))
    assert err <= 16 * err_ref, (n, p, err, err_ref)


def _assert_same_bits(a, b, rows_a, rows_b, what, keys=("x", "f", "status", "iters")):
    for k in keys:
        va, vb = a[k][rows_a], b[k][rows_b]
        same = va.tobytes() == vb.tobytes()  # NaN-safe bit comparison
        assert same, (what, k, va, vb)


def test_gi_wave_mates_do_not_disturb_each_other():
    """Family D, B = 67 at (8, 0, 24): consecutive instances cycle NOT_PD /
    INFEASIBLE / solved with an active set / solved with every constraint
    slack, so each wave of gi_kernel holds one group that leaves at the
    failed Cholesky, one that ends INFEASIBLE mid-loop and two that solve;
    the last wave holds three.  Every instance equals, bit for bit, the same
    instance solved alone (B = 1); status, iterations and f equal the
    restatement's, and so does x on OK instances and on NOT_PD ones (x = 0).
    With one instance's g0 turned to NaN the other 66 keep their bits."""
    dev = _dev()
    probs, sol = Q.family_d()
    B = len(probs)
    assert sol.census() == {Q.OK: 33, Q.INFEASIBLE: 17, Q.NOT_PD: 17}
    res = _gpu_solve(dev, probs)
    _assert_parity(res, sol, True, "D")
    finite = np.isfinite(sol.f)
    assert np.array_equal(np.isinf(res["f"]), ~finite) and np.all(res["f"][~finite] > 0)
    assert np.allclose(res["f"][finite], sol.f[finite], rtol=1e-9, atol=1e-9)
    bad = np.flatnonzero(sol.status == Q.NOT_PD)
    assert np.all(res["x"][bad] == 0.0) and np.all(sol.x[bad] == 0.0) and np.all(res["iters"][bad] == 0)
    for b in range(B):
        alone = _gpu_solve(dev, probs, rows=[b])
        _assert_same_bits(alone, res, [0], [b], ("alone", b))
    poisoned = 6  # an active-set instance, second wave
    assert sol.status[poisoned] == Q.OK and sol.iters[poisoned] > 1
    pp = list(probs)
    G, g0, CE, ce0, CI, ci0 = pp[poisoned]
    pp[poisoned] = (G, np.full_like(g0, np.nan), CE, ce0, CI, ci0)
    res_p = _gpu_solve(dev, pp)
    others = [b for b in range(B) if b != poisoned]
    _assert_same_bits(res_p, res, others, others, "NaN wave-mate")
    assert np.all(np.isnan(res_p["x"][poisoned]))


def _capi_solve(dev, probs, B, pad=0, rows_extra=4, optional=True, sentinel=-777.25):
    """qloco_eiquadprog_solve through the C ABI on the first B problems;
    operands with `pad` unused trailing elements per instance (stride k +
    pad, the padding NaN); outputs allocated with rows_extra rows of
    sentinel after the B used ones.  optional=False passes NULL for f,
    status and iters."""
    from quadrupedal_loco_amd._lib import check, lib, ptr
    G, _, CE, _, CI, _ = probs[0]
    n, p, m = G.shape[0], CE.shape[1], CI.shape[1]
    ops, strides = [], []
    for k in range(6):
        a = Q.stack(probs[:B], k)
        if a.shape[1] == 0:
            ops.append(None)
            strides.append(0)
            continue
        buf = np.full((B, a.shape[1] + pad), np.nan)
        buf[:, :a.shape[1]] = a
        ops.append(torch.from_numpy(buf).to(dev))
        strides.append(a.shape[1] + pad)
    R = B + rows_extra
    out = {"x": torch.full((R, n), sentinel, dtype=torch.float64, device=dev),
           "f": torch.full((R,), sentinel, dtype=torch.float64, device=dev),
           "status": torch.full((R,), -777, dtype=torch.int32, device=dev),
           "iters": torch.full((R,), -777, dtype=torch.int32, device=dev)}
    opt = [ptr(out[k]) if optional else None for k in ("f", "status", "iters")]
    args = []
    for t, s in zip(ops, strides):
        args += [ptr(t), s]
    check(lib().qloco_eiquadprog_solve(n, p, m, B, *args, ptr(out["x"]), *opt, None),
          "qloco_eiquadprog_solve")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("shape,batches", [((12, 3, 24, 0), (1, 2, 3, 5, 67)), ((17, 0, 8, 0), (1, 3))])
def test_gi_ragged_batches_and_guard_rows(shape, batches):
    """Tail waves of gi_kernel (B mod 4 != 0, B = 1) and single blocks of
    gi_wide_kernel through the C ABI: rows < B carry the bits of the same
    instances in the B = 67 run (which matches the restatement), and the
    four sentinel rows allocated after them are untouched -- also with f,
    status and iters NULL, when those buffers stay sentinel throughout."""
    dev = _dev()
    n, p, m, zero_ce = shape
    rng = np.random.default_rng(Q.shape_seed("R", n, p, m))
    probs = [random_feasible_qp(rng, n, p, m, zero_ce) for _ in range(67)]
    full = _capi_solve(dev, probs, 67)
    _assert_parity({k: v[:67] for k, v in full.items()}, Q.Solved(probs), _is_fast(n, p, m), ("ragged", shape))
    for B in batches:
        for optional in (True, False):
            out = _capi_solve(dev, probs, B, optional=optional)
            keys = ("x", "f", "status", "iters") if optional else ("x",)
            _assert_same_bits(out, full, slice(0, B), slice(0, B), ("ragged", B, optional), keys)
            assert np.all(out["x"][B:] == -777.25), (B, optional)
            lo = B if optional else 0
            assert np.all(out["f"][lo:] == -777.25), (B, optional)
            assert np.all(out["status"][lo:] == -777) and np.all(out["iters"][lo:] == -777), (B, optional)


@pytest.mark.parametrize("n,p,m", [(12, 3, 24), (20, 3, 8)])
def test_gi_operand_strides(n, p, m):
    """Stride 0 and padded strides, both kernels.  Each of the six operands
    in turn is passed as one 1-D tensor shared by all instances (the others
    stacked): the results are the bits of the packed call whose stack
    repeats that operand.  All six shared with batch= give B copies of the
    single solve.  Every operand with a padded stride (k + 3, NaN padding)
    through the C ABI equals the packed call too."""
    dev = _dev()
    B = 9
    rng = np.random.default_rng(Q.shape_seed("S", n, p, m))
    base = [random_feasible_qp(rng, n, p, m) for _ in range(B)]
    dt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for shared in range(6):
        probs = [tuple(base[0][k] if k == shared else pr[k] for k in range(6)) for pr in base]
        packed = _gpu_solve(dev, probs)
        if shared == 0:
            assert np.array_equal(packed["status"], Q.Solved(probs).status)
        ops = [dt(Q.stack(probs[:1], k)[0]) if k == shared else dt(Q.stack(probs, k)) for k in range(6)]
        res = qp.eiquadprog_solve(*ops, n=n, p=p, m=m)
        torch.cuda.synchronize()
        _assert_same_bits({k: v.cpu().numpy() for k, v in res.items()}, packed, slice(0, B), slice(0, B),
                          ("shared", shared))
        assert res["x"].shape == (B, n)
    one = _gpu_solve(dev, base, rows=[0])
    res = qp.eiquadprog_solve(*(dt(Q.stack(base[:1], k)[0]) for k in range(6)), n=n, p=p, m=m, batch=5)
    torch.cuda.synchronize()
    for b in range(5):
        _assert_same_bits({k: v.cpu().numpy() for k, v in res.items()}, one, [b], [0], ("all shared", b))
    packed = _gpu_solve(dev, base)
    padded = _capi_solve(dev, base, B, pad=3)
    _assert_same_bits(padded, packed, slice(0, B), slice(0, B), "padded strides")
    assert np.all(padded["x"][B:] == -777.25)


@pytest.mark.parametrize("n,p,m,zero_ce", Q.EDGES)
def test_gi_edges_and_dispatch_boundary(n, p, m, zero_ce):
    """n = 1, m = 0, p = 0, the four-per-wave kernel's full capacity
    (16, 16, 64) with two zero CE columns (me = p / A(i) quirks: the
    restatement reports 35 OK, 29 INFEASIBLE), and one step past each
    dispatch limit -- (17, 0, 8), (4, 0, 65), (20, 17, 8) run gi_wide_kernel.
    Parity with the restatement as above; unconstrained shapes end after one
    iteration at x = -G^-1 g0 (numpy, 1e-9 relative)."""
    probs, sol = Q.edge(n, p, m, zero_ce)
    res = _gpu_solve(_dev(), probs)
    solved = _assert_parity(res, sol, _is_fast(n, p, m), ("edge", n, p, m))
    assert solved == int(np.sum(sol.status == Q.OK)) >= (16 if (n, p, m) == (16, 16, 64) else 64)
    if p == 0 and m == 0:
        assert np.all(res["iters"] == 1)
        for b, pr in enumerate(probs):
            xu = -np.linalg.solve(pr[0], pr[1])
            assert np.abs(res["x"][b] - xu).max() <= 1e-9 * max(1.0, np.abs(xu).max()), b


@pytest.mark.parametrize("n,p,m", [s for s in Q.OVERFULL if s[0] > 2])
def test_gi_more_equalities_than_variables(n, p, m):
    """More live CE columns than variables, (4, 6, 4) on gi_kernel and
    (20, 24, 8) on gi_wide_kernel: QLOCO_DEGENERATE when column n + 1
    arrives, 0 iterations, x as the first n equalities left it -- equal to
    the restatement, which guards the same step (both would otherwise write
    column n of an n-column R)."""
    probs, sol = Q.overfull(n, p, m)
    assert sol.census() == {Q.DEGENERATE: len(probs)}
    res = _gpu_solve(_dev(), probs)
    assert np.array_equal(res["status"], sol.status) and np.all(res["iters"] == 0)
    for b in range(len(probs)):
        err = np.abs(res["x"][b] - sol.x[b]).max()
        assert err <= 1e-9 * max(1.0, np.abs(sol.x[b]).max()), (b, err)
        assert abs(res["f"][b] - sol.f[b]) <= 1e-9 * max(1.0, abs(sol.f[b])), b
