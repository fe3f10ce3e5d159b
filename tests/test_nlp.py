"""Step-timing SQP of the slow planner (csrc/qloco_nlp.hip, include/qloco.h
section 14) -- CPU tests: the restatement (tests/nlp_ref.py) against an
independent short transcription of the QP assembly, the branch census and
finiteness of the GPU tests' inputs, the agreement of the restatement's two
formulations and the spreads the GPU bounds are built from, the selection of
the chain test, and the C ABI's host-side checks.
"""
import collections
import ctypes as C
import math

import numpy as np

import nlp_ref as R
from quadrupedal_loco_amd import _lib, nlp

SYMBOLS = ("qloco_nlp_params_default", "qloco_nlp_workspace_bytes", "qloco_nlp_init", "qloco_nlp_step_timing",
           "qloco_nlp_get_state", "qloco_nlp_set_state", "qloco_nlp_set_group_width")


def test_section_14_symbols_and_bindings():
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert L.qloco_abi_version() == 1
    assert nlp.STATE == R.STATE == 309 and nlp.NS == R.NS == 27
    assert (nlp.SKIPPED, nlp.FINISHED) == (R.SKIPPED, R.FINISHED)


def test_params_default_round_trip():
    p = nlp.default_params()
    for k, v in R.DEFAULTS.items():
        assert getattr(p, k) == v, k
    assert [f[0] for f in _lib.NlpParams._fields_][:-1] == list(R.PARAM_ORDER)
    assert C.sizeof(_lib.NlpParams) == 8 * 32
    q = nlp.default_params(lamda_comx=0.25, foot_width=0.01)
    assert q.lamda_comx == 0.25 and q.foot_width == 0.01 and q.t_max == 1.0
    try:
        nlp.default_params(nonsense=1.0)
    except ValueError:
        pass
    else:
        raise AssertionError("unknown parameter accepted")


def test_argument_validation_without_device_work():
    L = _lib.lib()
    p = nlp.default_params()
    one = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: every call below is refused
    assert L.qloco_nlp_workspace_bytes(-1) == -1 and L.qloco_nlp_workspace_bytes(0) == -1
    assert L.qloco_nlp_workspace_bytes(3) == 3 * 309 * 8
    assert L.qloco_nlp_init(None, 4, one, one, one, None, None) == 100
    assert L.qloco_nlp_init(C.byref(p), 0, one, one, one, None, None) == 100
    assert L.qloco_nlp_init(C.byref(p), 4, None, one, one, None, None) == 100
    assert L.qloco_nlp_init(C.byref(p), 4, one, None, one, None, None) == 100
    bad = nlp.default_params(dt=0.0)
    assert L.qloco_nlp_init(C.byref(bad), 4, one, one, one, None, None) == 100
    args = [one] * 6 + [None] * 6
    assert L.qloco_nlp_step_timing(None, 4, *args, None) == 100
    assert L.qloco_nlp_step_timing(C.byref(p), -1, *args, None) == 100
    for k in range(6):           # workspace, t_int, estimated_state, the feedbacks, vari_ini
        a = list(args)
        a[k] = None
        assert L.qloco_nlp_step_timing(C.byref(p), 4, *a, None) == 100, k
    assert L.qloco_nlp_get_state(4, None, one, None) == 100 and L.qloco_nlp_get_state(4, one, None, None) == 100
    assert L.qloco_nlp_set_state(0, one, one, None) == 100 and L.qloco_nlp_set_state(4, one, None, None) == 100
    assert L.qloco_nlp_set_group_width(5) == 100
    prev = L.qloco_nlp_set_group_width(8)
    assert prev in (4, 8, 16) and L.qloco_nlp_set_group_width(prev) == 8


def test_tick_kernels_are_spill_and_scratch_free():
    """Every instantiation of the tick kernel: no spilled register, no private
    segment, at most 256 registers (two waves per SIMD) and LDS for at least
    two one-wave workgroups per SIMD in the shipped form."""
    import test_kernel_resources as K
    ks = {n: k for n, k in K._kernels().items() if "nlp_step_kernel" in n}
    assert len(ks) == 4, sorted(ks)
    for n, k in ks.items():
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, n
        assert not k.get(".uses_dynamic_stack", False), n
        assert k[".vgpr_count"] + k[".agpr_count"] <= 256, (n, k[".vgpr_count"], k[".agpr_count"])
    shipped = ks["_ZN5qloco15nlp_step_kernelILi4ELb0EEEvNS_7NlpArgsE"]
    assert 8 * shipped[".group_segment_fixed_size"] <= 160 * 1024


def test_initialize_restatement():
    """FootStepInputs + Initialize for the reference's own inputs (:55-67,
    :131-138, :164-206)."""
    r = R.Robot(0.075, 2 * 0.12675)
    L = 0.075
    assert list(r.Lxx_ref) == [0, 0, 0, L / 2] + [L] * 10 + [0] + [-L] * 7 + [0] * 5
    W = 2 * 0.12675
    assert list(r.Lyy_ref) == [W / 2] + [(-1) ** j * W for j in range(1, 27)]
    assert r.footx_ref[4] == L / 2 and abs(r.footx_ref[14] - (L / 2 + 10 * L)) < 1e-15      # a running sum
    assert r.footy_ref[1] == W / 2 and abs(r.footy_ref[2] - (W / 2 - W)) < 1e-16
    assert (r.ts == 0.7).all() and np.allclose(r.td, 0.14, atol=1e-16) and r.tx[0] == 0.0
    assert np.allclose(r.tx[1:], 0.7 * np.arange(1, 27) - 1e-6, atol=1e-12)
    assert R.t_end_footstep() == 672
    rec = r.to_record()
    assert rec.shape == (309,) and np.array_equal(R.Robot().from_record(rec).to_record(), rec)


def _independent_assembly(rob, i, c):
    """The QP of one pass written the way the reference writes it: selection
    rows _SS1.._SS4 and matrix expressions (:1146-1165, :1188-1455, :1619-1634),
    no shared code with nlp_ref.Robot.assemble."""
    p, v, Wn, dt = rob.p, rob.vari.reshape(4, 1), rob.Wn, rob.p["dt"]
    S1, S2, S3, S4 = (np.eye(4)[k:k + 1] for k in range(4))
    pi = c["p"]
    cx, cvx, _, cy, cvy, _ = rob.feed
    Ax, Bx, Cx = cx - rob.footx_ref[pi], cvx / Wn, -0.5 * c["Lxr"]
    Ay, By, Cy = cy - rob.footy_ref[pi], cvy / Wn, -0.5 * c["Lyr"]
    Axv, Bxv, Cxv = Wn * Bx, Wn * Ax, -rob.endref[0]
    Ayv, Byv, Cyv = Wn * By, Wn * Ay, -rob.endref[1]
    w = (p["aax"], p["aay"], p["aaxv"], p["aayv"])
    A_, B_, C_ = (Ax, Ay, Axv, Ayv), (Bx, By, Bxv, Byv), (Cx, Cy, Cxv, Cyv)
    dot = lambda a, b: sum(wk * ak * bk for wk, ak, bk in zip(w, a, b))
    Q = np.diag([0.5 * p["bbx"], 0.5 * p["bby"], 0.5 * (p["rr1"] + dot(A_, A_)), 0.5 * (p["rr2"] + dot(B_, B_))])
    Q[2, 3] = Q[3, 2] = 0.5 * dot(A_, B_)
    q = np.array([[-p["bbx"] * c["Lxr"]], [-p["bby"] * c["Lyr"]], [-p["rr1"] * c["tr1_ref"] + dot(A_, C_)],
                  [-p["rr2"] * c["tr2_ref"] + dot(B_, C_)]])
    G, g0 = 2 * Q, 2 * Q @ v + q
    M = S3.T @ S3 - S4.T @ S4
    CE, ce0 = -(2 * M @ v), float((-(v.T @ M @ v)).item()) + 1
    rows, det = [], []

    def pair(row, hi, lo):
        # "up": row x <= hi  ->  A = row, b = -(row v) + hi ; "lp": -row x <= -lo
        rows.extend([row, -row])
        det.extend([-(row @ v).item() + hi, (row @ v).item() - lo])

    pair(S3, c["tr1_max"], c["tr1_min"])
    pair(S4, c["tr2_max"], c["tr2_min"])
    hw, fw = p["half_hip_width"], p["foot_width"]
    late = i >= round(2 * rob.ts[1] / dt) + 1
    if c["period"] % 2 == 0:
        fy = (-(fw + 0.01) if late else -(hw - 0.03), -(2 * hw + 0.03))
    else:
        fy = (2 * hw + 0.03, fw + 0.01 if late else hw - 0.03)
    pair(S1, p["footx_max"], p["footx_min"])
    pair(S2, fy[0], fy[1])
    if c["k_yu"] == 0:
        rows.extend([np.zeros((1, 4))] * 4)
        det.extend([0.0] * 4)
    else:
        pair(S1, rob.Lxx_ref[pi] + p["footx_vmax"] * dt, rob.Lxx_ref[pi] + p["footx_vmin"] * dt)
        pair(S2, rob.Lyy_ref[pi] + p["footy_vmax"] * dt, rob.Lyy_ref[pi] + p["footy_vmin"] * dt)
    sh, ch = math.sinh(Wn * dt), math.cosh(Wn * dt)
    blocks = []
    for kind in ("acc", "vel", "vel0"):
        for Sa, CC, cv, amax, amin in ((S1, Ax, cvx, p["comax_max"], p["comax_min"]),
                                       (S2, Ay, cvy, p["comay_max"], p["comay_min"])):
            if kind == "acc":
                a1, a2, a3, hi, lo, half = Wn * sh * Wn, -2 * Wn * sh * CC * Wn, 2 * Wn ** 2 * CC * ch, 2 * amax, 2 * amin, 1.0
            elif kind == "vel":
                a1, a2, a3 = ch * Wn, -2 * ch * CC * Wn, 2 * Wn * CC * sh - 2 * cv
                hi, lo, half = 2 * amax * dt, 2 * amin * dt, 1.0
            else:
                a1, a2, a3, hi, lo, half = Wn, -2 * CC * Wn, -2 * cv, 2 * amax * dt, 2 * amin * dt, 0.5
            up = a1 * Sa + a2 * S3 + (a3 - hi) * S4
            lp = -a1 * Sa - a2 * S3 - (a3 - lo) * S4
            up_d = a1 * Sa + a2 * S3 + (a3 - hi * half) * S4
            lp_d = -a1 * Sa - a2 * S3 - (a3 - lo * half) * S4
            blocks.append((up, lp, -(up_d @ v).item(), -(lp_d @ v).item()))
    for up, lp, du, dl in blocks:
        rows.extend([up, lp])
        det.extend([du, dl])
    A = np.vstack(rows)
    return G, g0.ravel(), CE.ravel(), ce0, -A.T, np.array(det)


def test_assembly_against_independent_transcription():
    """G, g0, CE, ce0, CI, ci0 element by element, at a tick with _k_yu == 0
    (the zero rows), an even and an odd step, before and after the footy limit
    switch, and after a push."""
    seen = collections.Counter()
    for i_stop in (1, 2, 28, 29, 40, 57, 60, 84):
        rob = R.Robot(0.06, 0.26)
        for i in range(1, i_stop):
            rob.tick(i)
        rob.feed = rob.feed + np.array([0.003, -0.04, 0.0, -0.002, 0.03, 0.0])
        captured = {}
        orig = rob.assemble

        def spy(i, c, _o=orig, _cap=captured, _rob=rob):
            if not _cap:
                _cap["v"], _cap["state"] = _rob.vari.copy(), _rob.to_record()
                _cap["arrays"] = _o(i, c)
                _cap["c"] = dict(c)
                return _cap["arrays"]
            return _o(i, c)

        rob.assemble = spy
        rob.tick(i_stop)
        c = captured["c"]
        twin = R.Robot(0.06, 0.26).from_record(captured["state"])
        twin.vari = captured["v"]
        want = _independent_assembly(twin, i_stop, c)
        va = np.abs(captured["v"])
        scales = dict(G=np.abs(want[0]).max(), g0=(np.abs(want[0]) @ va).max(), CE=np.abs(want[2]).max(),
                      ce0=va[2] ** 2 + va[3] ** 2 + 1, CI=np.abs(want[4]).max(),
                      ci0=(np.abs(want[4]).T @ va).max() + va.max() + 1)
        for name, g, w in zip(("G", "g0", "CE", "ce0", "CI", "ci0"), captured["arrays"], want):
            g, w = np.asarray(g, float), np.asarray(w, float)
            assert g.shape == w.shape, (i_stop, name)
            # same expressions in another association: a few ulps of the largest term of the
            # sums behind each array (g0 and ci0 cancel: G v against Sq_goal, A v against the limits)
            scale = scales[name]
            assert np.abs(g - w).max() <= 64 * np.finfo(float).eps * scale, (i_stop, name, np.abs(g - w).max())
            if name in ("G", "CE", "CI"):
                assert np.array_equal(g == 0, w == 0), (i_stop, name)  # the sparsity pattern, exactly
        seen["kyu0"] += c["k_yu"] == 0
        seen["even"] += c["period"] % 2 == 0
        seen["odd"] += c["period"] % 2 == 1
        seen["late"] += bool(c.get("late"))
        if c["k_yu"] == 0:
            assert not captured["arrays"][4][:, 8:12].any() and not captured["arrays"][5][8:12].any()
    assert seen["kyu0"] >= 2 and seen["even"] >= 2 and seen["odd"] >= 2 and seen["late"] >= 2, seen


# how often each branch must occur over the GPU tests' inputs (tick x robot)
# (tick x robot): every robot starts at i = 1; three step boundaries in 90 ticks
# (_k_yu == 0 once per robot each); _k_yu >= 20 on the last 8 ticks of a 28-tick
# step; _Tk < 0.1 _ts on its last two
CENSUS_MIN = dict(i1=67, kyu0=3 * 67 - 1, inf=100, clamp=3 * 8 * 67 - 100, skip=3 * 2 * 67 - 100, late=1500,
                  not_late=1500, even=1500, odd=3000, neg=30)


def test_branch_census_and_finiteness_of_the_gpu_test_inputs():
    count = collections.Counter()
    for name, kw in R.cases():
        a = R.rollout(**kw)
        assert (a["status"] == R.OK).all(), name
        for k in ("record_in", "record_out", "vari", "step", "com"):
            assert np.isfinite(a[k]).all(), (name, k)
        assert set(np.unique(a["pass_status"])) <= {R.SKIPPED, R.OK, R.INFEASIBLE}, name
        push = a["inputs"]["push"]
        assert np.abs(push[..., [0, 3]]).max() <= 0.004 and np.abs(push[..., [1, 4]]).max() <= 0.05
        if name == "main":
            assert (push != 0).any(axis=(1, 2)).sum() == len(R.PUSH_TICKS)
            assert a["steplength"].min() >= 0.04 and a["steplength"].max() <= 0.09
            assert np.abs(a["stepwidth"] / (2 * 0.12675) - 1).max() <= 0.1
        for row in a["census"]:
            for c in row:
                count["i1"] += c["i1"]
                count["kyu0"] += c["kyu0"]
                count["inf"] += c["inf"]                      # +inf returns whose partial iterate was added
                count["clamp"] += c["clamp"]
                count["skip"] += c["skip"]
                count["late"] += c["late"]
                count["not_late"] += not c["late"]
                count["even"] += c["even"]
                count["odd"] += not c["even"]
                count["neg"] += c["neg"]
        if name == "main":
            assert count["neg"] == 0                          # the late window is what reaches steps 15-21
            inf = a["pass_status"] == R.INFEASIBLE
            assert inf.any() and np.isfinite(a["vari"][inf.any(-1)]).all()
    print("census:", dict(count))
    for k, n in CENSUS_MIN.items():
        assert count[k] >= n, (k, count[k], n)


def test_formulations_agree_and_spreads_reproduce():
    """The two formulations choose the same status, iteration count and active
    set in every solve (asserted inside measure()), and their spreads are the
    figures tests/test_nlp_gpu.py hard-codes."""
    import test_nlp_gpu as G
    m = R.measure()
    for mode, committed in (("teacher", G.SPREAD_TEACHER), ("blend", G.SPREAD_BLEND), ("free", G.SPREAD_FREE)):
        print(mode, "measured:", m[mode])
        assert set(committed) == set(m[mode]), mode
        for k, v in committed.items():
            got = m[mode][k]
            assert (got == 0.0 and v == 0.0) or 0.5 * v <= got <= 2.0 * v, (mode, k, got, v)


def test_chain_selection_is_clear_of_every_decision_boundary():
    a = R.rollout(**dict(R.cases())["main"])
    mask = R.chain_mask(a)
    assert mask[::3].mean() >= 0.9
    (s0, s1), (x0, x1) = R.SLICES["ts"], R.SLICES["tx"]
    for t in range(0, a["t_int"].shape[0], 9):
        for b in np.nonzero(mask[t])[0][:8]:
            rec = a["record_out"][t, b]
            assert R.support_margin(rec[s0:s1], rec[x0:x1], int(a["t_int"][t, b])) > 1e-9
    # the margin sees a boundary: a schedule whose _tx sits on the sampling time
    ts, tx = np.full(27, 0.7), np.array([(28 * j) * 0.025 for j in range(27)])
    assert R.support_margin(ts, tx, 28) == 0.0 and R.support_margin(ts, tx - 1e-6, 28) > 1e-9
