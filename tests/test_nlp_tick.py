"""The rest of the slow planner's tick (csrc/qloco_nlp_tick.hip, include/qloco.h
section 15) -- CPU tests: the C ABI's symbols and host-side checks, the pinned
facts of section 14, the restatement (tests/nlp_tick_ref.py): that its two
formulations take the same branch on every robot-tick of the GPU tests'
inputs, that every branch occurs there, and that the spreads the GPU bounds
are built from reproduce; the new kernel's register and scratch figures.
"""
import collections
import ctypes as C

import numpy as np

import nlp_ref as R
import nlp_tick_ref as K
from quadrupedal_loco_amd import _lib, nlp

SYMBOLS = ("qloco_nlp_tick_params_default", "qloco_nlp_tick_workspace_bytes", "qloco_nlp_tick_init",
           "qloco_nlp_tick", "qloco_nlp_tick_get_state", "qloco_nlp_tick_set_state",
           "qloco_nlp_tick_set_group_width")


def test_section_15_symbols_and_bindings():
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert nlp.TICK_STATE == K.STATE == 374 and nlp.TICK_RING == K.RING == 48
    assert set(nlp.TICK_STATE_FIELDS) == set(K.SLICES) and all(nlp.TICK_STATE_FIELDS[k] == K.SLICES[k] for k in K.SLICES)
    p = nlp.default_tick_params()
    assert (p.lift_height, p.hcom) == (K.TICK_DEFAULTS["lift_height"], K.TICK_DEFAULTS["hcom"])
    assert C.sizeof(_lib.NlpTickParams) == 64
    assert L.qloco_nlp_tick_workspace_bytes(3) == 3 * (374 + 21) * 8


def test_section_14_is_as_it_was():
    L = _lib.lib()
    assert L.qloco_nlp_workspace_bytes(3) == 3 * 309 * 8 and nlp.STATE == 309
    assert C.sizeof(_lib.NlpParams) == 256
    assert L.qloco_abi_version() == 1


def test_argument_validation_without_device_work():
    L = _lib.lib()
    p, tp = nlp.default_params(), nlp.default_tick_params()
    one = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: every call below is refused
    assert L.qloco_nlp_tick_workspace_bytes(-1) == -1 and L.qloco_nlp_tick_workspace_bytes(0) == -1
    init = [one] * 4 + [None]    # nlp_workspace, tick_workspace, steplength, stepwidth, stepheight
    assert L.qloco_nlp_tick_init(None, C.byref(tp), 4, *init, None) == 100
    assert L.qloco_nlp_tick_init(C.byref(p), None, 4, *init, None) == 100
    assert L.qloco_nlp_tick_init(C.byref(p), C.byref(tp), 0, *init, None) == 100
    for k in range(4):
        a = list(init)
        a[k] = None
        assert L.qloco_nlp_tick_init(C.byref(p), C.byref(tp), 4, *a, None) == 100, k
    # t_max / dt ticks of a step, the look-back and the forecast slot must fit the ring
    long_step = nlp.default_params(t_max=0.025 * 45)
    assert L.qloco_nlp_tick_init(C.byref(long_step), C.byref(tp), 4, *init, None) == 100
    bad = nlp.default_params(dt=0.0)
    assert L.qloco_nlp_tick_init(C.byref(bad), C.byref(tp), 4, *init, None) == 100
    # nlp_ws, tick_ws, t_int, est, rfoot, lfoot, stop | com_traj, rlfoot, right_support, vari | optional
    args = [one] * 6 + [None] + [one] * 4 + [None] * 6
    assert L.qloco_nlp_tick(None, C.byref(tp), 4, *args, None) == 100
    assert L.qloco_nlp_tick(C.byref(p), None, 4, *args, None) == 100
    assert L.qloco_nlp_tick(C.byref(p), C.byref(tp), -1, *args, None) == 100
    assert L.qloco_nlp_tick(C.byref(long_step), C.byref(tp), 4, *args, None) == 100
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10):
        a = list(args)
        a[k] = None
        assert L.qloco_nlp_tick(C.byref(p), C.byref(tp), 4, *a, None) == 100, k
    assert L.qloco_nlp_tick_get_state(4, None, one, None) == 100 and L.qloco_nlp_tick_get_state(4, one, None, None) == 100
    assert L.qloco_nlp_tick_set_state(0, one, one, None) == 100 and L.qloco_nlp_tick_set_state(4, one, None, None) == 100
    assert L.qloco_nlp_tick_set_group_width(4) == 100
    prev = L.qloco_nlp_tick_set_group_width(8)
    assert prev in (1, 8) and L.qloco_nlp_tick_set_group_width(prev) == 8


def test_tick_kernels_are_spill_and_scratch_free():
    """Both forms of the new kernel (one robot per lane, one per 8-lane group):
    no spilled register, no private segment, no dynamic stack, at most 256
    registers (two waves per SIMD), no LDS."""
    import test_kernel_resources as Q
    ks = {n: k for n, k in Q._kernels().items() if "nlp_tick_kernel" in n}
    assert len(ks) == 2, sorted(ks)
    for n, k in ks.items():
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, n
        assert k.get(".sgpr_spill_count", 0) == 0, n
        assert not k.get(".uses_dynamic_stack", False), n
        assert k[".vgpr_count"] + k[".agpr_count"] <= 256, (n, k[".vgpr_count"], k[".agpr_count"])
        assert k[".group_segment_fixed_size"] == 0, n


def test_members_restatement():
    """_footz_ref, _lift_height_ref, _t_end_footstep and the initial arrays for
    the reference's own inputs (:67, :71-75, :176-180, :496-499, :593)."""
    st = K.TickState(2 * 0.12675, 0.02)
    assert st.t_end == 672 == R.t_end_footstep() and st.sw0 == 0.12675 and st.bjx1 == 0 and st.ry == 0.0
    assert list(st.lift) == [0.03] * 23 + [0.03, 0.015, 0.0, 0.0]
    assert st.footz_ref[0] == 0.0 and st.footz_ref[1] == 0.02 and abs(st.footz_ref[26] - 0.52) < 1e-15
    assert np.array_equal(st.tx0, R.Robot().tx)
    assert (st.ring == [0.0, -0.12675, 0.0, 0.0, 0.12675, 0.0]).all()
    rec = st.to_record()
    assert rec.shape == (374,) and np.array_equal(K.TickState().from_record(rec).to_record(), rec)
    # _Zsc: the step (k + 1) dt falls in under the initial schedule; 0 from _nsum - 1 on
    p = R.params()
    assert K._zsc(st, 26, p) == 0.0 and K._zsc(st, 27, p) == 0.02 and K._zsc(st, 55, p) == 0.04
    assert K._zsc(st, 726, p) == st.footz_ref[25] and K._zsc(st, 727, p) == 0.0


def test_linear_algebra_of_both_formulations():
    """The scalar LU inverse, LU solve and cofactor inverse against numpy on a
    well-conditioned system of each size."""
    rng = np.random.default_rng(5)
    for n in (4, 7):
        M = rng.normal(size=(n, n)) + n * np.eye(n)
        v = rng.normal(size=n)
        want = np.linalg.solve(M, v)
        assert np.allclose(K._matvec(K._lu_inverse(M.tolist()), list(v)), want, rtol=0, atol=1e-13)
        assert np.allclose(K._lu_solve(*K._lu(M.tolist()), list(v)), want, rtol=0, atol=1e-13)
    M = rng.normal(size=(4, 4)) + 4 * np.eye(4)
    assert np.allclose(K._cofactor_inverse4(M.tolist()), np.linalg.inv(M), rtol=0, atol=1e-13)
    # a pivot that is not on the diagonal
    M = np.array([[0.0, 2.0, 1.0, 0.5], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 3.0], [0.0, 1.0, 4.0, 0.0]])
    assert np.allclose(K._lu_inverse(M.tolist()), np.linalg.inv(M), rtol=0, atol=1e-14)
    assert K._powers(0.7, 3, K.B) == [0.7 * 0.7 * 0.7, 0.7 * 0.7, 0.7, 1.0]


# how often each branch must occur over cases 1-3 (tick x robot): 90 ticks cross three step boundaries
CENSUS_MIN = dict(init=26 * 85, ds=3 * 5 * 85 - 85, cubic=3000, snap=60, latch=2 * 85, right_swing=1000,
                  left_swing=1000, stop_lift0=9, stepped_max=20)


def test_formulations_take_the_same_branches_and_every_branch_occurs():
    count = collections.Counter()
    for name, _, free_only in K.cases()[:3]:
        for mode in K.MODES:
            a, b, d = K.pair(name, mode)                 # asserts branches_equal(a, b)
            assert K.branches_equal(a, b), (name, mode)
        a = K.rollout(name, K.A)
        assert (a["status"] == R.OK).all() and np.isfinite(a["com_traj"]).all() and np.isfinite(a["rlfoot"]).all(), name
        T, Bn = a["status"].shape
        for t in range(T):
            for r in range(Bn):
                br = a["branch"][t][r]
                count[br] += 1
                if br == "cubic":
                    even = a["sqp"]["sched"][t, r, 3] % 2 == 0
                    count["right_swing" if even else "left_swing"] += 1
                    assert a["right_support"][t, r] == (0 if even else 1)
                    if name == "stop" and a["lift_used"][t, r] == 0.0:
                        count["stop_lift0"] += 1
                    if name == "stepped":
                        fz, bj = a["rec2_out"][t, r][slice(*K.SLICES["footz_ref"])], a["sqp"]["sched"][t, r, 2]
                        count["stepped_max"] += fz[bj - 2] > fz[bj]          # a descending robot: max() picks bjxx - 2
                elif br in ("ds", "init"):
                    assert a["right_support"][t, r] == 2
        count["latch"] += int(a["latch"].sum())
        if name == "stepped":
            c = a["com_traj"]
            assert (np.abs(c[30:, :, 8]) > 1e-6).any() and (c[30:, :, 2] != K.TICK_DEFAULTS["hcom"]).any()
            assert (a["stepheight"] != 0).all() and (a["stepheight"] < 0).any()
        if name == "flat":
            assert np.abs(a["com_traj"][..., 2] - K.TICK_DEFAULTS["hcom"]).max() < 1e-12
            # both a right and a left swing run from lift-off to landing: the swing foot leaves the ground
            assert a["rlfoot"][..., 2].max() > 0.02 and a["rlfoot"][..., 5].max() > 0.02
    print("census:", dict(count))
    for k, n in CENSUS_MIN.items():
        assert count[k] >= n, (k, count[k], n)


def test_end_of_the_footstep_plan_restatement():
    """Case 4: three robots from tick 1 through _t_end_footstep + 3, free-running;
    the last three ticks take the hold branch."""
    a, b, d = K.pair("end", "free")
    T = a["status"].shape[0]
    assert T == R.t_end_footstep() + 3
    for r in range(3):
        assert [a["branch"][t][r] for t in range(T - 3, T)] == ["end"] * 3 and a["branch"][T - 4][r] != "end"
        assert (a["right_support"][T - 3:, r] == 2).all()
        assert np.array_equal(a["rlfoot"][T - 1, r, :6], a["rlfoot"][T - 4, r, :6])      # held
        assert not a["rlfoot"][T - 3:, r, 6:].any()
        assert not a["rec2_out"][T - 1, r][slice(*K.SLICES["lift"])][int(a["sqp"]["sched"][T - 1, r, 3]) + 1:].any()
    assert (a["status"] == R.OK).all()


def _reproduces(got, want, k, mode):
    assert (got == 0.0 and want == 0.0) or 0.5 * want <= got <= 2.0 * want, (mode, k, got, want)


def test_spreads_reproduce():
    """The figures tests/test_nlp_tick_gpu.py bounds the GPU with.  Of a key
    bounded per robot-tick (the 4 x 4 system at a condition number of 1e12 and
    more) only the median is a stable figure: its largest value is one
    formulation's noise."""
    for mode, committed in (("teacher", K.SPREAD_TEACHER), ("free", K.SPREAD_FREE)):
        m = K.pooled(mode)
        print(mode, "measured:", m)
        assert set(committed) == set(m), mode
        for k, (mx, med) in committed.items():
            per_tick = k in K.PER_TICK_KEYS and med > 0 and mx > K.OUTLIER * med
            assert per_tick == (k in K.PER_TICK_KEYS and m[k][1] > 0 and m[k][0] > K.OUTLIER * m[k][1]), (mode, k)
            _reproduces(m[k][1], med, k, mode)
            if not per_tick:
                _reproduces(m[k][0], mx, k, mode)
