"""The slow planner's node tick (csrc/qloco_nlp_node.hip, include/qloco.h
section 17) -- CPU tests: the C ABI's symbols and host-side checks, the
restatement (tests/nlp_node_ref.py): its slot map, that every branch occurs on
the GPU tests' inputs, that its two formulations take the same branch on every
robot-tick and stay finite, the over-time stop, that the spreads the GPU
bounds are built from reproduce; the new kernels' register, scratch and LDS
figures.
"""
import collections
import ctypes as C

import numpy as np

import nlp_node_ref as N
import nlp_ref as R
from quadrupedal_loco_amd import _lib, nlp

SYMBOLS = ("qloco_nlp_node_params_default", "qloco_nlp_node_workspace_bytes", "qloco_nlp_node_init",
           "qloco_nlp_node_tick", "qloco_nlp_node_set_form", "qloco_nlp_node_get_state",
           "qloco_nlp_node_set_state")


def test_section_17_symbols_and_bindings():
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert nlp.NODE_STATE == N.STATE == 254 and nlp.NODE_RING == N.RING == 48
    assert nlp.NODE_STATE_FIELDS == N.SLICES
    assert nlp.NODE_BRANCHES == N.BRANCH_NAMES
    p = nlp.default_node_params()
    assert {k: getattr(p, k) for k in N.NODE_DEFAULTS} == N.NODE_DEFAULTS
    assert C.sizeof(_lib.NlpNodeParams) == 128
    assert L.qloco_nlp_node_workspace_bytes(3) == 3 * (254 + 94) * 8
    # sections 14 and 15 are as they were
    assert L.qloco_nlp_workspace_bytes(3) == 3 * 309 * 8 and L.qloco_nlp_tick_workspace_bytes(3) == 3 * (374 + 21) * 8


def test_argument_validation_without_device_work():
    L = _lib.lib()
    p, tp, npar = nlp.default_params(), nlp.default_tick_params(), nlp.default_node_params()
    one = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: every call below is refused
    assert L.qloco_nlp_node_workspace_bytes(0) == -1 and L.qloco_nlp_node_workspace_bytes(-3) == -1
    ok = (C.byref(p), C.byref(tp), C.byref(npar))
    init = [one] * 5 + [None]    # nlp_ws, tick_ws, node_ws, steplength, stepwidth, stepheight
    for k in range(3):
        a = list(ok)
        a[k] = None
        assert L.qloco_nlp_node_init(*a, 4, *init, None) == 100, k
        assert L.qloco_nlp_node_tick(*a, 4, *([one] * 5), None, None, None) == 100, k
    assert L.qloco_nlp_node_init(*ok, 0, *init, None) == 100
    for k in range(5):
        a = list(init)
        a[k] = None
        assert L.qloco_nlp_node_init(*ok, 4, *a, None) == 100, k
    for k in range(5):           # nlp_ws, tick_ws, node_ws, nrt_msg, gait_msg
        a = [one] * 5
        a[k] = None
        assert L.qloco_nlp_node_tick(*ok, 4, *a, None, None, None) == 100, k
    # _dtx has to be the planner's _dt; _nTdx has to fit the tail
    other = nlp.default_node_params(dtx=0.005)
    assert L.qloco_nlp_node_tick(C.byref(p), C.byref(tp), C.byref(other), 4, *([one] * 5), None, None, None) == 100
    slow = nlp.default_params(t_max=1.2)
    assert L.qloco_nlp_node_tick(C.byref(slow), C.byref(tp), C.byref(npar), 4, *([one] * 5), None, None, None) == 100
    assert L.qloco_nlp_node_get_state(4, None, one, None) == 100 and L.qloco_nlp_node_set_state(4, one, None, None) == 100
    assert L.qloco_nlp_node_set_form(2) == 100
    prev = L.qloco_nlp_node_set_form(1)
    assert prev in (0, 1) and L.qloco_nlp_node_set_form(prev) == 1


def test_slot_map_covers_the_row():
    """Every slot of the 100-vector is listed with its source; a slot whose
    source is zero for ever, and slot 98, is zero in every row."""
    assert sorted(N.SLOT_MAP) == list(range(100))
    assert len(N.ZERO_SLOTS) == 3 + 6 + 12 + 6 + 1 and 98 in N.ZERO_SLOTS
    computed = set(N.FORCE_SLOTS) | set(N.MOMENT_SLOTS) | {14, 27, 97, 99}
    assert set(N.COPY_SLOTS) | computed | set(N.ZERO_SLOTS) == set(range(100))
    assert not set(N.COPY_SLOTS) & (computed | set(N.ZERO_SLOTS))
    # the tick's outputs are each used at most once
    assert len(set(N.COPY_SLOTS.values())) == len(N.COPY_SLOTS)
    for name in N.CASES:
        a = N.rollout(name)
        assert not a["rows"][..., list(N.ZERO_SLOTS)].any(), name
    st = N.NodeState()
    assert st.row[2] == 0.309458 and st.row[7] == 0.12675 and st.row[10] == -0.12675 and st.row[99] == 2.0
    assert np.count_nonzero(st.row) == 4


def test_walkdtime_max_and_the_walking_offset():
    p, npar = R.params(), dict(N.NODE_DEFAULTS)
    assert N.nsum(p) == 728 and N.walkdtime_max(p, npar) == 672
    st = N.NodeState()
    assert N.pre(st, 0.0, p, npar) == (N.NOT_STARTED, 0, 0) and N.pre(st, -1.0, p, npar)[0] == N.NOT_STARTED
    assert st.count == 0
    for n in range(1, 41):
        assert N.pre(st, 1.0, p, npar) == (N.SQUAT, n, 0)
    assert N.pre(st, 1.0, p, npar) == (N.WALKING, 1, 1)         # _walkdtime1 -= 40.0
    assert N.pre(st, 0.0, p, npar) == (N.WALKING, 1, 1)         # the latch holds, the count does not advance


# how often each branch must occur over both cases (tick x robot)
CENSUS_MIN = dict(not_started=76, squat=40 * 76, walking=90 * 76, first_walking=76, b1=26 * 76, even_ds=300,
                  even_ss=1000, odd_ds=150, odd_ss=1000, tail=90 * 76, ahead3=200, ahead6=4)


def test_formulations_take_the_same_branches_and_every_branch_occurs():
    count = collections.Counter()
    for name in N.CASES:
        a, b, d = N.pair(name)
        assert N.branches_equal(a, b), name
        # a condition on the inputs, not a measurement
        assert np.isfinite(a["rows"]).all() and np.isfinite(b["rows"]).all(), name
        assert (a["status"] == R.OK).all(), name
        for k, v in zip(N.BRANCH_NAMES, np.bincount(a["branch"].ravel(), minlength=5)):
            count[k] += int(v)
        walking = a["branch"] == N.WALKING
        count["first_walking"] += int((walking & (a["w1"] == 1)).sum())
        for row in a["dist"]:
            count.update(x for x in row if x)
        count["tail"] += int((a["ntd"] > 3).sum())
        ahead = np.where(a["kend"] >= 0, a["kend"] - a["w1"], -1)
        assert ahead.max() <= 6
        count["ahead3"] += int((ahead > 2).sum())                # ZMP_end comes from the tail
        count["ahead6"] += int((ahead == 6).sum())
        assert a["branch"][0].tolist() == [N.NOT_STARTED] * a["branch"].shape[1]
        assert (a["branch"][1:N.LEAD] == N.SQUAT).all() and walking[N.LEAD:].all()
        # not started and squat rows: the hold forces, bjx1 = 1, double support
        hold = a["rows"][:N.LEAD]
        assert (hold[..., [17, 20]] == 9.8 / 2 * 12).all() and (hold[..., 27] == 1).all() and (hold[..., 99] == 2).all()
        assert not hold[..., [15, 16, 18, 19, 21, 22, 23, 24, 25, 26]].any()
        assert np.abs(hold[1:, :, 2] - 0.309458).max() < 1e-12  # _height_offset = 0: Z_C plus rounding noise
        # a walking row's forces carry the robot's weight between them
        fz = a["rows"][N.LEAD:, :, 17] + a["rows"][N.LEAD:, :, 20]
        assert np.abs(fz - 12 * (a["rows"][N.LEAD:, :, 41] + 9.8)).max() < 1e-9
    print("census:", dict(count))
    assert count["over_time"] == 0 and count["stopped"] == 0 and count["b0"] == 0
    for k, n in CENSUS_MIN.items():
        assert count[k] >= n, (k, count[k], n)


def test_over_time_stops_the_node():
    """_walkdtime_max is reached through a record with advanced counters: the
    row takes mpc_stop = 2 and right_support = 2 and is re-emitted unchanged."""
    p, tp, npar = R.params(), dict(N.K.TICK_DEFAULTS), dict(N.NODE_DEFAULTS)
    st = N.NodeState()
    st.latch, st.count = True, 40 + 670
    st.row[:] = np.arange(100) / 7.0
    st.row[97], st.row[99] = 0.0, 1.0
    assert N.pre(st, 1.0, p, npar) == (N.WALKING, 671, 671)     # the last walking tick
    before = st.row.copy()
    branch, w1, ti = N.pre(st, 1.0, p, npar)
    assert (branch, w1, ti) == (N.OVER_TIME, 672, 0)
    row, info = N.post(st, branch, w1, N.A, p, tp, npar)
    want = before.copy()
    want[97], want[98], want[99] = 2.0, 0.0, 2.0
    assert np.array_equal(row, want) and st.mpc_stop == 2.0 and st.restart == st.count == 712
    for _ in range(3):
        branch, w1, ti = N.pre(st, 1.0, p, npar)
        assert (branch, ti) == (N.STOPPED, 0)
        again, _ = N.post(st, branch, w1, N.A, p, tp, npar)
        assert np.array_equal(again, row)
    assert st.count == 715                                        # the loop keeps counting


def test_spreads_reproduce():
    """The figures tests/test_nlp_node_gpu.py bounds the GPU with."""
    m = N.pooled()
    print("measured:", m)
    assert set(m) == set(N.SPREAD) == set(N.KEYS)
    for k, want in N.SPREAD.items():
        assert want > 0 and 0.5 * want <= m[k] <= 2.0 * want, (k, m[k], want)
    own = np.array([0.0, 1.0])
    assert N.bound("force", own).tolist() == [16 * N.SPREAD["force"], 16.0]


def test_node_kernels_are_spill_and_scratch_free():
    """The pre-kernel and both forms of the post-kernel: no spilled vector
    register, no private segment, no dynamic stack; at most 256 registers in
    the post-kernel (two waves per SIMD); the LDS form's tile lets at least
    two workgroups share a CU's 160 KiB."""
    import test_kernel_resources as Q
    ks = {n: k for n, k in Q._kernels().items() if "nlp_node_" in n}
    post = [n for n in ks if "nlp_node_post_kernel" in n]
    assert len(post) == 2 and any("nlp_node_pre_kernel" in n for n in ks), sorted(ks)
    for n, k in ks.items():
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, n
        assert not k.get(".uses_dynamic_stack", False), n
        assert k[".vgpr_count"] + k[".agpr_count"] <= 256, (n, k[".vgpr_count"], k[".agpr_count"])
    lds = sorted(ks[n][".group_segment_fixed_size"] for n in post)
    assert lds[0] == 0 and lds[1] == 16 * 100 * 8 and 2 * lds[1] <= 160 * 1024, lds
