"""The batched Go1 servo tick (csrc/qloco_go1_servo.hip, include/qloco.h section
16) -- CPU tests: the C ABI's symbols and host-side checks, the new kernels'
register and scratch figures, and the restatement (tests/go1_servo_ref.py):
its Butterworth filter, that every branch occurs over the GPU tests' inputs,
and that no Newton stop decision of Inverse_kinematics_g over those inputs
sits within rounding of its threshold, which is what lets the GPU tests demand
equal update counts on every leg-tick.

Parity of the restatement with the reference itself is unpinned.
"""
import collections
import ctypes as C
import math

import numpy as np

import go1_servo_ref as K
import oracle_lib as O
from quadrupedal_loco_amd import _lib, go1servo

SYMBOLS = ("qloco_go1_servo_params_default", "qloco_go1_servo_workspace_bytes",
           "qloco_go1_servo_init", "qloco_go1_servo_tick", "qloco_go1_servo_get_state",
           "qloco_go1_servo_set_state")


def test_section_16_symbols_and_bindings():
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    assert not _lib.missing_symbols()
    assert go1servo.STATE == K.STATE == 288
    assert C.sizeof(_lib.Go1ServoParams) == 8 * (9 + 12 + 15 * 6 + 6 + 8)
    assert C.sizeof(_lib.Go1ServoDiag) == 8 * 21 and len(_lib.GO1_SERVO_DIAG) == 21
    p = go1servo.default_params()
    for k, v in K.DEFAULTS.items():
        assert getattr(p, k) == v, k
    assert tuple(p.target_pos) == go1servo.TARGET_POS
    fp = _lib.ForceParams()
    L.qloco_force_params_default(C.byref(fp))
    assert all(getattr(p.force, k) == getattr(fp, k) for k, _ in _lib.ForceParams._fields_)
    # the host's filter coefficients are the restatement's, bit for bit
    for i, fc in enumerate(K.filter_cutoffs()):
        want = K.butter_coef(1 / 0.005, fc)
        got = tuple(getattr(p.filter[i], k) for k in ("b0", "b1", "b2", "a1", "a2", "a"))
        assert got == want, (i, got, want)
    # the record's fields tile it without a gap up to the zero tail
    edges = sorted(go1servo.STATE_FIELDS.values())
    assert edges[0][0] == 0 and all(a[1] == b[0] for a, b in zip(edges, edges[1:])) and edges[-1][1] == 281
    q = go1servo.default_params(**K.TEST_PARAMS)
    assert (q.stand_duration, q.t_walk_start, q.t_period) == (0.007, 0.1, 0.1)


def test_sections_5_and_7_are_as_they_were():
    L = _lib.lib()
    assert L.qloco_abi_version() == 1
    assert _lib.SIGNATURES["qloco_leg_fk"] == (C.c_int, [_lib.i64] + [_lib.vp] * 7)
    assert _lib.SIGNATURES["qloco_leg_ik"] == (C.c_int, [_lib.i64] + [_lib.vp] * 10)
    assert _lib.SIGNATURES["qloco_servo_force_block"] == (C.c_int, [C.POINTER(_lib.ForceParams), _lib.i64] + [_lib.vp] * 22)
    for s in ("qloco_leg_fk", "qloco_leg_ik", "qloco_servo_workspace_bytes", "qloco_servo_init",
              "qloco_servo_force_block"):
        assert hasattr(L, s), s
    al = lambda x: (x + 255) & ~255
    want = 6 * al(8 * 12 * 5) + 2 * al(8 * 6 * 5) + al(4 * 4 * 5) + 2 * al(4 * 5) + al(4 * (2 * 5 + 160))
    assert L.qloco_servo_workspace_bytes(5) == want


def test_argument_validation_without_device_work():
    L = _lib.lib()
    p = go1servo.default_params()
    one = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: every call below is refused
    assert L.qloco_go1_servo_workspace_bytes(-1) == -1 and L.qloco_go1_servo_workspace_bytes(0) == -1
    assert L.qloco_go1_servo_workspace_bytes(3) > 3 * 8 * go1servo.STATE
    assert L.qloco_go1_servo_init(None, 4, one, None) == 100
    assert L.qloco_go1_servo_init(C.byref(p), 0, one, None) == 100
    assert L.qloco_go1_servo_init(C.byref(p), 4, None, None) == 100
    assert L.qloco_go1_servo_init(C.byref(go1servo.default_params(dtx=0.0)), 4, one, None) == 100
    assert L.qloco_go1_servo_init(C.byref(go1servo.default_params(dt_mpc_slow=0.001)), 4, one, None) == 100
    # ws, n_count | q_mea, quat, gait, mode, y_offset, q_cmd, ctrl, tau, grf | diag, gait_data
    args = [one, 0] + [one] * 9 + [None, None]
    assert L.qloco_go1_servo_tick(None, 4, *args, None) == 100
    assert L.qloco_go1_servo_tick(C.byref(p), 0, *args, None) == 100
    assert L.qloco_go1_servo_tick(C.byref(p), -3, *args, None) == 100
    for k in [0] + list(range(2, 11)):
        a = list(args)
        a[k] = None
        assert L.qloco_go1_servo_tick(C.byref(p), 4, *a, None) == 100, k
    a = list(args)
    a[1] = -1
    assert L.qloco_go1_servo_tick(C.byref(p), 4, *a, None) == 100
    assert L.qloco_go1_servo_tick(C.byref(go1servo.default_params(stand_duration=0.0)), 4, *args, None) == 100
    assert L.qloco_go1_servo_get_state(4, None, one, None) == 100 and L.qloco_go1_servo_get_state(4, one, None, None) == 100
    assert L.qloco_go1_servo_set_state(0, one, one, None) == 100 and L.qloco_go1_servo_set_state(4, one, None, None) == 100


def test_go1_servo_kernels_are_spill_and_scratch_free():
    """Every kernel of the new unit: no spilled vector register, no private
    segment, no dynamic stack, no LDS; the tick kernel fits two waves per SIMD."""
    import test_kernel_resources as Q
    ks = {n: k for n, k in Q._kernels().items() if "go1servo" in n}
    names = ("go1_servo_kernelILb0E", "go1_servo_kernelILb1E", "go1_gait_data_kernel", "go1_state_kernelILb0E",
             "go1_state_kernelILb1E", "go1_init_kernel", "go1_init2_kernel")
    assert len(ks) == len(names), sorted(ks)
    for s in names:
        assert any(s in n for n in ks), s
    for n, k in ks.items():
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, n
        assert not k.get(".uses_dynamic_stack", False), n
        assert k[".vgpr_count"] + k[".agpr_count"] <= 256, (n, k[".vgpr_count"], k[".agpr_count"])
        assert k[".group_segment_fixed_size"] == 0, n


def test_butterworth_restatement():
    """Three first-order calls, then the biquad; unit DC gain; lfoot_des[2] at 10 Hz."""
    c3, c10 = K.butter_coef(200.0, 3.0), K.butter_coef(200.0, 10.0)
    f = K.Butter(c3)
    x, ys = 0.0, [0.3, -0.2, 0.7, 0.1, 0.5]
    for n, y in enumerate(ys[:3]):
        got = f.filter(y)
        assert got == x + c3[5] * (y - x) and f.i == n + 1
        x = got
    m = f.memory()
    got = f.filter(ys[3])
    assert got == c3[0] * ys[3] + c3[1] * m[0] + c3[2] * m[1] + c3[3] * m[2] + c3[4] * m[3]
    assert f.i == 3 and f.memory()[:4] == [ys[3], m[0], got, m[2]]
    for c in (c3, c10):
        g = K.Butter(c)
        for _ in range(5000):
            out = g.filter(1.0)
        assert abs(out - 1.0) <= 1e-12, out
        assert abs((c[0] + c[1] + c[2]) / (1.0 - c[3] - c[4]) - 1.0) <= 1e-12
    cut = K.filter_cutoffs()
    assert go1servo.FILTER_SLOTS[8] == 8 and cut[8] == 10.0        # lfoot_des[2]: LPF12
    assert cut[6] == cut[7] == 3.0 and cut[:6] == [3.0] * 6 and cut[9:] == [10.0] * 6
    rb = K.Robot()
    assert rb.filt[8].c == c10 and rb.filt[7].c == c3 and rb.n_t_int == 5 and rb.n_period == 140


def test_every_branch_occurs_over_the_gpu_tests_inputs():
    r = K.rollout()
    T, B = r["ik_updates"].shape[:2]
    assert (T, B) == (K.TICKS, K.BATCH) and int(r["homing"].sum()) == 8 and r["homing"][:8].all()
    count = collections.Counter(b for row in r["branch"] for b in row)
    print("census:", dict(count))
    for k in ("homing", "prewalk", "101", "102", "103a", "103b", "other"):
        assert count[k] >= 50, (k, count[k])
    rs = r["right_support"][8:]
    assert all((rs == v).sum() >= 500 for v in (0, 1, 2)) and (r["right_support"][:8] == -1).all()
    up = r["ik_updates"][8:]
    assert (up == 0).sum() >= 1000 and (up >= 1).sum() >= 1000 and up.max() <= 15
    # the robot outside the three modes keeps its targets and its flags
    other = [b for b in range(B) if r["branch"][-1][b] == "other"]
    assert other == [3]
    assert np.array_equal(r["foot_des"][-1, 3], r["foot_des"][7, 3]) and not r["swing"][:, 3].any()
    assert np.isfinite(r["tau"]).all() and np.isfinite(r["angle_des"]).all()
    # inputs as the GPU tests need them
    inp = K.inputs()
    assert np.abs(inp["q_mea"] - np.asarray(go1servo.TARGET_POS)).max() <= 0.15
    assert np.abs(np.linalg.norm(inp["quat"], axis=-1) - 1.0).max() <= 1e-15
    assert np.abs(r["body_r_est"][..., :2]).max() <= 0.3
    assert np.abs(inp["gait_msg"][..., 39:42]).max() <= 2.0 and inp["gait_msg"][..., [8, 11]].max() <= 0.05
    assert np.array_equal(inp["gait_msg"][0], inp["gait_msg"][4]) and not np.array_equal(inp["gait_msg"][4], inp["gait_msg"][5])
    sub = go1servo.synth_inputs(K.SEED, 3, 16)                      # a pure function of (seed, robot, tick)
    assert all(np.array_equal(sub[k], inp[k][:16, :3] if inp[k].ndim > 1 else inp[k][:3]) for k in sub)


def test_ik_stop_decisions_are_clear_of_rounding():
    """The replay of Inverse_kinematics_g's Newton loop over the oracle's FK
    takes qo_leg_ik's update count on every leg-tick (asserted inside the
    rollout), and no decision has | |det_pos|^2 - 1e-6 | < 1e-12: 500 x the
    2e-15 a 1e-12 m position difference can move the left side by."""
    r = K.rollout_with_ik_replay()
    assert np.array_equal(r["ik_updates"], K.rollout()["ik_updates"])
    assert np.array_equal(r["state_after"], K.rollout()["state_after"])
    m = r["ik_margin"][8:]
    print("smallest distance of |det_pos|^2 from 1e-6:", m.min())
    assert np.isfinite(m).all() and m.min() >= 1e-12, m.min()
    # the replay itself, on one leg: same angles as the oracle to rounding, same count
    q, n, ms = K.ik_replay([0.17, -0.13, 0.01], [0.0, 0.87, -1.5], 0, [0.0, 0.0, 0.3], [0.0, 0.05, 0.0])
    qo, _, _, no = O.leg_ik([0.17, -0.13, 0.01], [0.0, 0.87, -1.5], 0, [0.0, 0.0, 0.3], [0.0, 0.05, 0.0])
    assert n == no >= 1 and len(ms) == n + 1 and np.abs(np.array(q) - qo).max() <= 1e-12
    assert math.isinf(r["ik_margin"][:8].min())
