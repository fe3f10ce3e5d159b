"""ctypes binding of libqloco.so (the C ABI in include/qloco.h).

The product path has no CPU fallback: if the HIP library is missing or no
gfx950 device is visible, calls raise instead of computing anything on the
host.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# QLOCO_LIB: an experimental build of the same library (tools/variant_lib.py)
# for A/B timing runs; unset, the in-tree product library
LIB_PATH = os.environ.get("QLOCO_LIB") or os.path.join(HERE, "lib", "libqloco.so")

_lib = None


class SrbdSpec(C.Structure):
    """Mirror of `qloco_srbd_spec` (include/qloco.h)."""
    _fields_ = [
        ("horizon", C.c_int32), ("feet_per_step", C.c_int32),
        ("contacts_per_step", C.c_int32), ("output_frame", C.c_int32),
        ("dt", C.c_float), ("mass", C.c_float), ("inertia", C.c_float * 9),
        ("q_weights", C.c_float * 13), ("r_weights", C.c_float * 12),
        ("mu", C.c_float), ("fz_min", C.c_float), ("fz_max", C.c_float),
        ("rho", C.c_float), ("sigma", C.c_float), ("alpha", C.c_float),
        ("eps_abs", C.c_float), ("eps_rel", C.c_float),
        ("max_iter", C.c_int32), ("check_termination", C.c_int32), ("scaling", C.c_int32),
        ("adaptive_rho", C.c_int32), ("adaptive_rho_interval", C.c_int32),
        ("adaptive_rho_tolerance", C.c_float), ("warm_start", C.c_int32),
        ("polish", C.c_int32), ("literal_full_qp", C.c_int32), ("reserved", C.c_int32 * 5),
    ]


class SrbdModel(C.Structure):
    """Mirror of `qloco_srbd_model`: one robot's body, 64 bytes."""
    _fields_ = [("mass", C.c_float), ("inertia", C.c_float * 9), ("mu", C.c_float),
                ("fz_min", C.c_float), ("fz_max", C.c_float), ("reserved", C.c_float * 3)]


class ForceParams(C.Structure):
    """Mirror of `qloco_force_params`."""
    _fields_ = [(k, C.c_double) for k in ("mass", "alpha", "beta", "gamma", "fz_max", "mu")]


class ForceBody(C.Structure):
    """Mirror of `qloco_force_body`: one robot's body for the Go1 force QP and
    the servo ticks, 128 bytes (the six `qloco_force_params`, Momentum_sum
    row-major, one reserved zero)."""
    _fields_ = ForceParams._fields_ + [("momentum", C.c_double * 9), ("reserved", C.c_double * 1)]


class A1Params(C.Structure):
    """Mirror of `qloco_a1_params`."""
    _fields_ = [("kp_linear", C.c_double * 3), ("kd_linear", C.c_double * 3),
                ("kp_angular", C.c_double * 3), ("kd_angular", C.c_double * 3),
                ("robot_mass", C.c_double), ("q_diag", C.c_double * 6), ("r", C.c_double),
                ("mu", C.c_double), ("f_min", C.c_double), ("f_max", C.c_double),
                ("rho", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double),
                ("eps_abs", C.c_double), ("eps_rel", C.c_double),
                ("adaptive_rho_tolerance", C.c_double),
                ("max_iter", C.c_int32), ("check_termination", C.c_int32),
                ("scaling", C.c_int32), ("adaptive_rho", C.c_int32),
                ("adaptive_rho_interval", C.c_int32), ("reserved", C.c_int32 * 3)]


class A1Body(C.Structure):
    """Mirror of `qloco_a1_body`: one robot's body and gains, 192 bytes (the
    first 23 doubles of `qloco_a1_params` and one pad)."""
    _fields_ = A1Params._fields_[:10] + [("reserved", C.c_double)]


class A1KinParams(C.Structure):
    """Mirror of `qloco_a1_kin_params`."""
    _fields_ = [("rho_fix", (C.c_double * 5) * 4), ("rho_opt", (C.c_double * 3) * 4)]


class A1EkfParams(C.Structure):
    """Mirror of `qloco_a1_ekf_params`."""
    _fields_ = [("process_noise_pimu", C.c_double), ("process_noise_vimu", C.c_double),
                ("process_noise_pfoot", C.c_double), ("sensor_noise_pimu_rel_foot", C.c_double),
                ("sensor_noise_vimu_rel_foot", C.c_double), ("sensor_noise_zfoot", C.c_double),
                ("assume_flat_ground", C.c_int32), ("reserved", C.c_int32 * 7)]


class A1CtrlParams(C.Structure):
    """Mirror of `qloco_a1_ctrl_params`."""
    _fields_ = [("counter_per_gait", C.c_double), ("counter_per_swing", C.c_double),
                ("gait_counter_speed", C.c_double * 4), ("gait_counter_reset", C.c_double * 4),
                ("default_foot_pos", C.c_double * 12), ("control_dt", C.c_double),
                ("kp_foot", C.c_double * 12), ("kd_foot", C.c_double * 12),
                ("km_foot", C.c_double * 3), ("torques_gravity", C.c_double * 12),
                ("foot_delta_x_limit", C.c_double), ("foot_delta_y_limit", C.c_double),
                ("foot_force_low", C.c_double), ("foot_swing_clearance1", C.c_double),
                ("foot_swing_clearance2", C.c_double), ("recent_contact_window", C.c_int32),
                ("terrain_window", C.c_int32), ("torque_holdoff_ticks", C.c_int32),
                ("reserved", C.c_int32 * 5)]


class NlpParams(C.Structure):
    """Mirror of `qloco_nlp_params`."""
    _fields_ = [(k, C.c_double) for k in (
        "dt", "tstep", "t_min", "t_max", "footx_vmax", "footx_vmin", "footy_vmax", "footy_vmin",
        "comax_max", "comax_min", "comay_max", "comay_min", "aax", "aay", "aaxv", "aayv", "bbx", "bby",
        "rr1", "rr2", "footx_max", "footx_min", "z_c", "g", "half_hip_width", "foot_width",
        "lamda_comx", "lamda_comvx", "lamda_comy", "lamda_comvy")] + [("reserved", C.c_double * 2)]


class NlpTickParams(C.Structure):
    """Mirror of `qloco_nlp_tick_params`."""
    _fields_ = [("lift_height", C.c_double), ("hcom", C.c_double), ("reserved", C.c_double * 6)]


class NlpNodeParams(C.Structure):
    """Mirror of `qloco_nlp_node_params`."""
    _fields_ = [(k, C.c_double) for k in ("dtx", "height_offset_time", "height_squat_time", "height_offset",
                                          "height_offsetx", "totalmass", "rad")] + [("reserved", C.c_double * 9)]


class ButterCoef(C.Structure):
    """Mirror of `qloco_butter_coef`."""
    _fields_ = [(k, C.c_double) for k in ("b0", "b1", "b2", "a1", "a2", "a")]


class Go1ServoParams(C.Structure):
    """Mirror of `qloco_go1_servo_params`."""
    _fields_ = [(k, C.c_double) for k in (
        "rt_frequency", "stand_duration", "dtx", "dt_mpc_slow", "t_period", "t_walk_start", "pi",
        "half_hip_width", "z_c")] + [("target_pos", C.c_double * 12), ("filter", ButterCoef * 15),
                                     ("force", ForceParams), ("reserved", C.c_double * 8)]


GO1_SERVO_DIAG = (("body_r_est", 3, "f8"), ("foot_rel_mea", 12, "f8"), ("v_est_rel", 12, "f8"),
                  ("Jaco_est", 36, "f8"), ("com_des", 3, "f8"), ("rfoot_des", 3, "f8"),
                  ("lfoot_des", 3, "f8"), ("coma_des", 3, "f8"), ("thetaacc_des", 3, "f8"),
                  ("comv_des", 3, "f8"), ("body_p_des", 3, "f8"), ("body_r_des", 3, "f8"),
                  ("foot_des", 12, "f8"), ("angle_des", 12, "f8"), ("Jaco", 36, "f8"),
                  ("ik_updates", 4, "i4"), ("F_sum", 6, "f8"), ("Force_L_R", 6, "f8"),
                  ("swing", 4, "i4"), ("qp_solution", 1, "i4"), ("status", 1, "i4"))


class Go1ServoDiag(C.Structure):
    """Mirror of `qloco_go1_servo_diag`: one device pointer per member."""
    _fields_ = [(k, C.c_void_p) for k, _, _ in GO1_SERVO_DIAG]


vp = C.c_void_p
i64 = C.c_int64
i32 = C.c_int32

# name -> (restype, argtypes); every symbol include/qloco.h declares
SIGNATURES = {
    "qloco_status_string": (C.c_char_p, [C.c_int]),
    "qloco_abi_version": (C.c_int, []),
    "qloco_last_error": (C.c_char_p, []),
    "qloco_srbd_spec_default": (None, [C.POINTER(SrbdSpec)]),
    "qloco_srbd_max_stance_vars": (C.c_int, []),
    "qloco_srbd_route": (C.c_int, [C.POINTER(SrbdSpec)]),
    "qloco_srbd_lit_tables": (C.c_int, [C.POINTER(SrbdSpec), vp, i64, vp, vp, vp]),
    "qloco_srbd_solve": (C.c_int, [C.POINTER(SrbdSpec), i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                   vp, vp, vp]),
    "qloco_srbd_solve_ex": (C.c_int, [C.POINTER(SrbdSpec), i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                      vp, vp, vp, i32, vp]),
    "qloco_srbd_solve_placed": (C.c_int, [C.POINTER(SrbdSpec), i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                          vp, vp, vp, i32, vp, vp]),
    "qloco_srbd_model_from_spec": (C.c_int, [C.POINTER(SrbdSpec), i64, C.POINTER(SrbdModel)]),
    "qloco_srbd_solve_model": (C.c_int, [C.POINTER(SrbdSpec), i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                         vp, vp, vp, i32, vp, vp, vp]),
    "qloco_srbd_build_model": (C.c_int, [C.POINTER(SrbdSpec), i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                         vp, vp, vp, vp]),
    "qloco_srbd_place_bytes": (i64, [i64]),
    "qloco_srbd_place_order_host": (C.c_int, [i64, i64, i32, vp, vp]),
    "qloco_srbd_place_assign_host": (C.c_int, [i64, i64, vp]),
    "qloco_srbd_build": (C.c_int, [C.POINTER(SrbdSpec), i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                   vp, vp, vp]),
    "qloco_gen_srbd_host": (C.c_int, [C.c_uint64, i32, C.c_float, i32, i64, i64, vp, vp, vp,
                                      vp]),
    "qloco_gen_srbd_host_strided": (C.c_int, [C.c_uint64, i32, C.c_float, i32, i64, i64, i64, vp,
                                              vp, vp, vp]),
    "qloco_eiquadprog_solve": (C.c_int, [i32, i32, i32, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                         vp, i64, vp, i64, vp, vp, vp, vp, vp]),
    "qloco_max_gi_vars": (C.c_int, []),
    "qloco_gi_limits": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "qloco_gi_fast_limits": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "qloco_srbd_scratch_sets": (C.c_int, [C.c_void_p]),
    "qloco_force_params_default": (None, [C.POINTER(ForceParams)]),
    "qloco_force_qp_solve": (C.c_int, [C.POINTER(ForceParams), i64] + [vp] * 18),
    "qloco_force_qp_solve_ordered": (C.c_int, [C.POINTER(ForceParams), i64] + [vp] * 19),
    "qloco_force_order_ws_len": (i64, [i64]),
    "qloco_force_body_from_params": (C.c_int, [C.POINTER(ForceParams), i64, C.POINTER(ForceBody)]),
    "qloco_force_body_check": (C.c_int, [C.POINTER(ForceBody)]),
    "qloco_force_qp_solve_body": (C.c_int, [C.POINTER(ForceParams), i64] + [vp] * 20),
    "qloco_leg_fk": (C.c_int, [i64] + [vp] * 7),
    "qloco_leg_ik": (C.c_int, [i64] + [vp] * 10),
    "qloco_joint_torques": (C.c_int, [i64] + [vp] * 9),
    "qloco_force_params_hw": (None, [C.POINTER(ForceParams)]),
    "qloco_force_set_group_width": (C.c_int, [C.c_int]),
    "qloco_hw_torque_ff": (C.c_int, [i64] + [vp] * 6),
    "qloco_body_state_init_host": (C.c_int, [i64, vp]),
    "qloco_body_mpc_step": (C.c_int, [i64] + [vp] * 10),
    "qloco_body_indexfind": (C.c_int, [i64, vp, vp, vp]),
    "qloco_rt_workspace_bytes": (C.c_int64, [i64]),
    "qloco_rt_init": (C.c_int, [i64, vp, vp]),
    "qloco_rt_tick": (C.c_int, [i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "qloco_servo_workspace_bytes": (C.c_int64, [i64]),
    "qloco_servo_init": (C.c_int, [i64, vp, vp]),
    "qloco_servo_force_block": (C.c_int, [C.POINTER(ForceParams), i64] + [vp] * 22),
    "qloco_servo_force_block_body": (C.c_int, [C.POINTER(ForceParams), i64] + [vp] * 23),
    "qloco_support_phase": (C.c_int, [i64] + [vp] * 8),
    "qloco_a1_params_default": (None, [C.POINTER(A1Params)]),
    "qloco_a1_params_check": (C.c_int, [C.POINTER(A1Params)]),
    "qloco_a1_qp_solve": (C.c_int, [C.POINTER(A1Params), i64] + [vp] * 9),
    "qloco_a1_body_from_params": (C.c_int, [C.POINTER(A1Params), i64, C.POINTER(A1Body)]),
    "qloco_a1_body_check": (C.c_int, [C.POINTER(A1Body)]),
    "qloco_a1_qp_solve_body": (C.c_int, [C.POINTER(A1Params), i64] + [vp] * 10),
    "qloco_a1_kin_params_default": (None, [C.POINTER(A1KinParams)]),
    "qloco_a1_leg_kin": (C.c_int, [C.POINTER(A1KinParams), i64] + [vp] * 16),
    "qloco_a1_ekf_params_default": (None, [C.POINTER(A1EkfParams)]),
    "qloco_a1_ekf_workspace_bytes": (C.c_int64, [i64]),
    "qloco_a1_ekf_init": (C.c_int, [C.POINTER(A1EkfParams), i64, vp, vp, vp, vp]),
    "qloco_a1_ekf_update": (C.c_int, [C.POINTER(A1EkfParams), i64] + [vp] * 13),
    "qloco_a1_ekf_get_state": (C.c_int, [i64, vp, vp, vp, vp]),
    "qloco_a1_ekf_set_state": (C.c_int, [i64, vp, vp, vp, vp]),
    "qloco_a1_ctrl_params_default": (None, [C.POINTER(A1CtrlParams)]),
    "qloco_a1_ctrl_workspace_bytes": (C.c_int64, [i64]),
    "qloco_a1_ctrl_reset": (C.c_int, [C.POINTER(A1CtrlParams), i64, vp, vp]),
    "qloco_a1_ctrl_plan_swing": (C.c_int, [C.POINTER(A1CtrlParams), i64] + [vp] * 21),
    "qloco_a1_ctrl_terrain": (C.c_int, [C.POINTER(A1CtrlParams), i64] + [vp] * 6),
    "qloco_a1_ctrl_joint_torques": (C.c_int, [C.POINTER(A1CtrlParams), i64] + [vp] * 5),
    "qloco_a1_ctrl_get_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_a1_ctrl_set_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_nlp_params_default": (None, [C.POINTER(NlpParams)]),
    "qloco_nlp_workspace_bytes": (C.c_int64, [i64]),
    "qloco_nlp_init": (C.c_int, [C.POINTER(NlpParams), i64] + [vp] * 5),
    "qloco_nlp_step_timing": (C.c_int, [C.POINTER(NlpParams), i64] + [vp] * 13),
    "qloco_nlp_get_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_nlp_set_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_nlp_set_group_width": (C.c_int, [C.c_int]),
    "qloco_nlp_tick_params_default": (None, [C.POINTER(NlpTickParams)]),
    "qloco_nlp_tick_workspace_bytes": (C.c_int64, [i64]),
    "qloco_nlp_tick_init": (C.c_int, [C.POINTER(NlpParams), C.POINTER(NlpTickParams), i64] + [vp] * 6),
    "qloco_nlp_tick": (C.c_int, [C.POINTER(NlpParams), C.POINTER(NlpTickParams), i64] + [vp] * 18),
    "qloco_nlp_tick_set_group_width": (C.c_int, [C.c_int]),
    "qloco_nlp_tick_get_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_nlp_tick_set_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_nlp_node_params_default": (None, [C.POINTER(NlpNodeParams)]),
    "qloco_nlp_node_workspace_bytes": (C.c_int64, [i64]),
    "qloco_nlp_node_init": (C.c_int, [C.POINTER(NlpParams), C.POINTER(NlpTickParams), C.POINTER(NlpNodeParams),
                                      i64] + [vp] * 7),
    "qloco_nlp_node_tick": (C.c_int, [C.POINTER(NlpParams), C.POINTER(NlpTickParams), C.POINTER(NlpNodeParams),
                                      i64] + [vp] * 8),
    "qloco_nlp_node_set_form": (C.c_int, [C.c_int]),
    "qloco_nlp_node_get_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_nlp_node_set_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_go1_servo_params_default": (None, [C.POINTER(Go1ServoParams)]),
    "qloco_go1_servo_workspace_bytes": (C.c_int64, [i64]),
    "qloco_go1_servo_init": (C.c_int, [C.POINTER(Go1ServoParams), i64, vp, vp]),
    "qloco_go1_servo_tick": (C.c_int, [C.POINTER(Go1ServoParams), i64, vp, i64] + [vp] * 9 +
                             [C.POINTER(Go1ServoDiag), vp, vp]),
    "qloco_go1_servo_tick_body": (C.c_int, [C.POINTER(Go1ServoParams), i64, vp, i64] + [vp] * 9 +
                                  [C.POINTER(Go1ServoDiag), vp, vp, vp]),
    "qloco_go1_servo_get_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_go1_servo_set_state": (C.c_int, [i64, vp, vp, vp]),
    "qloco_mgpu_shard": (C.c_int, [i64, i32, i32, i32, vp, vp, vp]),
    "qloco_mgpu_gather_rows": (C.c_int, [i64, i32, i32, vp]),
    "qloco_mgpu_reorder": (C.c_int, [i64, i32, i32, i32, vp, vp, vp, vp, vp]),
    "qloco_mgpu_unique_id": (C.c_int, [vp]),
    "qloco_mgpu_init": (C.c_int, [vp, vp, i32, i32, i64, i32]),
    "qloco_mgpu_info": (C.c_int, [vp, vp, vp, vp, vp]),
    "qloco_mgpu_solve": (C.c_int, [vp, C.POINTER(SrbdSpec), vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
    "qloco_mgpu_solve_model": (C.c_int, [vp, C.POINTER(SrbdSpec), vp, vp, vp, vp, vp, vp, vp, vp, i32, vp,
                                         vp]),
    "qloco_mgpu_destroy": (C.c_int, [vp]),
}


class QlocoError(RuntimeError):
    pass


def lib():
    """Load libqloco.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QlocoError(
                "libqloco.so not built (%s); run `python -m quadrupedal_loco_amd.build` "
                "or __graft_entry__.build()" % LIB_PATH)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            if not hasattr(L, name):
                continue  # reported by missing_symbols()
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def missing_symbols():
    L = lib()
    return [n for n in SIGNATURES if not hasattr(L, n)]


def check(status, what):
    if status != 0:
        L = lib()
        msg = L.qloco_status_string(status).decode()
        err = L.qloco_last_error().decode()
        raise QlocoError("%s failed: %s %s" % (what, msg, err))


def ptr(t):
    """Device (or host) address of a torch tensor / numpy array, or None."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)
