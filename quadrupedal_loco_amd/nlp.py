"""Batched step-timing SQP of the slow gait planner (fp64) on gfx950.

Python mirror of NLPClass::step_timing_opti_loop of the Go1 planner node
(unitree_ros/mosek_nlp_kmp/src/NLP/NLPClass_sqp.cpp:693-1102): per 40 Hz tick
and robot, three SQP passes over a QP with 4 variables (next step length and
width, cosh / sinh of the remaining step time), 1 equality and 24
inequalities, then the _ts / _tx / foot-location / CoM boundary-state updates
and the LIP CoM at i, i + 1, i + 2 -- `qloco_nlp_step_timing`, one fused
kernel (csrc/qloco_nlp.hip).  There is no host fallback.

Every robot's members live in a device workspace.  `ts` and `tx` are (B, 27)
views of it in the layout `qloco_support_phase` takes, so

    out = planner.tick(t_int, est, rfoot, lfoot)
    rt.support_phase(planner.ts, planner.tx, t_int, t_end)

chains on one stream with no copy.  `StepTimingPlanner` does not compute
CoM_height_solve (and with it _comz, ZMP, DCM) or the foot trajectories;
`PlannerTick` (`qloco_nlp_tick`, csrc/qloco_nlp_tick.hip) runs the same SQP
kernel and adds them: the full 38-vector of step_timing_opti_loop and the
18-vector and support flag of Foot_trajectory_solve_mod2.  `PlannerNode`
(`qloco_nlp_node_tick`, csrc/qloco_nlp_node.hip) wraps that tick in the node
loop: the /rt2nrt/state row in, the /MPC/Gait row out, so that

    gait_msg = node.tick(nrt_msg).gait_msg
    traj_msg, nrt_msg, *_ = rt_node.tick(gait_msg, ctrl_msg)

closes the planner - rt loop on the device.  KMP is not computed.
"""
import ctypes as C
from dataclasses import dataclass

from ._lib import NlpNodeParams, NlpParams, NlpTickParams, check, lib, ptr
from .a1est import _dev

NS = 27               # QLOCO_NLP_STEPS
STATE = 309           # QLOCO_NLP_STATE
SKIPPED, FINISHED = -1, -2   # QLOCO_NLP_SKIPPED, QLOCO_NLP_FINISHED
STATE_FIELDS = dict(  # slices of the dense record get_state / set_state use
    ts=(0, 27), tx=(27, 54), td=(54, 81), Lxx_ref=(81, 108), Lyy_ref=(108, 135), footx_ref=(135, 162),
    footy_ref=(162, 189), COMx_is=(189, 216), COMvx_is=(216, 243), COMy_is=(243, 270),
    COMvy_is=(270, 297), vari=(297, 301), feed=(301, 307), endref=(307, 309))


def _defaults(struct, fill, overrides):
    """The library's default parameter struct (qloco_<fill>) with overrides."""
    p = struct()
    getattr(lib(), "qloco_" + fill)(C.byref(p))
    for k, v in overrides.items():
        if k == "reserved" or not hasattr(p, k):
            raise ValueError("unknown parameter %s" % k)
        setattr(p, k, v)
    return p


def _workspace(sizer, batch, device):
    """A zeroed float64 workspace of qloco_<sizer>(batch) bytes."""
    import torch
    nbytes = getattr(lib(), "qloco_" + sizer)(int(batch))
    if nbytes <= 0:
        raise ValueError("qloco_%s(%d) = %d" % (sizer, batch, nbytes))
    return torch.zeros(nbytes // 8, dtype=torch.float64, device=torch.device(device))


def default_params(**overrides):
    """NLPClass.h:32-37, the "go1" branch of Initialize and the constants
    NLPRTControlClass.cpp:33-56 passes."""
    return _defaults(NlpParams, "nlp_params_default", overrides)


@dataclass
class StepTimingResult:
    vari_ini: object      # (B, 4): Lxx, Lyy, tr1, tr2 after the three passes
    sched: object         # (B, 4) int32: _periond_i, _k_yu, _bjxx, _bjx1
    step: object          # (B, 3): _ts, _Lxx_ref, _Lyy_ref of step _periond_i - 1
    com: object           # (B, 18): i, i+1, i+2 x (comx, comy, comvx, comvy, comax, comay)
    pass_status: object   # (B, 3) int32: EiQuadProg outcome per pass, or SKIPPED
    pass_iters: object    # (B, 3) int32
    status: object        # (B,) int32: 0, QLOCO_NAN (3), QLOCO_BAD_SIZE (4) or FINISHED


class StepTimingPlanner:
    """Batched drop-in for NLPClass's step-timing optimisation: one set of
    members per robot, resident on the device."""

    def __init__(self, batch, device, params=None, steplength=0.075, stepwidth=None, **overrides):
        import torch
        if batch < 1:
            raise ValueError("batch < 1")
        self.batch = int(batch)
        self.device = torch.device(device)
        self.params = params if params is not None else default_params(**overrides)
        self.workspace = _workspace("nlp_workspace_bytes", self.batch, self.device)
        B = self.batch
        self.ts = self.workspace[:B * NS].view(B, NS)            # _ts, a row per robot
        self.tx = self.workspace[B * NS:2 * B * NS].view(B, NS)  # _tx
        if stepwidth is None:
            stepwidth = 2 * self.params.half_hip_width
        self.init(steplength, stepwidth)

    def _stream(self, stream):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream
                          if stream is None else stream)

    def _f64(self, *shape):
        import torch
        return torch.empty(shape, dtype=torch.float64, device=self.device)

    def _i32(self, *shape):
        import torch
        return torch.empty(shape, dtype=torch.int32, device=self.device)

    def _step_timing_result(self):
        B = self.batch
        return StepTimingResult(self._f64(B, 4), self._i32(B, 4), self._f64(B, 3), self._f64(B, 18), self._i32(B, 3),
                                self._i32(B, 3), self._i32(B))

    def _record(self, fn, workspace, state, stream):
        """qloco_nlp*_get_state / _set_state: `state` is the dense (B, n) record."""
        check(getattr(lib(), fn)(self.batch, ptr(workspace), ptr(state), self._stream(stream)), fn)
        return state

    def _per_robot(self, v, name):
        import torch
        if not torch.is_tensor(v):
            v = torch.as_tensor(v, dtype=torch.float64).expand(self.batch).contiguous().to(self.device)
        return _dev(v, "f64", (self.batch,), name)

    def init(self, steplength, stepwidth, stream=None):
        """FootStepInputs + Initialize: scalars or per-robot (B,) values."""
        sl = self._per_robot(steplength, "steplength")
        sw = self._per_robot(stepwidth, "stepwidth")
        check(lib().qloco_nlp_init(C.byref(self.params), self.batch, ptr(self.workspace), ptr(sl), ptr(sw),
                                   None, self._stream(stream)), "qloco_nlp_init")

    def tick(self, t_int, estimated_state, rfoot_feedback, lfoot_feedback, out=None, stream=None):
        """One planner tick: t_int (B,) int32, estimated_state (B, 6),
        rfoot_feedback / lfoot_feedback (B, 2), device tensors."""
        B = self.batch
        _dev(t_int, "i32", (B,), "t_int")
        _dev(estimated_state, "f64", (B, 6), "estimated_state")
        _dev(rfoot_feedback, "f64", (B, 2), "rfoot_feedback")
        _dev(lfoot_feedback, "f64", (B, 2), "lfoot_feedback")
        if out is None:
            out = self._step_timing_result()
        check(lib().qloco_nlp_step_timing(
            C.byref(self.params), B, ptr(self.workspace), ptr(t_int), ptr(estimated_state),
            ptr(rfoot_feedback), ptr(lfoot_feedback), ptr(out.vari_ini), ptr(out.sched), ptr(out.step),
            ptr(out.com), ptr(out.pass_status), ptr(out.pass_iters), ptr(out.status),
            self._stream(stream)), "qloco_nlp_step_timing")
        return out

    def get_state(self, stream=None):
        """Dense (B, 309) record per robot (STATE_FIELDS)."""
        return self._record("qloco_nlp_get_state", self.workspace, self._f64(self.batch, STATE), stream)

    def set_state(self, state, stream=None):
        self._record("qloco_nlp_set_state", self.workspace, _dev(state, "f64", (self.batch, STATE), "state"), stream)


TICK_STATE = 374      # QLOCO_NLP_TICK_STATE
TICK_RING = 48        # QLOCO_NLP_TICK_RING
TICK_STATE_FIELDS = dict(  # slices of the dense record of the second workspace
    bjx1=(0, 1), ry=(1, 2), t_end=(2, 3), sw0=(3, 4), last=(4, 5), footz_ref=(5, 32), lift=(32, 59),
    tx0=(59, 86), ring=(86, 374))


def default_tick_params(**overrides):
    """_lift_height (NLPRTControlClass.cpp:48) and _hcom (NLPClass_sqp.cpp:212)."""
    return _defaults(NlpTickParams, "nlp_tick_params_default", overrides)


@dataclass
class PlannerTickResult:
    com_traj: object       # (B, 38): step_timing_opti_loop's return value, every slot
    rlfoot_traj: object    # (B, 18): Foot_trajectory_solve_mod2's return value
    right_support: object  # (B,) int32: 0 left support, 1 right support, 2 double support
    status: object         # (B,) int32
    step_timing: object    # StepTimingResult of the same tick (its status is `status`)


class PlannerTick(StepTimingPlanner):
    """Batched drop-in for one NLPClass tick up to the class boundary:
    step_timing_opti_loop followed by Foot_trajectory_solve_mod2.  The SQP's
    record (`get_state`) and kernel are StepTimingPlanner's; the members it
    lacks live in a second workspace (`get_tick_state`)."""

    def __init__(self, batch, device, params=None, tick_params=None, steplength=0.075, stepwidth=None,
                 stepheight=None, **overrides):
        self.tick_params = tick_params if tick_params is not None else default_tick_params()
        self.tick_workspace = _workspace("nlp_tick_workspace_bytes", batch, device)
        self._stepheight = stepheight
        super().__init__(batch, device, params=params, steplength=steplength, stepwidth=stepwidth, **overrides)

    def init(self, steplength, stepwidth, stepheight=None, stream=None):
        """FootStepInputs + Initialize of both records: scalars or per-robot
        (B,) values; stepheight None is flat ground."""
        sl, sw, sh = self._step_inputs(steplength, stepwidth, stepheight)
        check(lib().qloco_nlp_tick_init(C.byref(self.params), C.byref(self.tick_params), self.batch,
                                        ptr(self.workspace), ptr(self.tick_workspace), ptr(sl), ptr(sw),
                                        None if sh is None else ptr(sh), self._stream(stream)),
              "qloco_nlp_tick_init")

    def _step_inputs(self, steplength, stepwidth, stepheight):
        if stepheight is None:
            stepheight = self._stepheight
        return (self._per_robot(steplength, "steplength"), self._per_robot(stepwidth, "stepwidth"),
                None if stepheight is None else self._per_robot(stepheight, "stepheight"))

    def step_timing_tick(self, t_int, estimated_state, rfoot_feedback, lfoot_feedback, out=None, stream=None):
        """The SQP alone (StepTimingPlanner.tick): the second record is not advanced."""
        return super().tick(t_int, estimated_state, rfoot_feedback, lfoot_feedback, out=out, stream=stream)

    def tick(self, t_int, estimated_state, rfoot_feedback, lfoot_feedback, stop_walking=None, out=None,
             stream=None):
        """One planner tick: the inputs of StepTimingPlanner.tick and an
        optional stop_walking (B,) int32.  out: a PlannerTickResult of an
        earlier call to write into."""
        B = self.batch
        _dev(t_int, "i32", (B,), "t_int")
        _dev(estimated_state, "f64", (B, 6), "estimated_state")
        _dev(rfoot_feedback, "f64", (B, 2), "rfoot_feedback")
        _dev(lfoot_feedback, "f64", (B, 2), "lfoot_feedback")
        if stop_walking is not None:
            _dev(stop_walking, "i32", (B,), "stop_walking")
        if out is None:
            st = self._step_timing_result()
            out = PlannerTickResult(self._f64(B, 38), self._f64(B, 18), self._i32(B), st.status, st)
        st = out.step_timing
        check(lib().qloco_nlp_tick(
            C.byref(self.params), C.byref(self.tick_params), B, ptr(self.workspace), ptr(self.tick_workspace),
            ptr(t_int), ptr(estimated_state), ptr(rfoot_feedback), ptr(lfoot_feedback),
            None if stop_walking is None else ptr(stop_walking), ptr(out.com_traj), ptr(out.rlfoot_traj),
            ptr(out.right_support), ptr(st.vari_ini), ptr(st.sched), ptr(st.step), ptr(st.com),
            ptr(st.pass_status), ptr(st.pass_iters), ptr(st.status), self._stream(stream)), "qloco_nlp_tick")
        return out

    def get_tick_state(self, stream=None):
        """Dense (B, 374) second record per robot (TICK_STATE_FIELDS)."""
        return self._record("qloco_nlp_tick_get_state", self.tick_workspace, self._f64(self.batch, TICK_STATE), stream)

    def set_tick_state(self, state, stream=None):
        self._record("qloco_nlp_tick_set_state", self.tick_workspace,
                     _dev(state, "f64", (self.batch, TICK_STATE), "state"), stream)


NODE_STATE = 254      # QLOCO_NLP_NODE_STATE
NODE_RING = 48        # QLOCO_NLP_NODE_RING
NODE_SCRATCH = 94     # QLOCO_NLP_NODE_SCRATCH
NODE_SCHED_LEN = 8    # QLOCO_NLP_NODE_SCHED_LEN
NODE_STATE_FIELDS = dict(  # slices of the dense record of the third workspace
    count=(0, 1), latch=(1, 2), restart=(2, 3), mpc_stop=(3, 4), co_l=(4, 7), co_r=(7, 10), ring=(10, 154),
    row=(154, 254))
NODE_BRANCHES = ("not_started", "squat", "walking", "over_time", "stopped")   # sched[:, 0]
GAIT_MSG_LEN, NRT_MSG_LEN = 100, 25


def default_node_params(**overrides):
    """NLPRTControlClass.h:16-18, NLPClass.h:37-38, RobotPara_totalmass and
    the "go1" _rad."""
    return _defaults(NlpNodeParams, "nlp_node_params_default", overrides)


@dataclass
class PlannerNodeResult:
    gait_msg: object      # (B, 100): the /MPC/Gait row
    sched: object         # (B, 8) int32: branch, _walkdtime1, _t_int, bjx1, status, count, _nTdx, ZMP_end index
    status: object        # (B,) int32


class PlannerNode(PlannerTick):
    """Batched drop-in for one iteration of the slow planner node's loop
    (gait_nlp_kmp.cpp:101-158 with NLPRTControlClass::WalkingReactStepping):
    per robot the start latch and counter, the branch, `PlannerTick`'s tick
    launched unchanged, Zmp_distributor and the 100-slot row.  The node's
    members live in a third workspace (`get_node_state`)."""

    def __init__(self, batch, device, params=None, tick_params=None, node_params=None, steplength=0.075,
                 stepwidth=None, stepheight=None, **overrides):
        self.node_params = node_params if node_params is not None else default_node_params()
        self.node_workspace = _workspace("nlp_node_workspace_bytes", batch, device)
        super().__init__(batch, device, params=params, tick_params=tick_params, steplength=steplength,
                         stepwidth=stepwidth, stepheight=stepheight, **overrides)

    def init(self, steplength, stepwidth, stepheight=None, stream=None):
        """FootStepInputs + Initialize + NLPRTControlClass() of all three records."""
        sl, sw, sh = self._step_inputs(steplength, stepwidth, stepheight)
        check(lib().qloco_nlp_node_init(C.byref(self.params), C.byref(self.tick_params), C.byref(self.node_params),
                                        self.batch, ptr(self.workspace), ptr(self.tick_workspace),
                                        ptr(self.node_workspace), ptr(sl), ptr(sw),
                                        None if sh is None else ptr(sh), self._stream(stream)),
              "qloco_nlp_node_init")

    def planner_tick(self, *args, **kw):
        """PlannerTick.tick on the same two records (the node record is not advanced)."""
        return super().tick(*args, **kw)

    def tick(self, nrt_msg, out=None, stream=None):
        """One iteration of the node loop: nrt_msg (B, 25), the latest
        /rt2nrt/state row of every robot (a device tensor; `qloco_rt_tick`'s
        output as it is).  out: a PlannerNodeResult of an earlier call."""
        B = self.batch
        _dev(nrt_msg, "f64", (B, NRT_MSG_LEN), "nrt_msg")
        if out is None:
            out = PlannerNodeResult(self._f64(B, GAIT_MSG_LEN), self._i32(B, NODE_SCHED_LEN), self._i32(B))
        check(lib().qloco_nlp_node_tick(
            C.byref(self.params), C.byref(self.tick_params), C.byref(self.node_params), B, ptr(self.workspace),
            ptr(self.tick_workspace), ptr(self.node_workspace), ptr(nrt_msg), ptr(out.gait_msg), ptr(out.sched),
            ptr(out.status), self._stream(stream)), "qloco_nlp_node_tick")
        return out

    def scratch(self):
        """Views of what the inner tick of the last `tick` wrote: com_traj
        (B, 38), rlfoot_traj (B, 18), com (B, 18), vari_ini (B, 4),
        rfoot_feedback / lfoot_feedback (B, 2), prev (B, 2: the _bjx1 and
        _td(1) of before the tick), and as int32 t_int (B,),
        right_support (B,), sched (B, 4), status (B,), branch (B,)."""
        import torch
        B = self.batch
        s = self.node_workspace[NODE_STATE * B:]
        f = lambda off, n: s[off * B:(off + n) * B].view(B, n)
        n = s[90 * B:94 * B].view(torch.int32)
        return dict(com_traj=f(0, 38), rlfoot_traj=f(38, 18), com=f(56, 18), vari_ini=f(74, 4),
                    rfoot_feedback=f(84, 2), lfoot_feedback=f(86, 2), prev=f(88, 2),
                    t_int=n[:B], right_support=n[B:2 * B], sched=n[2 * B:6 * B].view(B, 4), status=n[6 * B:7 * B],
                    branch=n[7 * B:8 * B])

    def get_node_state(self, stream=None):
        """Dense (B, 254) node record per robot (NODE_STATE_FIELDS)."""
        return self._record("qloco_nlp_node_get_state", self.node_workspace, self._f64(self.batch, NODE_STATE), stream)

    def set_node_state(self, state, stream=None):
        self._record("qloco_nlp_node_set_state", self.node_workspace,
                     _dev(state, "f64", (self.batch, NODE_STATE), "state"), stream)


def set_node_form(form):
    """Form of the node's row store: 0 (each lane writes its robot's row) or 1
    (16 rows at a time through LDS, coalesced; the default); returns the previous value.  A
    throughput knob: results do not depend on it."""
    r = lib().qloco_nlp_node_set_form(int(form))
    if r == 100:
        raise ValueError("form must be 0 or 1")
    return r


def set_group_width(gw):
    """Lanes per robot of the tick kernel (4, 8 or 16); returns the previous
    width.  A throughput knob: results do not depend on it."""
    r = lib().qloco_nlp_set_group_width(int(gw))
    if r == 100:
        raise ValueError("group width must be 4, 8 or 16")
    return r


def set_tick_group_width(gw):
    """Form of the second kernel of PlannerTick.tick: 1 (one robot per lane) or
    8 (one robot per 8-lane group); returns the previous value.  A throughput
    knob: results do not depend on it."""
    r = lib().qloco_nlp_tick_set_group_width(int(gw))
    if r == 100:
        raise ValueError("group width must be 1 or 8")
    return r
