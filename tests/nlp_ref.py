"""Restatement of the slow planner's step-timing SQP (numpy / Python fp64).

TEST INFRASTRUCTURE ONLY.  Restates, line by line, the part of
unitree_ros/mosek_nlp_kmp/src/NLP/NLPClass_sqp.cpp that csrc/qloco_nlp.hip
replaces (line numbers below are that file's):

  FootStepInputs (:51-77), the "go1" branch of Initialize (:131-138, :160-206,
  :212-216, :243-306, :343-346) and NLPClass::step_timing_opti_loop
  (:693-1102) with Indexfind (:1105-1141), step_timing_object_function
  (:1144-1173), step_timing_constraints (:1175-1458, only what reaches _A_q1,
  _b_q1, _trx12 and _det_trx12) and solve_stepping_timing (:1619-1638).

The inner QP (4 variables, 1 equality, 24 inequalities) is solved by the
oracle's qo_eqp_solve, the EiQuadProg restatement the device
Goldfarb-Idnani core is bit-compared with.  QPBaseClass::solveQP
(QP/QPBaseClass.cpp:126-152) ignores EiQuadProg's +inf return, and :795-798
add whatever _X holds to _vari_ini: the partial iterate of an infeasible solve
is part of the trajectory and is kept.

Parity unpinned: the reference needs ROS, Eigen and Armadillo, none of which
is available to the tests, so nothing here was compared with the reference
binary.  The Indexfind scans are bounded at the 27 footsteps (the reference
reads past the end), like oracle/support_phase.c.  CoM_height_solve (:936)
and with it _comz, ZMP and DCM are out of scope, as is the _nTdx > 3 tail of
the roll-out at :938-947 (later ticks overwrite it before anything reads it).

Two formulations of the transcendental steps: FIRST uses libm cosh / sinh /
log, SECOND exp pairs and log1p.  Run as a script this prints,
per compared key, the largest difference between the two over exactly the
inputs of tests/test_nlp_gpu.py: teacher-forced (the second formulation
re-seeded from the first before every tick; the two windows pooled, the
feedback-blend case on its own) and free-running.
"""
import ctypes as C
import functools
import math

import numpy as np

import oracle_lib as O

NS = 27                      # _footstepsnumber (NLPClass.h:30)
FIRST, SECOND = "first", "second"

# qloco_nlp_params: NLPClass.h:32-37, Initialize :243-306 ("go1"), the
# constructor :39-44 as NLPRTControlClass.cpp:33-56 overrides it
DEFAULTS = dict(
    dt=0.025, tstep=0.7, t_min=0.5, t_max=1.0,
    footx_vmax=3.0, footx_vmin=-2.875, footy_vmax=2.0, footy_vmin=-1.0,
    comax_max=5.0, comax_min=-5.0, comay_max=6.0, comay_min=-6.0,
    aax=50000.0, aay=50000.0, aaxv=1000.0, aayv=500.0,
    bbx=2000000.0, bby=10000000.0, rr1=1000000.0, rr2=1000000.0,
    footx_max=0.15, footx_min=-0.05,
    z_c=0.309458, g=9.8, half_hip_width=0.12675, foot_width=0.03,
    lamda_comx=0.0, lamda_comvx=0.0, lamda_comy=0.0, lamda_comvy=0.0)
PARAM_ORDER = tuple(DEFAULTS)

# dense per-robot record of qloco_nlp_get_state / set_state
FIELDS = (("ts", NS), ("tx", NS), ("td", NS), ("Lxx_ref", NS), ("Lyy_ref", NS), ("footx_ref", NS),
          ("footy_ref", NS), ("COMx_is", NS), ("COMvx_is", NS), ("COMy_is", NS), ("COMvy_is", NS),
          ("vari", 4), ("feed", 6), ("endref", 2))
STATE = sum(n for _, n in FIELDS)      # 309
SLICES = {}
_o = 0
for _k, _n in FIELDS:
    SLICES[_k] = (_o, _o + _n)
    _o += _n

SKIPPED, FINISHED = -1, -2             # QLOCO_NLP_SKIPPED / QLOCO_NLP_FINISHED
OK, INFEASIBLE, NAN, BAD = 0, 2, 3, 4  # qloco_status values used per robot


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        if k not in p:
            raise KeyError(k)
    p.update(kw)
    return p


def _log(s, f):
    """IEEE log (Python raises outside the domain)."""
    return f(s) if s > 0 else (-math.inf if s == 0 else math.nan)


class _Math:
    def __init__(self, form):
        self.form = form
        if form == FIRST:
            self.cosh, self.sinh = math.cosh, math.sinh
            self.log_sum = lambda a, b: _log(a + b, math.log)
        else:
            self.cosh = lambda x: (math.exp(x) + math.exp(-x)) / 2.0
            self.sinh = lambda x: (math.exp(x) - math.exp(-x)) / 2.0
            self.log_sum = lambda a, b: _log(a + b, lambda s: math.log1p(s - 1.0))


class _Qp:
    """One EiQuadProg workspace (4, 1, 24) and its argument buffers."""

    def __init__(self):
        self.ws = O.lib().qo_eqp_create(4, 1, 24)
        self.G, self.g0 = np.zeros(16), np.zeros(4)
        self.CE, self.ce0 = np.zeros(4), np.zeros(1)
        self.CI, self.ci0 = np.zeros(96), np.zeros(24)
        self.x = np.zeros(4)
        self.st, self.it = C.c_int(0), C.c_int(0)
        self.args = (O.P(self.G), O.P(self.g0), O.P(self.CE), O.P(self.ce0), O.P(self.CI), O.P(self.ci0),
                     O.P(self.x), C.byref(self.st), C.byref(self.it))
        self.solve = O.lib().qo_eqp_solve

    def __call__(self, G, g0, CE, ce0, CI, ci0, x0):
        self.G[:] = G.ravel(order="F")
        self.g0[:] = g0
        self.CE[:] = CE
        self.ce0[0] = ce0
        self.CI[:] = CI.ravel(order="F")
        self.ci0[:] = ci0
        self.x[:] = x0                       # _X = _vari_ini (:1621)
        self.st.value = 0
        self.it.value = 0
        f = self.solve(self.ws, *self.args)
        return self.x.copy(), f, self.st.value, self.it.value


_qp = None


def qp():
    global _qp
    if _qp is None:
        _qp = _Qp()
    return _qp


def _round(x):
    """C round(): half away from zero."""
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


class Robot:
    """One NLPClass restricted to the members the step-timing SQP touches."""

    def __init__(self, steplength=0.075, stepwidth=2 * 0.12675, prm=None, form=FIRST):
        self.p = prm or params()
        self.m = _Math(form)
        p = self.p
        # FootStepInputs :55-67
        sl = np.full(NS, float(steplength))
        sl[NS - 5:] = 0.0
        sl[0:3] = 0.0
        sl[3] = steplength / 2
        sw = np.full(NS, float(stepwidth))
        sw[0] = sw[0] / 2
        # Initialize :131-138
        sl[14] = 0.0
        sl[15:22] *= -1
        # :164-171
        self.Lxx_ref = sl.copy()
        self.Lyy_ref = np.array([(-1) ** j * sw[j] for j in range(NS)])
        # :174-181
        self.footx_ref, self.footy_ref = np.zeros(NS), np.zeros(NS)
        for i in range(1, NS):
            self.footx_ref[i] = self.footx_ref[i - 1] + sl[i - 1]
            self.footy_ref[i] = self.footy_ref[i - 1] + (-1) ** (i - 1) * sw[i - 1]
        # :195-206
        self.ts = np.full(NS, p["tstep"])
        self.td = 0.2 * self.ts
        self.tx = np.zeros(NS)
        for i in range(1, NS):
            self.tx[i] = self.tx[i - 1] + self.ts[i - 1]
            self.tx[i] = _round(self.tx[i] / p["dt"]) * p["dt"] - 0.000001
        # :234-240, :349-350
        self.COMx_is, self.COMvx_is = np.zeros(NS), np.zeros(NS)
        self.COMy_is, self.COMvy_is = np.zeros(NS), np.zeros(NS)
        self.vari = np.zeros(4)               # _Vari_ini.col(i - 1)
        self.feed = np.zeros(6)               # _comx/_comvx/_comax/_comy/_comvy/_comay _feed(i - 1)
        self.endref = np.zeros(2)             # _comvx_endref, _comvy_endref

    @property
    def Wn(self):                              # :212-214
        return math.sqrt(self.p["g"] / (self.p["z_c"] - 0.0))

    # ---- record
    def to_record(self):
        return np.concatenate([np.asarray(getattr(self, k), dtype=np.float64) for k, _ in FIELDS])

    def from_record(self, rec):
        for k, _ in FIELDS:
            a, b = SLICES[k]
            setattr(self, k, np.array(rec[a:b], dtype=np.float64))
        return self

    # ---- Indexfind :1105-1141, bounded at NS
    def _index_xyz0(self, goal):
        j = 0
        while j < NS and goal > self.tx[j] + 0.0001:
            j += 1
        return j - 1

    def _index_xyz1(self, goal):
        j = 0
        while j < NS and goal >= self.tx[j]:
            j += 1
        return j - 1

    # ---- step_timing_object_function :1144-1173 and step_timing_constraints :1175-1458
    def assemble(self, i, c):
        """The six QP arrays of one pass at the current _vari_ini (c: the
        per-tick scalars of tick())."""
        p, m, v, Wn = self.p, self.m, self.vari, self.Wn
        pi, dt = c["p"], p["dt"]
        cxf, cvxf, _, cyf, cvyf, _ = self.feed
        AxO = cxf - self.footx_ref[pi]
        BxO = cvxf / Wn
        Cx = -0.5 * c["Lxr"]
        Axv, Bxv, Cxv = Wn * BxO, Wn * AxO, -self.endref[0]
        AyO = cyf - self.footy_ref[pi]
        ByO = cvyf / Wn
        Cy = -0.5 * c["Lyr"]
        Ayv, Byv, Cyv = Wn * ByO, Wn * AyO, -self.endref[1]
        aax, aay, aaxv, aayv = p["aax"], p["aay"], p["aaxv"], p["aayv"]
        Q0 = np.zeros((4, 4))
        Q0[0, 0] = 0.5 * p["bbx"]
        Q0[1, 1] = 0.5 * p["bby"]
        Q0[2, 2] = 0.5 * (p["rr1"] + aax * AxO * AxO + aay * AyO * AyO + aaxv * Axv * Axv + aayv * Ayv * Ayv)
        Q0[2, 3] = 0.5 * (aax * AxO * BxO + aay * AyO * ByO + aaxv * Axv * Bxv + aayv * Ayv * Byv)
        Q0[3, 2] = 0.5 * (aax * BxO * AxO + aay * ByO * AyO + aaxv * Bxv * Axv + aayv * Byv * Ayv)
        Q0[3, 3] = 0.5 * (p["rr2"] + aax * BxO * BxO + aay * ByO * ByO + aaxv * Bxv * Bxv + aayv * Byv * Byv)
        Q = (Q0 + Q0.T) / 2.0                                     # :1158
        q = np.array([-p["bbx"] * c["Lxr"], -p["bby"] * c["Lyr"],
                      -p["rr1"] * c["tr1_ref"] + aax * AxO * Cx + aay * AyO * Cy + aaxv * Axv * Cxv + aayv * Ayv * Cyv,
                      -p["rr2"] * c["tr2_ref"] + aax * BxO * Cx + aay * ByO * Cy + aaxv * Bxv * Cxv + aayv * Byv * Cyv])
        G = 2 * Q                                                 # :1164, :1619
        g0 = np.zeros(4)                                          # :1165, :1620, row sums in column order
        for r in range(4):
            acc = 0.0
            for k in range(4):
                acc += G[r, k] * v[k]
            g0[r] = acc + q[r]
        # equality :1188-1190, :1632-1634
        CE = np.array([0.0, 0.0, 2.0 * v[2], -2.0 * v[3]]) * (-1)
        ce0 = -(v[2] * v[2] + (-v[3]) * v[3]) + 1
        A = np.zeros((24, 4))
        b = np.zeros(24)
        # remaining-time bounds :1193-1211
        A[0, 2], A[1, 2], A[2, 3], A[3, 3] = 1, -1, 1, -1
        b[0] = -v[2] + c["tr1_max"]
        b[1] = v[2] - c["tr1_min"]
        b[2] = -v[3] + c["tr2_max"]
        b[3] = v[3] - c["tr2_min"]
        # foot location :1216-1246, :1294-1311
        hw, fw = p["half_hip_width"], p["foot_width"]
        late = i >= _round(2 * self.ts[1] / dt) + 1
        if c["period"] % 2 == 0:
            fy_min = -(2 * hw + 0.03)
            fy_max = -(fw + 0.01) if late else -(hw - 0.03)
        else:
            fy_max = 2 * hw + 0.03
            fy_min = fw + 0.01 if late else hw - 0.03
        c["late"] = bool(late)
        A[4, 0], A[5, 0], A[6, 1], A[7, 1] = 1, -1, 1, -1
        b[4] = -v[0] + p["footx_max"]
        b[5] = v[0] - p["footx_min"]
        b[6] = -v[1] + fy_max
        b[7] = v[1] - fy_min
        # swing-foot velocity :1314-1336 (all zero at _k_yu == 0)
        if c["k_yu"] != 0:
            A[8, 0], A[9, 0], A[10, 1], A[11, 1] = 1, -1, 1, -1
            b[8] = -(v[0] - self.Lxx_ref[pi] - p["footx_vmax"] * dt)
            b[9] = v[0] - self.Lxx_ref[pi] - p["footx_vmin"] * dt
            b[10] = -(v[1] - self.Lyy_ref[pi] - p["footy_vmax"] * dt)
            b[11] = v[1] - self.Lyy_ref[pi] - p["footy_vmin"] * dt
        # CoM acceleration :1341-1363
        sh, ch = c["sh_dt"], c["ch_dt"]
        AA = Wn * sh
        CCx, CCy = AxO, AyO
        BBx, BBy = (Wn * Wn) * CCx * ch, (Wn * Wn) * CCy * ch
        rows = []
        for (a1, a2, a3, hi, lo) in (
                (AA * Wn, -2 * AA * CCx * Wn, 2 * BBx, 2 * p["comax_max"], 2 * p["comax_min"]),
                (AA * Wn, -2 * AA * CCy * Wn, 2 * BBy, 2 * p["comay_max"], 2 * p["comay_min"])):
            rows.append((a1, a2, a3 - hi, a3 - hi, a3 - lo, a3 - lo))
        # CoM velocity increment :1366-1387
        VAA = ch
        VBBx, VBBy = Wn * CCx * sh, Wn * CCy * sh
        for (a1, a2, a3, hi, lo) in (
                (VAA * Wn, -2 * VAA * CCx * Wn, 2 * VBBx - 2 * cvxf, 2 * p["comax_max"] * dt, 2 * p["comax_min"] * dt),
                (VAA * Wn, -2 * VAA * CCy * Wn, 2 * VBBy - 2 * cvyf, 2 * p["comay_max"] * dt, 2 * p["comay_min"] * dt)):
            rows.append((a1, a2, a3 - hi, a3 - hi, a3 - lo, a3 - lo))
        # CoM initial velocity :1392-1411 (the row and its offset use different limits, as written)
        for (a1, a2, a3, hi, lo) in (
                (Wn, -2 * CCx * Wn, -2 * cvxf, 2 * p["comax_max"] * dt, 2 * p["comax_min"] * dt),
                (Wn, -2 * CCy * Wn, -2 * cvyf, 2 * p["comay_max"] * dt, 2 * p["comay_min"] * dt)):
            rows.append((a1, a2, a3 - hi, a3 - hi / 2.0, a3 - lo, a3 - lo / 2.0))
        for blk in range(3):
            for ax in range(2):
                a1, a2, up_row, up_det, lo_row, lo_det = rows[2 * blk + ax]
                r = 12 + 4 * blk + 2 * ax
                A[r, ax], A[r, 2], A[r, 3] = a1, a2, up_row
                b[r] = -((a1 * v[ax] + a2 * v[2]) + up_det * v[3])
                A[r + 1, ax], A[r + 1, 2], A[r + 1, 3] = -a1, -a2, -lo_row
                b[r + 1] = -((-a1 * v[ax] + -a2 * v[2]) + -lo_det * v[3])
        CI = A.T * (-1)                                           # :1627
        return G, g0, CE, ce0, CI, b

    # ---- step_timing_opti_loop :693-1102
    def tick(self, i, est=None, rfoot=(0.0, -0.12675), lfoot=(0.0, 0.12675)):
        p, m, Wn = self.p, self.m, self.Wn
        dt = p["dt"]
        est = np.zeros(6) if est is None else np.array(est, dtype=np.float64)
        out = dict(status=OK, pass_status=[SKIPPED] * 3, pass_iters=[0] * 3, active=[(), (), ()],
                   vari=np.full(4, np.nan), sched=[0, 0, 0, 0], step=np.full(3, np.nan),
                   com=np.full(18, np.nan), census={})
        period = self._index_xyz0((i + 1) * dt) + 1              # :702-704
        out["sched"][0] = period
        if i < 1 or period < 1:
            out["status"] = BAD
            return out
        if period > NS - 1:
            out["status"] = FINISHED
            return out
        pi = period - 1
        px, py = self.footx_ref[pi], self.footy_ref[pi]          # :708-709
        ki = _round(self.tx[pi] / dt)                            # :714-716
        k_yu = int(i - ki)
        Tk = self.ts[pi] - k_yu * dt
        Lxr, Lyr = self.Lxx_ref[pi], self.Lyy_ref[pi]            # :724-725
        tr1_ref, tr2_ref = m.cosh(Wn * Tk), m.sinh(Wn * Tk)      # :727
        ref = np.array([Lxr, Lyr, tr1_ref, tr2_ref])
        if i == 1:                                               # :730-740
            self.vari = ref.copy()
        rem = p["t_min"] - k_yu * dt                             # :745-757
        clamp = not (rem >= 0.001)
        arg = 0.001 if clamp else rem
        tr1_min, tr2_min = m.cosh(Wn * arg), m.sinh(Wn * arg)
        tr1_max, tr2_max = m.cosh(Wn * (p["t_max"] - k_yu * dt)), m.sinh(Wn * (p["t_max"] - k_yu * dt))
        if i == 1:                                               # :761-771
            self._boundary(pi)
        c = dict(p=pi, period=period, k_yu=k_yu, Lxr=Lxr, Lyr=Lyr, tr1_ref=tr1_ref, tr2_ref=tr2_ref,
                 tr1_min=tr1_min, tr2_min=tr2_min, tr1_max=tr1_max, tr2_max=tr2_max,
                 sh_dt=m.sinh(Wn * dt), ch_dt=m.cosh(Wn * dt))
        gate = Tk >= 0.1 * self.ts[pi]                           # :791
        inf_added = 0
        for k in range(3):                                       # :776-810
            arrays = self.assemble(i, c)
            if gate:
                x, f, st, it = qp()(*arrays, self.vari)
                out["pass_status"][k], out["pass_iters"][k] = st, it
                s = arrays[4].T @ x + arrays[5]
                out["active"][k] = tuple(int(j) for j in np.nonzero(s <= 1e-9)[0]) if st == 0 else ()
                if st == INFEASIBLE:
                    inf_added += 1
                self.vari = self.vari + x                        # :795-798
            else:
                self.vari = ref.copy()                           # :802-805
        v = self.vari
        # :817, :886-901
        self.Lxx_ref[pi], self.Lyy_ref[pi] = v[0], v[1]
        self.ts[pi] = k_yu * dt + m.log_sum(v[2], v[3]) / Wn    # :888
        self._boundary(pi)
        for jxx in range(period + 1, NS + 1):                    # :906-909
            self.tx[jxx - 1] = self.tx[jxx - 2] + self.ts[jxx - 2]
        self.footx_ref[period] = self.footx_ref[pi] + v[0]       # :912-913
        self.footy_ref[period] = self.footy_ref[pi] + v[1]
        xi, vxi, yi, vyi = self.COMx_is[pi], self.COMvx_is[pi], self.COMy_is[pi], self.COMvy_is[pi]
        com = np.zeros(18)
        for jxx in (1, 2, 3):                                    # :938-947
            w = Wn * dt * jxx
            ch, sh = m.cosh(w), m.sinh(w)
            com[6 * (jxx - 1):6 * jxx] = (xi * ch + vxi * 1 / Wn * sh + px, yi * ch + vyi * 1 / Wn * sh + py,
                                          Wn * xi * sh + vxi * ch, Wn * yi * sh + vyi * ch,
                                          (Wn * Wn) * xi * ch + vxi * Wn * sh, (Wn * Wn) * yi * ch + vyi * Wn * sh)
        foot = lfoot if period % 2 == 0 else rfoot               # :966-975
        e0, e3 = est[0] - foot[0], est[3] - foot[1]
        lx, lvx, ly, lvy = p["lamda_comx"], p["lamda_comvx"], p["lamda_comy"], p["lamda_comvy"]
        self.feed = np.array([((1 - lx) * (com[0] - px) + lx * e0) + px,       # :1017-1022
                              (1 - lvx) * com[2] + lvx * est[1],
                              (1 - lx) * com[4] + lx * est[2],
                              ((1 - ly) * (com[1] - py) + ly * e3) + py,
                              (1 - lvy) * com[3] + lvy * est[4],
                              (1 - ly) * com[5] + ly * est[5]])
        bjxx = self._index_xyz1(i * dt) + 1                      # :1033-1039
        bjx1 = self._index_xyz1((i + 1) * dt) + 1
        self.td = 0.2 * self.ts                                  # :1041
        out.update(vari=v.copy(), sched=[period, k_yu, bjxx, bjx1],
                   step=np.array([self.ts[pi], self.Lxx_ref[pi], self.Lyy_ref[pi]]), com=com,
                   census=dict(i1=i == 1, kyu0=k_yu == 0, inf=inf_added, clamp=clamp, skip=not gate,
                               late=c["late"], even=period % 2 == 0, neg=15 <= pi <= 21))
        if not (np.isfinite(v).all() and np.isfinite(com).all() and np.isfinite(out["step"]).all()):
            out["status"] = NAN
        return out

    def _boundary(self, pi):
        """:763-770 / :896-901, :915-916."""
        v, Wn = self.vari, self.Wn
        self.COMx_is[pi] = self.feed[0] - self.footx_ref[pi]
        ex = v[0] * 0.5
        self.COMvx_is[pi] = _div(ex - self.COMx_is[pi] * v[2], 1 / Wn * v[3])
        self.COMy_is[pi] = self.feed[3] - self.footy_ref[pi]
        ey = v[1] * 0.5
        self.COMvy_is[pi] = _div(ey - self.COMy_is[pi] * v[2], 1 / Wn * v[3])
        self.endref = np.array([Wn * self.COMx_is[pi] * v[3] + self.COMvx_is[pi] * v[2],
                                Wn * self.COMy_is[pi] * v[3] + self.COMvy_is[pi] * v[2]])


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    return float(np.float64(a) / np.float64(b)) if b == 0 or b != b else a / b


# ------------------------------------------------------------------ test inputs
B_MAIN, T_MAIN = 67, 90
PUSH_TICKS = (7, 23, 41, 58, 77)
LATE_START, T_LATE = 405, 30           # steps 15-16: _steplength changes sign at step 15


def robot_inputs(seed, batch):
    """Per-robot step length in [0.04, 0.09], width within +-10 % of 2 * half hip."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.04, 0.09, batch), 2 * 0.12675 * rng.uniform(0.9, 1.1, batch)


def tick_inputs(seed, batch, ticks):
    """estimated_state[0:6] (read only through the _lamda_* blend), the two
    foot-location feedbacks, and the pushes: at PUSH_TICKS a third of the robots
    get at most +-4 mm / +-0.05 m/s added to the feed state before the tick."""
    rng = np.random.default_rng(seed + 1000)
    est = rng.normal(0.0, 0.02, (ticks, batch, 6))
    rf = np.tile([0.0, -0.12675], (ticks, batch, 1)) + rng.normal(0, 0.002, (ticks, batch, 2))
    lf = np.tile([0.0, 0.12675], (ticks, batch, 1)) + rng.normal(0, 0.002, (ticks, batch, 2))
    push = np.zeros((ticks, batch, 6))
    for t in PUSH_TICKS:
        if t < ticks:
            who = rng.random(batch) < 1 / 3
            d = np.zeros((batch, 6))
            d[:, 0] = rng.uniform(-0.004, 0.004, batch)
            d[:, 3] = rng.uniform(-0.004, 0.004, batch)
            d[:, 1] = rng.uniform(-0.05, 0.05, batch)
            d[:, 4] = rng.uniform(-0.05, 0.05, batch)
            push[t] = d * who[:, None]
    return dict(est=est, rfoot=rf, lfoot=lf, push=push)


OUT_KEYS = ("vari", "step", "com")
REC_KEYS = tuple(k for k, _ in FIELDS)


@functools.lru_cache(maxsize=None)
def rollout(seed=11, batch=B_MAIN, ticks=T_MAIN, i0=1, form=FIRST, teacher=None, lam=0.0):
    """Roll `batch` robots `ticks` ticks from tick i0.  Returns arrays over
    (tick, robot): record_in (the record before the tick, after the push),
    record_out, the outputs, the integer outputs and the census.  i0 > 1 first
    runs the first formulation up to i0 (no pushes).  teacher: a first-
    formulation roll-out whose record_in re-seeds every tick."""
    prm = params(lamda_comx=lam, lamda_comvx=lam / 10, lamda_comy=lam, lamda_comvy=lam / 10)
    sl, sw = robot_inputs(seed, batch)
    inp = tick_inputs(seed, batch, ticks)
    T, B = ticks, batch
    res = dict(record_in=np.zeros((T, B, STATE)), record_out=np.zeros((T, B, STATE)),
               vari=np.zeros((T, B, 4)), step=np.zeros((T, B, 3)), com=np.zeros((T, B, 18)),
               sched=np.zeros((T, B, 4), np.int32), pass_status=np.zeros((T, B, 3), np.int32),
               pass_iters=np.zeros((T, B, 3), np.int32), status=np.zeros((T, B), np.int32),
               active=[[None] * B for _ in range(T)], census=[[None] * B for _ in range(T)],
               t_int=np.zeros((T, B), np.int32), inputs=inp, steplength=sl, stepwidth=sw, params=prm)
    for b in range(B):
        rob = Robot(sl[b], sw[b], prm, form)
        if i0 > 1:
            warm = Robot(sl[b], sw[b], prm, FIRST)
            for i in range(1, i0):
                warm.tick(i)
            rob.from_record(warm.to_record())
        for t in range(T):
            i = i0 + t
            if teacher is not None:
                rob.from_record(teacher["record_in"][t, b])
            else:
                rob.feed = rob.feed + inp["push"][t, b]
            res["record_in"][t, b] = rob.to_record()
            o = rob.tick(i, inp["est"][t, b], inp["rfoot"][t, b], inp["lfoot"][t, b])
            res["record_out"][t, b] = rob.to_record()
            res["t_int"][t, b] = i
            for k in OUT_KEYS:
                res[k][t, b] = o[k]
            res["sched"][t, b] = o["sched"]
            res["pass_status"][t, b] = o["pass_status"]
            res["pass_iters"][t, b] = o["pass_iters"]
            res["status"][t, b] = o["status"]
            res["active"][t][b] = o["active"]
            res["census"][t][b] = o["census"]
    return res


class _Hashable(dict):
    """A roll-out as an lru_cache key of rollout(teacher=...): by identity."""

    def __hash__(self):
        return id(self)


def cases():
    """(name, rollout keyword arguments) of the GPU tests' inputs."""
    return (("main", dict(seed=11, batch=B_MAIN, ticks=T_MAIN, i0=1)),
            ("late", dict(seed=12, batch=9, ticks=T_LATE, i0=LATE_START)),
            # the feedback blend with _lamda_* = 0.02 / 0.002 across the first step boundary: the only
            # inputs through which estimated_state and the two foot-location feedbacks act
            ("blend", dict(seed=13, batch=9, ticks=12, i0=22, lam=0.02)))


def spread(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    d = d[np.isfinite(a) & np.isfinite(b)]
    return float(d.max()) if d.size else 0.0


def _keyed(res):
    d = {k: res[k] for k in OUT_KEYS}
    for k in REC_KEYS:
        a, b = SLICES[k]
        d["rec_" + k] = res["record_out"][..., a:b]
    return d


def decisions_equal(a, b):
    """status, iteration count and active set of every solve."""
    return (np.array_equal(a["pass_status"], b["pass_status"]) and np.array_equal(a["pass_iters"], b["pass_iters"])
            and a["active"] == b["active"] and np.array_equal(a["sched"], b["sched"]))


def t_end_footstep(prm=None):
    """round((_tx(26) - 2 _tstep) / _dt) of the initial schedule (:593)."""
    p = prm or params()
    return int(_round((Robot(prm=p).tx[NS - 1] - 2 * p["tstep"]) / p["dt"]))


def support_margin(ts, tx, i, dt=0.025):
    """Distance (seconds) of one robot's schedule from every decision boundary
    of qo_support_phase at loop index i: the two Indexfind comparisons, the
    tie of round(_tx / dt) and the double-support test."""
    m = min(np.abs(i * dt - tx).min(), np.abs((i + 1) * dt - tx).min())
    b1 = int(np.sum(np.cumprod((i + 1) * dt >= tx)))
    if b1 >= 2:
        q = tx[b1 - 1] / dt
        m = min(m, abs(abs(q - math.floor(q)) - 0.5) * dt)
        m = min(m, abs((i + 1 - _round(q)) * dt - 0.2 * ts[b1 - 1]))
    return float(m)


CHAIN_MARGIN = 1e-9


def chain_mask(res):
    """(tick, robot) pairs of a roll-out whose updated schedule sits more than
    CHAIN_MARGIN from every decision boundary of support_phase."""
    T, B = res["t_int"].shape
    (a0, a1), (b0, b1) = SLICES["ts"], SLICES["tx"]
    out = np.zeros((T, B), bool)
    for t in range(T):
        for b in range(B):
            rec = res["record_out"][t, b]
            out[t, b] = res["status"][t, b] == OK and \
                support_margin(rec[a0:a1], rec[b0:b1], int(res["t_int"][t, b]), res["params"]["dt"]) > CHAIN_MARGIN
    return out


# teacher-forced spreads are pooled per group of cases: the issue's two windows
# together, the feedback-blend case on its own
GROUPS = dict(main="teacher", late="teacher", blend="blend")


def measure():
    """{'teacher': {key: spread}, 'blend': {key: spread}, 'free': {key: spread}}
    over cases(): teacher-forced per group of cases (GROUPS), free-running
    over the main case."""
    out = dict(teacher={}, blend={}, free={})
    for name, kw in cases():
        a = rollout(form=FIRST, **kw)
        modes = {GROUPS[name]: rollout(form=SECOND, teacher=_Hashable(a), **kw)}
        if name == "main":
            modes["free"] = rollout(form=SECOND, **kw)
        for mode, b in modes.items():
            assert decisions_equal(a, b), (name, mode)
            ka, kb = _keyed(a), _keyed(b)
            for k in ka:
                out[mode][k] = max(out[mode].get(k, 0.0), spread(ka[k], kb[k]))
    return out


if __name__ == "__main__":
    m = measure()
    for mode in ("teacher", "blend", "free"):
        print(mode + ":", " ".join("%s %.3e" % kv for kv in m[mode].items()))
