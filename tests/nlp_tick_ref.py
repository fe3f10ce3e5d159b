"""Restatement of the rest of the slow planner's tick (numpy / Python fp64):
CoM height, ZMP / DCM and the swing feet.

TEST INFRASTRUCTURE ONLY.  Restates, line by line, what csrc/qloco_nlp_tick.hip
adds to the step-timing SQP of tests/nlp_ref.py (line numbers are those of
unitree_ros/mosek_nlp_kmp/src/NLP/NLPClass_sqp.cpp):

  CoM_height_solve (:2361-2473) as :936 calls it -- with the _bjx1 of the
  previous tick (it is reassigned at :1038 only; 0 after Initialize, :488) and
  the _ts / _tx the SQP of this tick has just updated; the ZMP and DCM samples
  (:950-954) with _Zsc as Initialize builds it (:323-328); the 38-vector
  (:1048-1090); Foot_trajectory_solve_mod2 (:2039-2358) with solve_AAA_inv2
  (:3633-3644), called right after step_timing_opti_loop with the same index
  (NLPRTControlClass.cpp:445-459).  Members: _footz_ref (:176-180),
  _lift_height_ref (:71-75), _t_end_footstep (:593), _hcom (:212),
  _footxyz_real as :1043-1046 leave it.

Nothing here feeds back into the SQP, so a roll-out is a post-process of an
nlp_ref.rollout: the record after each tick, `sched`, `com` and `status`.

_Zsc(k): Initialize looks _t_whole(k) up, a LinSpaced grid from _dt to _tx(26)
whose step is 1.4e-9 s short of _dt; this restatement (and the kernel) looks
(k + 1) _dt up, which falls in the same step for every k < _nsum - 1.  The
_Lfootx .. _Rfootz arrays of _nsum entries are kept as a ring of RING entries
per robot: the reference reads no further back than round(_tx(_bjx1-1)/_dt) - 2.
An index the ring no longer holds reads as NaN, one not yet written as the
value Initialize gave the arrays (:496-499).

Parity unpinned (no Eigen here, the reference needs ROS).  Two formulations:

  A  what Eigen does: the 7 x 7 system by partial-pivot LU, the inverse formed
     in full, then its product with the right-hand side; the 4 x 4 by the
     cofactor inverse of Eigen's fixed-size path, then the product; powers by
     pow(); over the FIRST formulation of the SQP.
  B  each system solved directly by LU, no inverse; powers by repeated
     multiplication, polynomials by Horner; over the SECOND formulation of the
     SQP (exp pairs, log1p).

Run as a script this prints the largest A - B difference per output key,
teacher-forced and free-running, with the median of the non-zero per
robot-tick differences, the smallest |t_plan(0) - t_plan(1)| and the largest
4 x 4 condition number.  SPREAD_TEACHER / SPREAD_FREE below are that output.
"""
import functools
import math

import numpy as np

import nlp_ref as R

NS = R.NS
RING = 48                              # QLOCO_NLP_TICK_RING
A, B = "A", "B"
NAN = math.nan

# qloco_nlp_tick_params: _lift_height (NLPRTControlClass.cpp:48), _hcom =
# RobotPara_Z_C - _height_offset (:212, NLPClass.h:37)
TICK_DEFAULTS = dict(lift_height=0.03, hcom=0.309458)
GGG = 9.8                              # _ggg (:538)

# dense per-robot record of qloco_nlp_tick_get_state / set_state
FIELDS = (("bjx1", 1), ("ry", 1), ("t_end", 1), ("sw0", 1), ("last", 1), ("footz_ref", NS), ("lift", NS),
          ("tx0", NS), ("ring", RING * 6))
STATE = sum(n for _, n in FIELDS)      # 374
SLICES = {}
_o = 0
for _k, _n in FIELDS:
    SLICES[_k] = (_o, _o + _n)
    _o += _n


# ------------------------------------------------------------------ linear algebra, scalar by scalar
def _lu(M):
    """Partial-pivot LU in place (row swaps; the first largest |.| wins).
    Returns (LU as lists, row permutation)."""
    n = len(M)
    a = [list(map(float, r)) for r in M]
    perm = list(range(n))
    for k in range(n):
        p, best = k, abs(a[k][k])
        for r in range(k + 1, n):
            if abs(a[r][k]) > best:
                p, best = r, abs(a[r][k])
        if p != k:
            a[k], a[p] = a[p], a[k]
            perm[k], perm[p] = perm[p], perm[k]
        for r in range(k + 1, n):
            a[r][k] = _div(a[r][k], a[k][k])
            for c in range(k + 1, n):
                a[r][c] = a[r][c] - a[r][k] * a[k][c]
    return a, perm


def _div(a, b):
    return R._div(a, b)


def _lu_solve(a, perm, rhs):
    n = len(a)
    y = [rhs[perm[r]] for r in range(n)]
    for r in range(n):
        acc = y[r]
        for c in range(r):
            acc = acc - a[r][c] * y[c]
        y[r] = acc
    for r in range(n - 1, -1, -1):
        acc = y[r]
        for c in range(r + 1, n):
            acc = acc - a[r][c] * y[c]
        y[r] = _div(acc, a[r][r])
    return y


def _lu_inverse(M):
    n = len(M)
    a, perm = _lu(M)
    cols = [_lu_solve(a, perm, [1.0 if r == j else 0.0 for r in range(n)]) for j in range(n)]
    return [[cols[j][r] for j in range(n)] for r in range(n)]


def _matvec(M, v):
    out = []
    for row in M:
        acc = 0.0
        for k in range(len(v)):
            acc = acc + row[k] * v[k]
        out.append(acc)
    return out


def _cofactor_inverse4(m):
    """Eigen's compute_inverse_size4 (scalar path): cofactors by three 3 x 3
    sub-determinants each, the determinant along column 0, one division."""
    def det3(i1, j1, i2, j2, i3, j3):
        return m[i1][j1] * (m[i2][j2] * m[i3][j3] - m[i2][j3] * m[i3][j2])

    def cof(i, j):
        i1, i2, i3 = (i + 1) % 4, (i + 2) % 4, (i + 3) % 4
        j1, j2, j3 = (j + 1) % 4, (j + 2) % 4, (j + 3) % 4
        return det3(i1, j1, i2, j2, i3, j3) + det3(i2, j1, i3, j2, i1, j3) + det3(i3, j1, i1, j2, i2, j3)

    res = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            res[j][i] = cof(i, j) if (i + j) % 2 == 0 else -cof(i, j)
    det = 0.0
    for k in range(4):
        det = det + m[k][0] * res[0][k]
    return [[_div(res[r][c], det) for c in range(4)] for r in range(4)]


def _powers(t, n, form):
    """[t^n, .., t^1, 1]."""
    if form == A:
        return [math.pow(t, k) for k in range(n, 0, -1)] + [1.0]
    p = [1.0, t]
    for _ in range(n - 1):
        p.append(p[-1] * t)
    return p[::-1]


def _dot(a, b):
    acc = 0.0
    for x, y in zip(a, b):
        acc = acc + x * y
    return acc


# ------------------------------------------------------------------ members
class TickState:
    """The members of one NLPClass the tick reads beyond the SQP's record."""

    def __init__(self, stepwidth=2 * 0.12675, stepheight=0.0, prm=None, tprm=None):
        p = prm or R.params()
        tp = tprm or dict(TICK_DEFAULTS)
        self.bjx1, self.ry, self.last = 0, 0.0, 0             # :488, :500
        self.sw0 = float(stepwidth) / 2                        # _stepwidth(0), :67
        self.footz_ref = np.zeros(NS)                          # :176-180
        for i in range(1, NS):
            self.footz_ref[i] = self.footz_ref[i - 1] + float(stepheight)
        lh = tp["lift_height"]                                 # :71-75
        self.lift = np.full(NS, lh)
        self.lift[NS - 1] = 0.0
        self.lift[NS - 2] = 0.0
        self.lift[NS - 3] = lh / 2
        self.lift[NS - 4] = lh
        self.tx0 = R.Robot(prm=p).tx.copy()                    # the initial _tx, for _Zsc (:323-328)
        self.t_end = int(R._round((self.tx0[NS - 1] - 2 * p["tstep"]) / p["dt"]))   # :593
        self.ring = np.tile(self.init6(), (RING, 1))           # :496-499

    def init6(self):
        return np.array([0.0, -self.sw0, 0.0, 0.0, self.sw0, 0.0])

    def to_record(self):
        return np.concatenate([[self.bjx1, self.ry, self.t_end, self.sw0, self.last], self.footz_ref, self.lift,
                               self.tx0, self.ring.ravel()]).astype(np.float64)

    def from_record(self, rec):
        self.bjx1, self.ry, self.t_end = int(rec[0]), float(rec[1]), int(rec[2])
        self.sw0, self.last = float(rec[3]), int(rec[4])
        for k in ("footz_ref", "lift", "tx0"):
            a, b = SLICES[k]
            setattr(self, k, np.array(rec[a:b], dtype=np.float64))
        a, b = SLICES["ring"]
        self.ring = np.array(rec[a:b], dtype=np.float64).reshape(RING, 6)
        return self

    def rd(self, k):
        """Both feet's xyz at array index k (Rx, Ry, Rz, Lx, Ly, Lz)."""
        if k > self.last + 1:
            return self.init6()
        if k < 0 or k <= self.last + 1 - RING:
            return np.full(6, NAN)
        return self.ring[k % RING].copy()


def _zsc(st, k, p):
    nsum = (NS - 1) * int(R._round(p["tstep"] / p["dt"]))      # NLPClass.h:35-36
    if k < 0 or k >= nsum - 1:
        return 0.0
    goal, j = (k + 1) * p["dt"], 0
    while j < NS and goal >= st.tx0[j]:
        j += 1
    return float(st.footz_ref[j - 1]) if j >= 1 else NAN


def _at(arr, k):
    return float(arr[k]) if 0 <= k < NS else NAN


def tick_part(st, form, p, tp, i, sched, com, status, rec, stop):
    """What follows the SQP in one tick.  sched / com / status: the SQP's
    outputs of this tick; rec: its record after the tick."""
    out = dict(com_traj=np.full(38, NAN), rlfoot=np.full(18, NAN), right_support=2, status=int(status),
               branch="none", latch=False, gap=NAN, m4=None)
    if status in (R.FINISHED, R.BAD):
        return out
    dt, hcom = p["dt"], tp["hcom"]
    S = R.SLICES
    ts, tx, td = rec[slice(*S["ts"])], rec[slice(*S["tx"])], rec[slice(*S["td"])]
    fx, fy = rec[slice(*S["footx_ref"])], rec[slice(*S["footy_ref"])]
    lxx, lyy = rec[slice(*S["Lxx_ref"])], rec[slice(*S["Lyy_ref"])]
    fz = st.footz_ref
    period, _, bjxx, bjx1 = (int(v) for v in sched)
    # ---- CoM_height_solve (:2361-2473) with the previous tick's _bjx1
    b0 = st.bjx1
    cz, cvz, caz = [hcom] * 3, [0.0] * 3, [0.0] * 3
    if b0 >= 2:
        tsb = _at(ts, b0 - 1)
        tpl = (0.0001, tsb / 2 + 0.0001, tsb + 0.0001)
        pw = [_powers(t, 6, form) for t in tpl]                # t^6 .. t, 1
        rows = []
        for which, t in (("v", 0), ("a", 0), ("p", 0), ("p", 1), ("p", 2), ("v", 2), ("a", 2)):
            q = pw[t]
            if which == "p":
                rows.append([q[0], q[1], q[2], q[3], q[4], q[5], 1.0])
            elif which == "v":
                rows.append([6 * q[1], 5 * q[2], 4 * q[3], 3 * q[4], 2 * q[5], 1.0, 0.0])
            else:
                rows.append([30 * q[2], 20 * q[3], 12 * q[4], 6 * q[5], 2.0, 0.0, 0.0])
        plan = [0.0, 0.0, _at(fz, b0 - 2) + hcom, (_at(fz, b0 - 2) + _at(fz, b0 - 1)) / 2 + hcom,
                _at(fz, b0 - 1) + hcom, 0.0, 0.0]
        if form == A:
            co = _matvec(_lu_inverse(rows), plan)
        else:
            co = _lu_solve(*_lu(rows), plan)
        rt0 = R._round(_at(tx, b0 - 1) / dt) if _at(tx, b0 - 1) == _at(tx, b0 - 1) else NAN
        for jxx in (1, 2, 3):
            t_des = (i + jxx - rt0) * dt
            if form == A:
                q = _powers(t_des, 6, A)
                cz[jxx - 1] = _dot(q, co)
                cvz[jxx - 1] = _dot([6 * q[1], 5 * q[2], 4 * q[3], 3 * q[4], 2 * q[5], 1.0, 0.0], co)
                caz[jxx - 1] = _dot([30 * q[2], 20 * q[3], 12 * q[4], 6 * q[5], 2.0, 0.0, 0.0], co)
            else:
                t = t_des
                cz[jxx - 1] = (((((co[0] * t + co[1]) * t + co[2]) * t + co[3]) * t + co[4]) * t + co[5]) * t + co[6]
                cvz[jxx - 1] = ((((6 * co[0] * t + 5 * co[1]) * t + 4 * co[2]) * t + 3 * co[3]) * t + 2 * co[4]) * t + co[5]
                caz[jxx - 1] = (((30 * co[0] * t + 20 * co[1]) * t + 12 * co[2]) * t + 6 * co[3]) * t + 2 * co[4]
    st.bjx1 = bjx1                                               # :1038
    # ---- :950-954, :1048-1090
    c = out["com_traj"]
    zd = []
    for s in range(3):
        comx, comy, comvx, comvy, comax, comay = (float(v) for v in com[6 * s:6 * s + 6])
        q = _div(cz[s] - _zsc(st, i + s, p), caz[s] + GGG)
        r = math.sqrt(q) if q >= 0 else NAN
        zd.append((comx - q * comax, comy - q * comay, comx + comvx * r, comy + comvy * r))
    c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8] = com[0], com[1], cz[0], com[2], com[3], cvz[0], com[4], com[5], caz[0]
    c[9:13], c[13:17], c[17:21] = zd[0], zd[1], zd[2]
    c[21], c[22], c[23] = com[10], com[11], caz[1]
    c[24], c[25], c[26] = com[16], com[17], caz[2]
    c[27] = bjxx
    if 0 <= bjxx and bjxx + 1 < NS:
        c[28], c[29], c[30], c[31], c[32], c[33] = fx[bjxx], fx[bjxx + 1], fy[bjxx], fy[bjxx + 1], fz[bjxx], fz[bjxx + 1]
    c[34] = period - 1
    c[35], c[36], c[37] = ts[period - 1], lxx[period - 1], lyy[period - 1]
    # ---- Foot_trajectory_solve_mod2 (:2039-2358)
    if stop or i > st.t_end:                                     # :2043-2050
        st.lift[bjx1 + 1:NS] = 0.0
    fyr = np.array(fy, dtype=np.float64)
    fyr[0] = -st.sw0                                             # :1046, :2052
    cur, nxt = st.rd(i), st.rd(i + 1)
    vel, acc = [0.0] * 6, [0.0] * 6
    rs = 2
    if bjx1 >= 2 and i <= st.t_end:                              # :2076
        b = bjx1
        txb, tsb, tdb = _at(tx, b - 1), _at(ts, b - 1), _at(td, b - 1)
        rt = R._round(txb / dt) if txb == txb else NAN
        H = st.rd(int(rt) - 2) if rt == rt else np.full(6, NAN)
        sw = 0 if b % 2 == 0 else 3                              # the swing foot's columns: right, left
        sn = 3 - sw
        rs = 0 if b % 2 == 0 else 1
        cur[sn:sn + 3] = H[sn:sn + 3]                            # :2082-2088, :2191-2197
        nxt[sn:sn + 3] = H[sn:sn + 3]
        if (i + 1 - rt) * dt < tdb:                              # :2091, :2200
            rs = 2
            cur[sw:sw + 3] = H[sw:sw + 3]
            nxt[sw:sw + 3] = H[sw:sw + 3]
            out["branch"] = "ds"
        else:
            t_des = (i + 1 - rt + 1) * dt
            tpl = (t_des - dt, (tdb + tsb) / 2 + 0.0001, tsb)
            F = lambda k: np.array([_at(fx, k), _at(fyr, k), _at(fz, k)])
            if abs(t_des - tsb) <= 0.0005:                       # :2113, :2226
                cur[sw:sw + 3] = F(bjxx)
                nxt[sw:sw + 3] = F(bjxx)
                out["branch"] = "snap"
            else:
                out["branch"] = "cubic"
                out["gap"] = abs(tpl[0] - tpl[1])
                pw = [_powers(t, 3, form) for t in tpl]
                M = [pw[0], pw[1], pw[2], [3 * pw[2][1], 2 * pw[2][2], 1.0 if form == B else math.pow(tpl[2], 0), 0.0]]
                out["m4"] = M
                prev = st.rd(i - 1)
                if (i + 1 - rt) * dt < tdb + dt:                 # :2150, :2268
                    st.ry = (_at(fyr, bjxx) + _at(fyr, bjxx - 2)) / 2
                    out["latch"] = True
                f0, f2 = F(bjxx - 2), F(bjxx)
                z_mid = (f2[2] if f0[2] < f2[2] else f0[2]) + _at(st.lift, b - 1)   # std::max
                plans = ([prev[sw], (f0[0] + f2[0]) / 2, f2[0], 0.0], [prev[sw + 1], st.ry, f2[1], 0.0],
                         [prev[sw + 2], z_mid, f2[2], 0.0])
                if form == A:
                    inv = _cofactor_inverse4(M)
                    cos = [_matvec(inv, pl) for pl in plans]
                else:
                    lu = _lu(M)
                    cos = [_lu_solve(*lu, pl) for pl in plans]
                t = t_des
                for ax, co in enumerate(cos):
                    if form == A:
                        q = _powers(t, 3, A)
                        pos = _dot(q, co)
                        v = _dot([3 * q[1], 2 * q[2], 1.0, 0.0], co)
                        a_ = _dot([6 * q[2], 2.0, 0.0, 0.0], co)
                    else:
                        pos = ((co[0] * t + co[1]) * t + co[2]) * t + co[3]
                        v = (3 * co[0] * t + 2 * co[1]) * t + co[2]
                        a_ = 6 * co[0] * t + 2 * co[1]
                    cur[sw + ax], vel[sw + ax], acc[sw + ax] = pos, v, a_
                    nxt[sw + ax] = pos + dt * v                  # :2181-2183
    else:
        if i > st.t_end:                                         # :2314-2322
            cur = st.rd(i - 1)
            out["branch"] = "end"
        else:                                                    # :2325-2326
            cur[1], cur[4] = -st.sw0, st.sw0
            out["branch"] = "init"
    st.ring[i % RING] = cur
    st.ring[(i + 1) % RING] = nxt
    st.last = i
    out["right_support"] = rs
    out["rlfoot"] = np.concatenate([cur, vel, acc])
    fin = np.isfinite(out["rlfoot"]).all() and np.isfinite(c[:28]).all() and np.isfinite(c[34:]).all()
    if 0 <= bjxx and bjxx + 1 < NS:
        fin = fin and np.isfinite(c[28:34]).all()
    if not fin and status == R.OK:
        out["status"] = R.NAN
    return out


# ------------------------------------------------------------------ test inputs
T_MAIN = R.T_MAIN
STOP_TICK = 40                          # inside step 2 (ticks 27..54 of the initial schedule)


def t_end_footstep():
    return R.t_end_footstep()


def cases():
    """(name, nlp_ref.rollout keyword arguments, free-running only)."""
    return (("flat", dict(seed=11, batch=R.B_MAIN, ticks=T_MAIN, i0=1), False),
            ("stepped", dict(seed=21, batch=9, ticks=T_MAIN, i0=1), False),
            ("stop", dict(seed=22, batch=9, ticks=T_MAIN, i0=1), False),
            ("end", dict(seed=23, batch=3, ticks=t_end_footstep() + 3, i0=1), True))


def case_inputs(name, batch, ticks):
    """(stepheight[B], stop_walking[T, B]) of a case."""
    sh = np.zeros(batch)
    stop = np.zeros((ticks, batch), np.int32)
    if name == "stepped":
        sh = np.random.default_rng(210).uniform(0.01, 0.03, batch) * np.where(np.arange(batch) % 3 == 2, -1.0, 1.0)
    if name == "stop":
        stop[STOP_TICK - 1:] = 1                                 # tick index t holds loop index i = t + 1
    return sh, stop


OUT_KEYS = ("comz", "comvz", "comaz", "zmp", "dcm", "com_rest", "foot_pos", "foot_vel", "foot_acc")
REC_KEYS = ("rec_ry", "rec_ring")


def keyed(res):
    c, f = res["com_traj"], res["rlfoot"]
    a, b = SLICES["ring"]
    rest = [k for k in range(38) if k not in (2, 5, 8, 23, 26) and not 9 <= k <= 20]
    return dict(comz=c[..., [2]], comvz=c[..., [5]], comaz=c[..., [8, 23, 26]],
                zmp=c[..., [9, 10, 13, 14, 17, 18]], dcm=c[..., [11, 12, 15, 16, 19, 20]], com_rest=c[..., rest],
                foot_pos=f[..., 0:6], foot_vel=f[..., 6:12], foot_acc=f[..., 12:18],
                rec_ry=res["rec2_out"][..., 1:2], rec_ring=res["rec2_out"][..., a:b])


@functools.lru_cache(maxsize=None)
def rollout(name, form=A, teacher=None):
    """Roll a case.  teacher: the A roll-out whose two records re-seed every
    tick of a B roll-out."""
    kw = next(k for n, k, _ in cases() if n == name)
    sform = R.FIRST if form == A else R.SECOND
    sqp = R.rollout(form=sform, **kw) if teacher is None else \
        R.rollout(form=sform, teacher=R._Hashable(teacher["sqp"]), **kw)
    T, Bn = sqp["t_int"].shape
    sh, stop = case_inputs(name, Bn, T)
    p, tp = sqp["params"], dict(TICK_DEFAULTS)
    res = R._Hashable(sqp=sqp, name=name, stepheight=sh, stop=stop, tick_params=tp,
               rec2_in=np.zeros((T, Bn, STATE)), rec2_out=np.zeros((T, Bn, STATE)),
               com_traj=np.zeros((T, Bn, 38)), rlfoot=np.zeros((T, Bn, 18)),
               right_support=np.zeros((T, Bn), np.int32), status=np.zeros((T, Bn), np.int32),
               branch=[[None] * Bn for _ in range(T)], latch=np.zeros((T, Bn), bool),
               gap=np.full((T, Bn), NAN), m4=[[None] * Bn for _ in range(T)], lift_used=np.full((T, Bn), NAN))
    for b in range(Bn):
        st = TickState(sqp["stepwidth"][b], sh[b], p, tp)
        for t in range(T):
            if teacher is not None:
                st.from_record(teacher["rec2_in"][t, b])
            res["rec2_in"][t, b] = st.to_record()
            o = tick_part(st, form, p, tp, int(sqp["t_int"][t, b]), sqp["sched"][t, b], sqp["com"][t, b],
                          int(sqp["status"][t, b]), sqp["record_out"][t, b], bool(stop[t, b]))
            res["rec2_out"][t, b] = st.to_record()
            for k in ("com_traj", "rlfoot", "right_support", "status", "latch", "gap"):
                res[k][t, b] = o[k]
            res["branch"][t][b] = o["branch"]
            res["m4"][t][b] = o["m4"]
            if o["branch"] == "cubic":
                res["lift_used"][t, b] = st.lift[int(sqp["sched"][t, b][3]) - 1]
    return res


def branches_equal(a, b):
    """The landing snap, the double-support test, the _ry_left_right latch and
    the integer outputs, on every robot-tick."""
    return (a["branch"] == b["branch"] and np.array_equal(a["latch"], b["latch"])
            and np.array_equal(a["right_support"], b["right_support"]) and np.array_equal(a["status"], b["status"])
            and np.array_equal(a["sqp"]["sched"], b["sqp"]["sched"])
            and np.array_equal(a["rec2_out"][..., [0, 2, 4]], b["rec2_out"][..., [0, 2, 4]]))


def differences(a, b):
    """{key: per robot-tick largest |A - B| over the key's elements, (T, B)}."""
    ka, kb = keyed(a), keyed(b)
    out = {}
    for k in ka:
        with np.errstate(invalid="ignore"):
            d = np.abs(ka[k] - kb[k])
        d = np.where(np.isfinite(ka[k]) & np.isfinite(kb[k]), d, 0.0)
        assert np.array_equal(np.isfinite(ka[k]), np.isfinite(kb[k])), k
        out[k] = d.max(axis=-1)
    return out


MODES = ("teacher", "free")
OUTLIER = 100.0                        # a robot-tick this far above the key's median gets a bound of its own
# the keys the 4 x 4 system reaches.  t_plan(0) = t_des - dt comes within
# microseconds of t_plan(2) = _ts on the tick after a step the SQP has stretched
# by that much (the landing snap has passed, _bjx1 has not moved on yet): the
# condition number reaches 1e12 and more there, and every formulation returns
# noise of its own.  Only these keys get bounds per robot-tick; the 7 x 7 system
# is benign and its keys are bounded by their pooled spread.
PER_TICK_KEYS = ("foot_pos", "foot_vel", "foot_acc", "rec_ring")


@functools.lru_cache(maxsize=None)
def pair(name, mode):
    """(A roll-out, B roll-out, per robot-tick differences) of a case."""
    a = rollout(name, A)
    b = rollout(name, B, a if mode == "teacher" else None)
    assert branches_equal(a, b), (name, mode)
    return a, b, differences(a, b)


def pooled(mode):
    """{key: (largest, median of the non-zero) A - B difference} pooled over
    the cases of a mode."""
    acc = {}
    for name, _, free_only in cases():
        if mode == "teacher" and free_only:
            continue
        for k, d in pair(name, mode)[2].items():
            acc.setdefault(k, []).append(d.ravel())
    out = {}
    for k, ds in acc.items():
        d = np.concatenate(ds)
        nz = d[d > 0]
        out[k] = (float(d.max()), float(np.median(nz)) if nz.size else 0.0)
    return out


def bound(spreads, key, own):
    """Bound of the GPU's difference from A on one key: 16 x the pooled spread,
    or per robot-tick 16 x max(pooled median, that tick's own A - B difference)
    where one robot-tick lifts the spread OUTLIER x above the median.  spreads:
    {key: (largest, median)}; own: (...,) A - B differences."""
    mx, med = spreads[key]
    if key in PER_TICK_KEYS and med > 0 and mx > OUTLIER * med:
        return 16 * np.maximum(med, own)
    return np.full(np.shape(own), 16 * mx)


# python tests/nlp_tick_ref.py: {key: (largest, median of the non-zero)}
SPREAD_TEACHER = dict(
    comz=(2.232e-14, 3.886e-16),
    comvz=(1.417e-13, 2.167e-15),
    comaz=(1.005e-12, 3.083e-14),
    zmp=(1.218e-14, 5.551e-17),
    dcm=(5.662e-15, 2.776e-17),
    com_rest=(3.553e-15, 2.220e-16),
    foot_pos=(4.446e-02, 6.203e-15),
    foot_vel=(1.323e-01, 1.096e-14),
    foot_acc=(1.265e-01, 3.158e-14),
    rec_ry=(0.000e+00, 0.000e+00),
    rec_ring=(4.446e-02, 6.606e-15),
)
SPREAD_FREE = dict(
    comz=(2.232e-14, 4.441e-16),
    comvz=(1.417e-13, 2.494e-15),
    comaz=(9.933e-13, 3.329e-14),
    zmp=(1.205e-14, 5.551e-17),
    dcm=(7.327e-15, 3.469e-17),
    com_rest=(1.172e-13, 1.554e-15),
    foot_pos=(4.446e-02, 1.657e-14),
    foot_vel=(1.323e-01, 2.296e-13),
    foot_acc=(1.265e-01, 2.755e-12),
    rec_ry=(5.829e-15, 2.776e-17),
    rec_ring=(4.446e-02, 2.005e-06),
)


def conditioning():
    """Smallest |t_plan(0) - t_plan(1)| and largest 4 x 4 condition number over
    the cubic ticks of every case (formulation A, free-running)."""
    gap, cond = math.inf, 0.0
    for name, _, _ in cases():
        a = rollout(name, A)
        g = a["gap"][np.isfinite(a["gap"])]
        if g.size:
            gap = min(gap, float(g.min()))
        for row in a["m4"]:
            for m in row:
                if m is not None:
                    cond = max(cond, float(np.linalg.cond(np.array(m))))
    return gap, cond


if __name__ == "__main__":
    for mode in MODES:
        print("SPREAD_" + mode.upper() + " = dict(")
        for k, (mx, med) in pooled(mode).items():
            print("    %s=(%.3e, %.3e)," % (k, mx, med))
        print(")")
    print("smallest |t_plan(0) - t_plan(1)| %.3e s, largest 4 x 4 condition number %.3e" % conditioning())
