"""Host-side G^-1 horizon tables of the literal QP (qloco_srbd_lit_tables,
quadrupedal_loco_amd/csrc/qloco_srbd_tables.cpp) against a
numpy float64 inverse of alpha K0 + beta K2.  CPU only.

Tolerance: an entry is the float32 cast of a float64 Gauss-Jordan inverse.
The cast is within 2^-24 relative of the float64 value; the float64 inverses
of these SPD blocks (condition <= ~1e5 at N = 20) differ between two
algorithms by <= ~N cond eps64 ~ 1e-10 of the block's largest entry.  So
|tab - ref| <= 2^-23 |ref| + 1e-9 max|ref| (one float32 ulp plus the float64
slack), and the padding entries are exactly zero."""
import ctypes as C

import numpy as np
import pytest

from quadrupedal_loco_amd import _lib, srbd

WEIGHT_SETS = {
    "default": None,  # qloco_srbd_spec_default (Go1)
    "gazebo": srbd.REFERENCE_WEIGHTS["gazebo"],
    "hardware": srbd.REFERENCE_WEIGHTS["hardware"],
}
HORIZONS = [1, 2, 3, 10, 11, 13, 20]


def _spec(N, wset):
    w = WEIGHT_SETS[wset] if wset in WEIGHT_SETS else srbd.REFERENCE_WEIGHTS[wset]
    if w is None:
        return srbd.default_spec(horizon=N)
    return srbd.default_spec(horizon=N, q_weights=w[0], r_weights=w[1])


def _tables(spec, fill=0.0):
    N = spec.horizon
    NT = 10 if N <= 10 else 20
    tab = np.full((NT, NT, 6), fill, np.float32)
    sq = np.full(1, fill, np.float32)
    gmx = np.full(1, fill, np.float32)
    served = np.full(1, -1, np.int32)
    rc = _lib.lib().qloco_srbd_lit_tables(C.byref(spec), _lib.ptr(tab), tab.size, _lib.ptr(sq),
                                          _lib.ptr(gmx), _lib.ptr(served))
    assert rc == 0
    return tab, float(sq[0]), float(gmx[0]), int(served[0])


def _ref_blocks(spec):
    """The six float64 inverses (axis, N, N) and the |S column|^2 factors."""
    N = spec.horizon
    q2 = 2.0 * np.array([np.float32(x) for x in spec.q_weights], np.float64)
    dt2 = float(np.float32(spec.dt)) ** 2
    idx = np.arange(N)
    M = np.maximum(idx[:, None], idx[None, :])
    K0 = (N - M).astype(np.float64)
    K2 = np.zeros((N, N))
    for j in range(N):
        for k in range(N):
            i = np.arange(M[j, k], N)
            K2[j, k] = float(((i - j) * (i - k)).sum())
    qw = q2[6]
    alpha = [1.0, 1.0, q2[8], q2[9], q2[10], q2[11]]
    beta = [dt2 * q2[0] / qw, dt2 * q2[1] / qw, dt2 * q2[2], dt2 * q2[3], dt2 * q2[4], dt2 * q2[5]]
    inv = np.stack([np.linalg.inv(alpha[a] * K0 + beta[a] * K2) for a in range(6)])
    sn2 = np.array([1.0 / qw, 1.0 / qw, 1.0, 1.0, 1.0, 1.0])
    return inv, sn2


@pytest.mark.parametrize("wset", list(WEIGHT_SETS))
@pytest.mark.parametrize("N", HORIZONS)
def test_host_tables_match_float64_inverse(N, wset):
    spec = _spec(N, wset)
    tab, sq, gmx, served = _tables(spec)
    assert served == 1
    inv, sn2 = _ref_blocks(spec)
    NT = tab.shape[0]
    H = N if N <= 10 else (N + 1) // 2          # two waves: the first wave's steps
    cs = [r if r < H else 10 + r - H for r in range(N)]  # column-space position of step r
    assert len(set(cs)) == N and max(cs) < NT
    if N > 10:
        assert cs[H - 1] == H - 1 and cs[H] == 10 and cs[N - 1] == 10 + (N - H) - 1
    live = np.zeros((NT, NT), bool)
    for a in range(6):
        got = tab[np.ix_(cs, cs)][:, :, a].astype(np.float64)
        ref = inv[a]
        tol = 2.0 ** -23 * np.abs(ref) + 1e-9 * np.abs(ref).max()
        err = np.abs(got - ref)
        assert np.all(err <= tol), (a, float((err / tol).max()))
    live[np.ix_(cs, cs)] = True
    assert np.all(tab[~live] == 0.0)            # padding steps: exactly zero
    assert np.all(tab[cs, cs, :] > 0.0)         # SPD blocks: every live step has its diagonal
    q2w = 2.0 * float(np.float32(spec.q_weights[6]))
    assert abs(sq - 1.0 / np.sqrt(q2w)) <= 2.0 ** -23 / np.sqrt(q2w)
    dref = max(float(sn2[a] * np.diag(inv[a]).max()) for a in range(6))
    assert abs(gmx - dref) <= 2.0 ** -22 * dref


def test_host_tables_symmetric_and_deterministic():
    spec = _spec(10, "default")
    t0 = _tables(spec)
    t1 = _tables(spec)
    assert np.array_equal(t0[0], t1[0]) and t0[1:] == t1[1:]
    for a in range(6):  # float64 Gauss-Jordan of a symmetric matrix, cast: symmetric to an ulp
        blk = t0[0][:, :, a].astype(np.float64)
        assert np.all(np.abs(blk - blk.T) <= 2.0 ** -22 * np.abs(blk).max())


@pytest.mark.parametrize("N", [10, 13])
def test_anisotropic_omega_weights_are_not_served(N):
    """q_omega_x != q_omega_y (the reference's isaac set): lambda depends on the
    yaw, the kernel builds the tables per instance and the host writes nothing."""
    spec = _spec(N, "isaac")
    assert spec.q_weights[6] != spec.q_weights[7]
    tab, sq, gmx, served = _tables(spec, fill=7.0)
    assert served == 0
    assert np.all(tab == 7.0) and sq == 7.0 and gmx == 7.0
    one = _spec(N, "default")
    one.q_weights[7] = np.nextafter(np.float32(one.q_weights[6]), np.float32(1.0))
    assert _tables(one)[3] == 0


def test_bad_arguments():
    spec = _spec(10, "default")
    tab = np.zeros(10, np.float32)
    one = np.zeros(1, np.float32)
    srv = np.zeros(1, np.int32)
    L = _lib.lib()
    assert L.qloco_srbd_lit_tables(C.byref(spec), _lib.ptr(tab), tab.size, _lib.ptr(one), _lib.ptr(one),
                                   _lib.ptr(srv)) == 100  # QLOCO_ERR_ARG: gtab too short
    spec.horizon = 21
    big = np.zeros(2400, np.float32)
    assert L.qloco_srbd_lit_tables(C.byref(spec), _lib.ptr(big), big.size, _lib.ptr(one), _lib.ptr(one),
                                   _lib.ptr(srv)) == 4    # QLOCO_BAD_SIZE
