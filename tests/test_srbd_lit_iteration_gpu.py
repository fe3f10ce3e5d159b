"""The literal wrench-space kernels after the issue-slot work on the ADMM
iteration and the Gauss-Jordan pivot (the variable's own
wrench row read by its lane address instead of selected from the step's six,
slot 1's rows at an immediate offset from slot 0's, the first rows' lower
bound parked in LDS per segment of iterations instead of rebuilt every
iteration, the LDS members reordered so that one lane register reaches every
per-lane array, the pivot's negated multiplier without a sign flip).

No other test runs the literal kernels with fz_min != 0: with the default
fz_min = 0 the parked lower bound is 0 on every row and a stale or misplaced
one could not show.  So:

1. fz_min = 10, fz_max = 180 against the float64 restatement of the same OSQP
   call given the same spec (srbd_ref.Instance builds the QP with the oracle,
   which honours fz_min), default settings, N = 10 trot, N = 7 mixed, N = 1
   and N = 13 (two-wave).  Preconditions, asserted on the reference alone: a
   stance fz sits at fz_min on some instance, and some instance has a rho
   update, so the parked bound survives a refactorisation.  (Run on the CPU
   before the inputs were fixed: 17 / 48 of 64, 42 / 50 of 64, 11 / 1 of 64
   and 10 / 23 of 32 instances; check-heavy 16 / 53 and 38 / 54 of 64.)
2. the same bounds under the check-heavy settings of
   tests/test_srbd_lit_overhead_gpu.py (a check every 5 iterations, a rho
   estimate every 10): every segment re-parks the bound and the
   factorisation rewrites its LDS in between.  Run on the CPU first, the
   float64 restatement against the float32 emulation of the kernel's solve
   (tools/proto_lit.py, mode wrench32, its rho estimate at the interval of 10,
   64 instances each, fz_min = 10): 0 of 64 one check apart at N = 10 trot
   (mean 57.3 iterations, at most 105) and at N = 7 mixed (mean 56.2, at most
   90), no status differing -- under the 10 % at which the intervals would
   have been lengthened, so the settings stand as given.
3. the wrench-component reads: slot 1 empty (N = 1, 5), part valid (N = 6)
   and full (N = 10), and both waves of the two-wave kernel (N = 11, 20).
   Byte equality of u0 / obj between one 37-iteration segment and 37 segments
   of one iteration, and of every output of instance 0 solved alone against
   solved in the batch.
4. the pivots: the shapes of test_cold_solve (N = 1, 3, 7, 10: fewer than 60
   pivots, odd N) with the host G^-1 tables and the in-kernel ones, against
   the restatement.

Bounds: those of the literal parity tests -- status equal; iteration counts
equal or one termination check apart, equal on >= 90 % of instances; |du0|
inside U0Bound."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import oracle_lib as O  # noqa: E402
from srbd_ref import Instance  # noqa: E402
from test_srbd_gpu import SEED, U0Bound, _dev  # noqa: E402
from test_srbd_lit_overhead_gpu import CHECK_HEAVY, SAME_SHARE  # noqa: E402

from quadrupedal_loco_amd import srbd  # noqa: E402

FZ_MIN, FZ_MAX = 10.0, 180.0
AT_BOUND = 0.05  # N: a force this close to fz_min counts as held by the bound (eps_abs = 1e-3 solves)
FIELDS = ("u0", "status", "iters", "rho_updates", "obj")


@functools.lru_cache(maxsize=None)
def _reference(N, gait, count, fz, settings):
    """Inputs and the float64 restatement's (u0, status, iters) per instance,
    its fz over the stance (step, leg) pairs and its rho update counts;
    computed once per (shape, bounds, settings), shared and read-only."""
    x0, xr, ft, ct = srbd.generate(SEED, N, count, gait)
    sp = O.srbd_spec(N=N, **dict(fz))
    u0 = np.zeros((count, 12))
    st = np.zeros(count, np.int64)
    it = np.zeros(count, np.int64)
    ru = np.zeros(count, np.int64)
    fz_low = np.full(count, np.inf)  # the smallest stance fz of the instance
    for b in range(count):
        xf, info = Instance(sp, x0[b], xr[b], ft[b], ct[b]).admm_full(**dict(settings))
        u0[b], st[b], it[b], ru[b] = xf[:12], info.status, info.iters, info.rho_updates
        stance = np.asarray(ct[b]).reshape(-1)[:4 * N] > 0
        if stance.any():
            fz_low[b] = xf[2::3][stance].min()
    for a in (x0, xr, ft, ct, u0, st, it, ru, fz_low):
        a.setflags(write=False)
    return (x0, xr, ft, ct), (u0, st, it), ru, fz_low


def _compare(u0, status, iters, ref, check_every, where):
    ru0, rst, rit = ref
    dit = np.abs(iters.astype(np.int64) - rit)
    same = dit == 0
    du0 = np.abs(u0.astype(np.float64) - ru0).max(axis=1)
    print("%s: status equal %d / %d, same check %d, one apart %d, further %d, max |du0| same %.3g apart %.3g" % (
        where, int((status == rst).sum()), len(same), int(same.sum()), int((dit == check_every).sum()),
        int((dit > check_every).sum()), du0[same].max() if same.any() else 0.0,
        du0[~same].max() if (~same).any() else 0.0))
    assert np.array_equal(status.astype(np.int64), rst), (where, status, rst)
    assert np.all(same | (dit == check_every)), (where, np.unique(dit))
    bound = U0Bound()
    for b in range(len(same)):
        bound.add(float(du0[b]), bool(same[b]), (where, b))
    bound.check()
    assert same.sum() >= SAME_SHARE * len(same), (where, int(same.sum()))


def _run(N, gait, count, flag, fz, **settings):
    inputs, ref, ru, fz_low = _reference(N, gait, count, tuple(sorted(fz.items())), tuple(sorted(settings.items())))
    if fz:  # the preconditions, on the reference alone
        assert np.any(np.abs(fz_low - fz["fz_min"]) <= AT_BOUND), (N, gait, "no stance fz at fz_min", fz_low.min())
        assert np.any(ru >= 1), (N, gait, "no rho update")
    dev = _dev()
    solver = srbd.BatchedConvexMpc(horizon=N, literal_full_qp=1, **fz, **settings)
    solver.spec.reserved[0] = flag
    assert srbd.route(solver.spec) == (1 if N <= 10 else 2)  # literal one-wave / two-wave
    out = solver.solve(*(torch.from_numpy(np.array(a)).to(dev) for a in inputs), full=True)
    torch.cuda.synchronize()
    _compare(out.u0.cpu().numpy(), out.status.cpu().numpy(), out.iters.cpu().numpy(), ref,
             int(solver.spec.check_termination), (N, gait, flag, fz, settings))


@pytest.mark.parametrize("N,gait,B", [(10, "trot", 64), (7, "mixed", 64), (1, "trot", 64), (13, "trot", 32)])
def test_fz_min_matches_restatement(N, gait, B):
    """A non-zero lower bound on the z rows, default settings."""
    _run(N, gait, B, 0, dict(fz_min=FZ_MIN, fz_max=FZ_MAX))


@pytest.mark.parametrize("N,gait", [(10, "trot"), (7, "mixed")])
def test_fz_min_check_heavy(N, gait):
    """The bound re-parked by every five-iteration segment, the factorisation
    rewriting its LDS every few of them (module docstring, 2)."""
    _run(N, gait, 64, 0, dict(fz_min=FZ_MIN, fz_max=FZ_MAX), **CHECK_HEAVY)


def _solve(solver, host, rows=None):
    dev = _dev()
    args = [torch.from_numpy(np.ascontiguousarray(a if rows is None else a[rows])).to(dev) for a in host]
    out = solver.solve(*args)
    torch.cuda.synchronize()
    return {k: getattr(out, k).cpu().numpy() for k in FIELDS}


def _assert_same(a, b, where, rows=None, fields=FIELDS):
    for k in fields:
        x = a[k] if rows is None else a[k][rows]
        assert x.tobytes() == b[k].tobytes(), (where, k, np.flatnonzero((x != b[k]).reshape(len(x), -1).any(axis=1)))


@pytest.mark.parametrize("N,B", [(1, 64), (5, 64), (6, 64), (10, 64), (11, 32), (20, 16)])
def test_wrench_reads_segments_and_residency(N, B):
    """Slot 1 empty, part valid and full; both waves of the two-wave kernel.
    With fz_min > 0, so the parked bound is carried over the segments too."""
    host = srbd.generate(SEED, N, B, "trot")
    common = dict(horizon=N, literal_full_qp=1, adaptive_rho=0, max_iter=37, fz_min=FZ_MIN, fz_max=FZ_MAX)
    solver = srbd.BatchedConvexMpc(check_termination=0, **common)
    assert srbd.route(solver.spec) == (1 if N <= 10 else 2)
    one = _solve(solver, host)
    # a check after every iteration that never passes: 37 segments of one
    each = _solve(srbd.BatchedConvexMpc(check_termination=1, eps_abs=1e-12, eps_rel=1e-12, **common), host)
    assert np.all(one["iters"] == 37) and np.all(each["iters"] == 37), (one["iters"], each["iters"])
    _assert_same(one, each, (N, "segments"), fields=("u0", "obj"))
    assert np.all(np.isfinite(one["u0"])) and np.any(one["u0"] != 0.0), N
    # instance 0 alone against instance 0 in the batch, default settings
    solver = srbd.BatchedConvexMpc(horizon=N, literal_full_qp=1, fz_min=FZ_MIN, fz_max=FZ_MAX)
    _assert_same(_solve(solver, host), _solve(solver, host, slice(0, 1)), (N, "instance 0 alone"), slice(0, 1))


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("gait", ["trot", "mixed"])
@pytest.mark.parametrize("N", [1, 3, 7, 10])
def test_pivots_match_restatement(N, gait, flag):
    """Fewer than 60 pivots (the k >= nc early-out), odd N, both table paths."""
    _run(N, gait, 64, flag, {})
