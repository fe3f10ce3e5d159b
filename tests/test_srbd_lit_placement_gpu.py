"""The placement state of the one-wave literal kernel on the device
(qloco_srbd_solve_placed): it changes which workgroup solves
an instance and nothing else, so every output array is byte-equal to a call
without it, whatever the state holds.

Reference: the same solver with placement=False, once per shape, shared and
read-only.  The bound is equality of bytes (the arithmetic of an instance
and the index of its outputs do not depend on the order).

Shapes: N = 3 mixed and N = 10 trot at B = 29 and B = 64.  spec.reserved[1]
sets the SIMD count S the placement assumes, so these small batches are
placed batches (S < B <= 4 S): S = 8 at B = 29 = 3 S + 5, a partial last row
of workgroups, and S = 16 at B = 64 = 4 S, a full one.  (B = 64 at S = 8 is
eight rows, more than the four that are resident: there the state must stay
untouched, which test_state_untouched_off_the_placed_path checks.)  One case
runs with the device's own S."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from test_srbd_gpu import SEED, _dev  # noqa: E402

from quadrupedal_loco_amd import _lib, srbd  # noqa: E402

FIELDS = ("u0", "u", "status", "iters", "rho_updates", "obj")
SHAPES = [(3, "mixed", 29, 8), (3, "mixed", 64, 16), (10, "trot", 29, 8), (10, "trot", 64, 16)]
HEADER = 4  # int32 words before hint[]


def _solver(N, simds, placement):
    s = srbd.BatchedConvexMpc(horizon=N, literal_full_qp=1, placement=placement)
    s.spec.reserved[1] = simds
    return s


def _bytes(out):
    return {f: getattr(out, f).cpu().numpy().view(np.uint8).copy() for f in FIELDS}


@functools.lru_cache(maxsize=None)
def _reference(N, gait, B, seed=SEED):
    """Inputs on the device and the outputs of a call without a placement
    state, as bytes (computed once per shape, read-only)."""
    dev = _dev()
    args = tuple(torch.from_numpy(a).to(dev) for a in srbd.generate(seed, N, B, gait))
    out = _solver(N, 0, False).solve(*args, full=True)
    torch.cuda.synchronize()
    ref = _bytes(out)
    for v in ref.values():
        v.setflags(write=False)
    return args, ref


def _assert_same(out, ref, where):
    torch.cuda.synchronize()
    got = _bytes(out)
    for f in FIELDS:
        assert np.array_equal(got[f], ref[f]), (where, f)


def _state(solver, B):
    dev = _dev()
    return solver.place_state(B, dev, torch.cuda.current_stream(dev).cuda_stream)


def _class(hint, check):
    return np.clip(np.maximum(hint.astype(np.int64), 0) // max(check, 1), 0, 255)


def _check_state(state, B, S, iters, check):
    """ready word, hint == iters, order a permutation equal to the host
    function's up to the order inside a class."""
    w = state.cpu().numpy()
    assert w[0] == B and not w[1:HEADER].any()
    hint, order = w[HEADER:HEADER + B], w[HEADER + B:]
    assert np.array_equal(hint, iters)
    assert np.array_equal(np.sort(order), np.arange(B))
    host = np.zeros(B, np.int32)
    assert _lib.lib().qloco_srbd_place_order_host(B, S, check, _lib.ptr(np.ascontiguousarray(hint)),
                                                  _lib.ptr(host)) == 0
    cls = _class(hint, check)
    assert np.array_equal(cls[order], cls[host])
    return order


@pytest.mark.parametrize("N,gait,B,S", SHAPES)
def test_outputs_byte_equal_with_any_state(N, gait, B, S):
    args, ref = _reference(N, gait, B)
    iters = ref["iters"].view(np.int32)
    # precondition, on the reference alone: the order is not the identity
    assert len(np.unique(iters)) >= 3, np.unique(iters)
    solver = _solver(N, S, True)
    check = solver.spec.check_termination
    out = solver.solve(*args, full=True)
    _assert_same(out, ref, "first call, zero state")
    state = _state(solver, B)
    order = _check_state(state, B, S, iters, check)
    assert not np.array_equal(order, np.arange(B))
    solver.solve(*args, full=True)
    out = solver.solve(*args, full=True)
    _assert_same(out, ref, "third call")
    _check_state(state, B, S, iters, check)
    # another batch of the same size in between: its counts order this one
    args2, ref2 = _reference(N, gait, B, SEED + 1)
    out = solver.solve(*args2, full=True)
    _assert_same(out, ref2, "other batch")
    out = solver.solve(*args, full=True)
    _assert_same(out, ref, "after another batch")
    # garbage hints under a valid ready word and order
    rng = np.random.default_rng(B + N)
    w = np.zeros(HEADER + 2 * B, np.int32)
    w[0] = B
    w[HEADER:HEADER + B] = rng.integers(-2 ** 31, 2 ** 31 - 1, B, dtype=np.int64).astype(np.int32)
    w[HEADER + B:] = rng.permutation(B).astype(np.int32)
    state.copy_(torch.from_numpy(w))
    out = solver.solve(*args, full=True)
    _assert_same(out, ref, "garbage hints")
    _check_state(state, B, S, iters, check)


def _solve_placed_raw(spec, args, state, warm=None):
    """qloco_srbd_solve_placed itself, with the caller's state."""
    dev = _dev()
    B = args[0].shape[0]
    u0 = torch.empty((B, 12), dtype=torch.float32, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().qloco_srbd_solve_placed(
        C.byref(spec), B, p(args[0]), p(args[1]), p(args[2]), p(args[3]), p(u0), None, None, None,
        None, None, p(warm), 4 * spec.horizon, p(state),
        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "qloco_srbd_solve_placed")
    torch.cuda.synchronize()
    return u0


def test_state_untouched_off_the_placed_path():
    """B <= S, B > 4 S, warm_start = 2 and the stance-only reduction ignore
    the pointer: a sentinel pattern survives the call."""
    N, gait = 3, "mixed"
    dev = _dev()
    sentinel = 0x5A5A5A5A
    cases = [("B <= S", 8, dict(), 8), ("B > 4 S", 64, dict(), 8), ("warm_start 2", 29, dict(warm_start=2), 8),
             ("reduced", 29, dict(literal_full_qp=0), 8)]
    for name, B, over, S in cases:
        args, _ = _reference(N, gait, B)
        spec = srbd.default_spec(horizon=N, **{"literal_full_qp": 1, **over})
        spec.contacts_per_step = 1
        spec.reserved[1] = S
        state = torch.full((HEADER + 2 * B,), sentinel, dtype=torch.int32, device=dev)
        warm = (torch.zeros((B, srbd.warm_len(spec)), dtype=torch.float32, device=dev)
                if spec.warm_start else None)
        _solve_placed_raw(spec, args, state, warm)
        assert bool((state == sentinel).all()), name


def test_persistent_solver_passes_no_state():
    N, B = 3, 29
    args, _ = _reference(N, "mixed", B)
    ctl = srbd.PersistentConvexMpc(B, _dev(), horizon=N, literal_full_qp=1)
    ctl.spec.reserved[1] = 8
    ctl.solve(*args)
    torch.cuda.synchronize()
    assert not ctl.placement and not ctl._place


def test_device_simd_count():
    """The device's own S (four SIMDs per compute unit): B = S + 76, 1100 on an
    MI355X, at N = 2."""
    N, gait = 2, "trot"
    S = 4 * torch.cuda.get_device_properties(_dev()).multi_processor_count
    B = S + 76
    args, ref = _reference(N, gait, B)
    iters = ref["iters"].view(np.int32)
    assert len(np.unique(iters)) >= 3
    solver = _solver(N, 0, True)
    out = solver.solve(*args, full=True)
    _assert_same(out, ref, "first call")
    order = _check_state(_state(solver, B), B, S, iters, solver.spec.check_termination)
    assert not np.array_equal(order, np.arange(B))
    out = solver.solve(*args, full=True)
    _assert_same(out, ref, "second call")
