"""The three per-robot row builders -- srbd.model_rows, a1qp.body_rows and
qp.force_body_rows -- against one table: shape, dtype and the filled defaults,
what a value may look like (a scalar, the field's own vector, one value or one
vector per robot), what is refused, and the two *_from_srbd builders' input
check.  Host only: numpy and the C ABI's from-params calls, no GPU.

B = 3 is the batch at which a (B,) array and a 3-wide field's own vector look
the same: it is taken as the field's vector, for every robot."""
import ctypes as C

import numpy as np
import pytest

from quadrupedal_loco_amd import _lib, a1qp, qp, srbd

# builder, its ABI fill (function, default parameters, row type), row length, dtype, column table,
# a width-1 field, a vector field, and whether a scalar fills every entry of a vector field
BUILDERS = {
    "srbd": dict(fn=srbd.model_rows, fill="qloco_srbd_model_from_spec", params=srbd.default_spec,
                 ctype=_lib.SrbdModel, length=16, dtype=np.float32, columns=srbd.MODEL_COLUMNS,
                 scalar="mu", vector="inertia", scalar_fills_vector=False),
    "a1qp": dict(fn=a1qp.body_rows, fill="qloco_a1_body_from_params", params=a1qp.default_params,
                 ctype=_lib.A1Body, length=24, dtype=np.float64, columns=a1qp.BODY_COLUMNS,
                 scalar="robot_mass", vector="kd_linear", scalar_fills_vector=True),
    "force": dict(fn=qp.force_body_rows, fill="qloco_force_body_from_params", params=qp.force_params,
                  ctype=_lib.ForceBody, length=16, dtype=np.float64, columns=qp.FORCE_BODY_COLUMNS,
                  scalar="fz_max", vector="momentum", scalar_fills_vector=True),
}
CASES = [(name, B) for name in BUILDERS for B in (3, 5)]


def _defaults(t, B):
    """The rows the C ABI fills from the default parameters (not through the builder)."""
    rows = np.zeros((B, t["length"]), t["dtype"])
    p = t["params"]()
    assert getattr(_lib.lib(), t["fill"])(C.byref(p), B, rows.ctypes.data_as(C.POINTER(t["ctype"]))) == 0
    return rows


def _only(rows, base, t, field, want):
    """`field`'s columns hold `want` (broadcast over robots) and every other column is base's."""
    lo, hi = t["columns"][field]
    assert rows.shape == base.shape and rows.dtype == base.dtype
    assert np.array_equal(rows[:, lo:hi], np.broadcast_to(np.asarray(want, rows.dtype), (len(rows), hi - lo)))
    rest = [c for c in range(rows.shape[1]) if not lo <= c < hi]
    assert rows[:, rest].tobytes() == base[:, rest].tobytes()


@pytest.mark.parametrize("name,B", CASES)
def test_shape_dtype_and_defaults(name, B):
    t = BUILDERS[name]
    base = t["fn"](B)
    assert base.shape == (B, t["length"]) and base.dtype == t["dtype"] and base.flags.c_contiguous
    assert base.tobytes() == _defaults(t, B).tobytes()
    assert np.all(base == base[0]) and np.all(base[:, max(hi for _, hi in t["columns"].values()):] == 0)


def test_default_values():
    assert tuple(qp.force_body_rows(1)[0, :6]) == (12.0, 1e4, 1e3, 10.0, 160.0, 0.25)
    assert tuple(a1qp.body_rows(1)[0, [12, 20, 21, 22]]) == (15.0, 0.7, 0.0, 180.0)
    s = srbd.default_spec()
    assert tuple(srbd.model_rows(1)[0, [0, 10, 11, 12]]) == tuple(
        np.float32([s.mass, s.mu, s.fz_min, s.fz_max]))


@pytest.mark.parametrize("name,B", CASES)
def test_unknown_field_is_named(name, B):
    with pytest.raises(ValueError, match="nonesuch"):
        BUILDERS[name]["fn"](B, nonesuch=1.0)


@pytest.mark.parametrize("name,B", CASES)
def test_width_one_field(name, B):
    t = BUILDERS[name]
    f, base = t["scalar"], t["fn"](B)
    _only(t["fn"](B, **{f: 2.5}), base, t, f, 2.5)                          # a scalar
    per = np.linspace(1.0, 2.0, B)
    _only(t["fn"](B, **{f: per}), base, t, f, per[:, None])                 # (B,): one value per robot
    _only(t["fn"](B, **{f: per[:, None]}), base, t, f, per[:, None])        # (B, 1)
    _only(t["fn"](B, **{f: [4.0]}), base, t, f, 4.0)                        # the field's own 1-vector
    with pytest.raises(ValueError):
        t["fn"](B, **{f: np.ones(B + 1)})


@pytest.mark.parametrize("name,B", CASES)
def test_vector_field(name, B):
    t = BUILDERS[name]
    f, base = t["vector"], t["fn"](B)
    w = t["columns"][f][1] - t["columns"][f][0]
    own = np.arange(w) + 0.5
    _only(t["fn"](B, **{f: own}), base, t, f, own)                          # the field's own vector, every robot
    _only(t["fn"](B, **{f: list(own)}), base, t, f, own)
    per = np.arange(B * w, dtype=np.float64).reshape(B, w)
    _only(t["fn"](B, **{f: per}), base, t, f, per)                          # (B, w): one vector per robot
    if t["scalar_fills_vector"]:
        _only(t["fn"](B, **{f: 7.0}), base, t, f, 7.0)
    else:
        with pytest.raises(ValueError):
            t["fn"](B, **{f: 7.0})
    for bad in (np.ones(w + 1), np.ones(w - 1), np.ones((B + 1, w)), np.ones((B, w + 1))):
        with pytest.raises(ValueError):
            t["fn"](B, **{f: bad})


def test_three_values_for_a_three_wide_field_of_three_robots_are_the_fields_vector():
    v = np.array([9.0, 2.0, 15.0])
    for f in ("kp_linear", "kd_linear", "kp_angular", "kd_angular"):
        r = a1qp.body_rows(3, **{f: v})
        lo, hi = a1qp.BODY_COLUMNS[f]
        assert np.array_equal(r[:, lo:hi], np.tile(v, (3, 1))), f
    r = a1qp.body_rows(3, robot_mass=v)                                     # a width-1 field: per robot
    assert np.array_equal(r[:, 12], v)


@pytest.mark.parametrize("B", [3, 5])
def test_inertia_three_by_three_is_stored_col_major(B):
    base = srbd.model_rows(B)
    M = np.arange(9.0).reshape(3, 3)
    r = srbd.model_rows(B, inertia=M)
    _only(r, base, BUILDERS["srbd"], "inertia", [0.0, 3.0, 6.0, 1.0, 4.0, 7.0, 2.0, 5.0, 8.0])
    _only(srbd.model_rows(B, inertia=M.T.reshape(9)), base, BUILDERS["srbd"], "inertia", r[0, 1:10])
    for bad in (1.0, np.ones(3), np.ones(8), np.ones((3, 2)), np.ones((B + 1, 9))):
        with pytest.raises(ValueError):
            srbd.model_rows(B, inertia=bad)


@pytest.mark.parametrize("from_srbd", [a1qp.body_rows_from_srbd, qp.force_body_rows_from_srbd])
@pytest.mark.parametrize("B", [3, 5])
def test_from_srbd_refuses_what_is_no_model_rows_array(from_srbd, B):
    m = srbd.model_rows(B, mass=np.arange(B) + 9.0)
    assert len(from_srbd(m)) == B
    for bad in (m.astype(np.float64), m[:, :15], m[0], m.reshape(B, 4, 4)):
        with pytest.raises(ValueError, match="model_rows"):
            from_srbd(bad)
