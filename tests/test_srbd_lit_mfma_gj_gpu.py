"""The one-wave literal SRBD kernels after the Gauss-Jordan rank-1 updates
moved to the matrix cores: lit_invert holds the 64 x 64 matrix
in the accumulator layout of two v_mfma_f32_32x32x1_2b_f32 and converts from
and to the row-per-lane layout with v_permlane32_swap.  Every entry still
receives the one fused multiply-add per pivot it received from the DPP form,
so every output of the kernels -- u0, u, status, iters, rho_updates, obj -- is
byte for byte what the commit before the change computed:
tests/golden/srbd_lit_parent_bits.npz, recorded on an MI355X with that
commit's library by tests/golden/make_srbd_lit_parent_bits.py, which also
holds the cases and how each is run (imported here).

Cases (B = 64, placement off): nc = 60 (every pivot, both accumulator
halves), 36 (pivots cross lane 32), 30 (the second half is padding only), 18
and 6; N = 10 trot with fz_min > 0; two ticks of PersistentConvexMpc (the
warm-start instantiation); per-robot model rows (the _rows kernel).

Preconditions, asserted on the fixture alone: every shape solves on >= 90 % of
its instances, and every N >= 3 shape has an instance with a rho update (a
refactorisation ran: the inverse was taken twice from different matrices) and
at least three distinct iteration counts (an inverse wrong in its last bits
moves some count)."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from test_srbd_gpu import _dev  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "make_srbd_lit_parent_bits", os.path.join(HERE, "golden", "make_srbd_lit_parent_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def fixture():
    with np.load(rec.PATH) as z:
        return {k: z[k] for k in z.files}


def _case(fixture, name):
    pre = name + "/"
    return {k[len(pre):]: v for k, v in fixture.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(rec.CASES))
def test_fixture_exercises_the_inverse(fixture, name):
    want = _case(fixture, name)
    assert rec.preconditions(name, want) is None, (name, rec.preconditions(name, want))
    ticks = 2 if rec.CASES[name][2] == "persistent" else 1
    assert len(want) == 1 + ticks * len(rec.FIELDS), sorted(want)
    assert want["u"].shape == (rec.B, 12 * rec.CASES[name][0])


@pytest.mark.parametrize("name", list(rec.CASES))
def test_outputs_are_the_parents_bytes(fixture, name):
    _dev()
    want = _case(fixture, name)
    got = rec.run_case(name, int(want.pop("seed")))
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in sorted(want):
        differ = np.flatnonzero((got[k] != want[k]).reshape(rec.B, -1).any(axis=1))
        print("%s %s: %d of %d instances differ" % (name, k, len(differ), rec.B))
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (
            name, k, np.flatnonzero((got[k] != want[k]).reshape(rec.B, -1).any(axis=1)))
