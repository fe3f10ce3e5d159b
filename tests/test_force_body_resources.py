"""Register, LDS and scratch budget of the Go1 force-QP kernels with and
without per-robot bodies (csrc/qloco_force.hip, qloco_force_qp.inc; DESIGN.md
§4f), read from the gfx950 code object's metadata as
tests/test_kernel_resources.py does (CPU, no GPU).

force_qp_kernel<8> / <16> are the kernels they were before the rows existed:
249 / 240 VGPRs, 19,776 / 9,888 B of LDS, no scratch -- the figures may not
grow (eight 8-robot blocks per CU rest on the LDS figure).  The rows kernels
must still run two waves per SIMD (64-thread workgroups: <= 256 registers),
spill-free, without scratch, in at most 20,480 / 10,240 B of LDS."""
import pytest

from test_kernel_resources import FORCE_GW16, FORCE_GW8, _kernels, assert_budget

ROWS_GW8 = "_ZN5qloco20force_qp_body_kernelILi8EEEvNS_9ForceArgsEPK16qloco_force_body"
ROWS_GW16 = "_ZN5qloco20force_qp_body_kernelILi16EEEvNS_9ForceArgsEPK16qloco_force_body"
PARENT = {FORCE_GW8: (249, 19776), FORCE_GW16: (240, 9888)}
ROWS_LDS = {ROWS_GW8: 20480, ROWS_GW16: 10240}


@pytest.fixture(scope="module")
def kernels():
    return _kernels()


def test_the_four_kernels_exist(kernels):
    for name in (FORCE_GW8, FORCE_GW16, ROWS_GW8, ROWS_GW16):
        assert name in kernels, [k for k in kernels if "force_qp" in k]
    assert len([k for k in kernels if "force_qp" in k]) == 4   # no further copy


@pytest.mark.parametrize("name", sorted(PARENT))
def test_no_rows_kernels_keep_the_budget_they_had(kernels, name):
    assert_budget(kernels[name], *PARENT[name])


@pytest.mark.parametrize("name", sorted(ROWS_LDS))
def test_rows_kernels_run_two_waves_per_simd(kernels, name):
    assert_budget(kernels[name], 256, ROWS_LDS[name], workgroup=64)


def test_the_servo_kernels_and_the_mark_pass_are_spill_free(kernels):
    names = [n for n in kernels if "servo_glue_kernel" in n or "go1_servo_kernel" in n or "force_body_mark" in n]
    assert len(names) == 4, names
    for n in names:
        assert kernels[n][".vgpr_spill_count"] == 0 and kernels[n][".private_segment_fixed_size"] == 0, n
