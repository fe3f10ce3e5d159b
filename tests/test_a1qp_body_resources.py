"""Register, LDS and scratch budget of the two instantiations of a1_qp_kernel
(csrc/qloco_a1qp.hip; DESIGN.md §4e "Per-robot bodies"), read from the gfx950
code object's metadata as tests/test_kernel_resources.py does (CPU, no GPU).

Without rows the kernel is the one it was before the rows existed: 233 VGPRs,
7,424 B of LDS, no scratch -- its figures may not grow.  With rows it must
still run two waves per SIMD (64-thread workgroups: <= 256 registers),
spill-free, without scratch, in at most 8 KB of LDS."""
import pytest

from test_kernel_resources import _kernels, assert_budget

NO_ROWS = "_ZN5qloco2a112a1_qp_kernelILb0EEEvNS0_4ArgsE"
ROWS = "_ZN5qloco2a112a1_qp_kernelILb1EEEvNS0_4ArgsE"
PARENT_VGPRS, PARENT_LDS = 233, 7424


@pytest.fixture(scope="module")
def kernels():
    return _kernels()


def test_both_instantiations_exist(kernels):
    assert NO_ROWS in kernels and ROWS in kernels, [k for k in kernels if "a1_qp" in k]
    assert "_ZN5qloco2a112a1_qp_kernelENS0_4ArgsE" not in kernels   # no third copy


def test_no_rows_instantiation_keeps_the_budget_it_had(kernels):
    assert_budget(kernels[NO_ROWS], PARENT_VGPRS, PARENT_LDS)


def test_rows_instantiation_runs_two_waves_per_simd(kernels):
    assert_budget(kernels[ROWS], 256, 8192, workgroup=64)
