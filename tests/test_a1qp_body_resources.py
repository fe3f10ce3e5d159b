"""Register, LDS and scratch budget of the two instantiations of a1_qp_kernel
(csrc/qloco_a1qp.hip; DESIGN.md §4e "Per-robot bodies"), read from the gfx950
code object's metadata as tests/test_kernel_resources.py does (CPU, no GPU).

Without rows the kernel is the one it was before the rows existed: 233 VGPRs,
7,424 B of LDS, no scratch -- its figures may not grow.  With rows it must
still run two waves per SIMD (64-thread workgroups: <= 256 registers),
spill-free, without scratch, in at most 8 KB of LDS."""
import pytest

from test_kernel_resources import _kernels

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
    k = kernels[NO_ROWS]
    assert k[".vgpr_count"] + k[".agpr_count"] <= PARENT_VGPRS, (k[".vgpr_count"], k[".agpr_count"])
    assert k[".group_segment_fixed_size"] <= PARENT_LDS, k[".group_segment_fixed_size"]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0
    assert not k.get(".uses_dynamic_stack", False)


def test_rows_instantiation_runs_two_waves_per_simd(kernels):
    k = kernels[ROWS]
    assert k[".vgpr_count"] + k[".agpr_count"] <= 256, (k[".vgpr_count"], k[".agpr_count"])
    assert k[".group_segment_fixed_size"] <= 8192, k[".group_segment_fixed_size"]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0
    assert not k.get(".uses_dynamic_stack", False)
    assert k[".max_flat_workgroup_size"] == 64
