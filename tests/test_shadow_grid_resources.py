"""Resources of k_shadow_grid (csrc/device/shadow_grid.hip), read from the code object inside the shipped libhprt.so as
tests/test_kernel_resources.py reads the walks' (no GPU needed): nothing in scratch, no LDS, and the registers of the occupancy
its launch code sizes the persistent grid for — HPRT_SHADOW_GRID_WAVES = 5 workgroups of 256 threads per CU, 512 / 5 -> 96 (the
kernel would fit seven; five measured fastest)."""
import pytest

from tree_walk_checks import LIBHPRT, kernel_metadata

WAVES = 5      # HPRT_SHADOW_GRID_WAVES


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    found = [v for n, v in kernel_metadata(LIBHPRT, tmp_path_factory.mktemp("co")).items() if "k_shadow_grid" in n]
    assert len(found) == 1
    return found[0]


def test_nothing_in_scratch_and_no_lds(kernel):
    assert kernel[".private_segment_fixed_size"] == 0 and kernel[".vgpr_spill_count"] == 0 and kernel[".sgpr_spill_count"] == 0
    assert kernel[".group_segment_fixed_size"] == 0


def test_registers_fit_the_occupancy_the_launch_code_assumes(kernel):
    assert kernel[".wavefront_size"] == 64 and kernel[".max_flat_workgroup_size"] == 256
    # 512 registers per lane and SIMD, allocated in blocks of 8: five waves get 96 each
    assert kernel[".vgpr_count"] + kernel.get(".agpr_count", 0) <= (512 // WAVES) // 8 * 8
    assert kernel[".sgpr_count"] <= 102
