"""Resources of k_distant_grid (csrc/device/distant_grid.hip), read from the code object inside the shipped libhprt_dg.so as
tests/test_shadow_grid_resources.py reads k_shadow_grid's (no GPU needed): exactly one kernel, nothing in scratch, no LDS, and the
registers of the occupancy its launch code sizes the persistent grid for — HPRT_DISTANT_GRID_WAVES = 5 workgroups of 256 threads per
CU, 512 / 5 -> 96."""
import os

import pytest

from tree_walk_checks import LIBHPRT, kernel_metadata

WAVES = 5      # HPRT_DISTANT_GRID_WAVES
LIBHPRT_DG = os.path.join(os.path.dirname(LIBHPRT), "libhprt_dg.so")


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    meta = kernel_metadata(LIBHPRT_DG, tmp_path_factory.mktemp("co"))
    assert len(meta) == 1, sorted(meta)
    found = [v for n, v in meta.items() if "k_distant_grid" in n]
    assert len(found) == 1 and not any("k_shadow_grid" in n for n in meta)
    return found[0]


def test_nothing_in_scratch_and_no_lds(kernel):
    assert kernel[".private_segment_fixed_size"] == 0 and kernel[".vgpr_spill_count"] == 0 and kernel[".sgpr_spill_count"] == 0
    assert kernel[".group_segment_fixed_size"] == 0


def test_registers_fit_the_occupancy_the_launch_code_assumes(kernel):
    assert kernel[".wavefront_size"] == 64 and kernel[".max_flat_workgroup_size"] == 256
    # 512 registers per lane and SIMD, allocated in blocks of 8: five waves get 96 each
    assert kernel[".vgpr_count"] + kernel.get(".agpr_count", 0) <= (512 // WAVES) // 8 * 8
    assert kernel[".sgpr_count"] <= 102
