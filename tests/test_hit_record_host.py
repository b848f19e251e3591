"""The one-word hit record (device/kernels.h, HitStream) must not cost the kernels that write and read it their occupancy: the
closest-hit wide walk stores the values tri_test has just produced and stays a six-wave kernel, and k_shade gathers one record
instead of two and stays a four-wave kernel.  Read from the code object inside the built libhprt.so; no GPU needed."""
import pytest

from tree_walk_checks import LIBHPRT, kernel_metadata


@pytest.fixture(scope="module")
def kernels(hprt, tmp_path_factory):
    return kernel_metadata(LIBHPRT, tmp_path_factory.mktemp("co_hit_record"))


def _one(kernels, key):
    found = [v for n, v in kernels.items() if key in n]
    assert len(found) == 1, key
    return found[0]


def test_closest_hit_wide_walk_keeps_six_waves(kernels):
    # k_walk4<ANY_HIT = false, PROF = false, INST = false, QUAD = false>: 512 / 6 -> 80 registers
    k = _one(kernels, "k_walk4ILb0ELb0ELb0ELb0E")
    print("k_walk4<closest>: vgpr %d spill %d" % (k[".vgpr_count"], k[".vgpr_spill_count"]))
    assert k[".vgpr_count"] <= 80, k[".vgpr_count"]
    assert k[".vgpr_spill_count"] == 0, k[".vgpr_spill_count"]


@pytest.mark.parametrize("mode,name", [(0, "matte"), (1, "plastic")])
def test_specialised_shading_variants_keep_four_waves(kernels, mode, name):
    # k_shade<MODE, 512 threads, TEX = false, INSTS = false>: 512 / 4 -> 128 registers
    k = _one(kernels, "k_shadeILi%dELi512ELb0ELb0E" % mode)
    print("k_shade<%s>: vgpr %d spill %d" % (name, k[".vgpr_count"], k[".vgpr_spill_count"]))
    assert k[".vgpr_count"] <= 128, k[".vgpr_count"]
    assert k[".vgpr_spill_count"] == 0, k[".vgpr_spill_count"]
