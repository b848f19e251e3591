"""Folded repair, host side (no GPU needed): the code object inside the shipped libhprt.so still has k_repair — the speculated vertices
at which a path ends have no later reader — and the fold-on-read in k_shade (one more byte and a selected address per vertex) pushed
none of the material-specialised variants into scratch: they run four waves per SIMD with every value in registers."""
import pytest

from tree_walk_checks import LIBHPRT, kernel_metadata


@pytest.fixture(scope="module")
def kernels(hprt, tmp_path_factory):
    return kernel_metadata(LIBHPRT, tmp_path_factory.mktemp("co"))


def test_k_repair_exists_plain_and_counting(kernels):
    for count in (0, 1):
        assert len([n for n in kernels if "k_repairILb%dE" % count in n]) == 1, count


def test_only_the_generic_shading_variants_have_scratch(kernels):
    shade = {n: v for n, v in kernels.items() if "k_shadeILi" in n}
    assert len(shade) >= 5
    seen = set()
    for n, v in shade.items():
        generic = "k_shadeILi2E" in n
        seen.add(generic)
        if not generic:
            assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0, (n, v[".private_segment_fixed_size"], v[".vgpr_spill_count"])
    assert seen == {True, False}
