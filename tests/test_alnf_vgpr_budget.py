"""The register budget of the 14-row alignment pass (k_alnf<MODE, 14, false>, csrc/kernels.hip), read from the
built library's code-object notes with the helper of the build gate (__graft_entry__.kernel_resources): resource counts only.

A SIMD has 512 vector registers, given out in steps of 8.  Four waves of the pass at no more than 112 leave 64 for a wave of k_err, k_emit
or k_loopw of another context; at 120 they left 32, room for none.  The count has to come from the source: a pass forced below its natural
size spills, and spill code inside its divergent pop region produced wrong records once -- so no k_alnf instantiation may spill or use
scratch at all."""
import os

import pytest

import __graft_entry__ as entry

LIB = os.path.join(entry.ROOT, "tksm_amd", "libtksmseq.so")
ROWS14 = ("6k_alnfILi0ELi14ELb0EE", "6k_alnfILi1ELi14ELb0EE")        # k_alnf<0, 14, false>, k_alnf<1, 14, false>
ALL = ROWS14 + ("6k_alnfILi0ELi64ELb0EE", "6k_alnfILi1ELi64ELb0EE", "6k_alnfILi0ELi64ELb1EE", "6k_alnfILi1ELi64ELb1EE")


@pytest.fixture(scope="module")
def alnf():
    """{mangled name: resources} of every k_alnf instantiation in the library"""
    assert os.path.exists(LIB), "the library is not built (python __graft_entry__.py)"
    return {n: r for n, r in entry.kernel_resources(LIB).items() if "6k_alnfILi" in n}


def test_every_instantiation_is_in_the_library(alnf):
    for tag in ALL:
        assert sum(tag in n for n in alnf) == 1, (tag, sorted(alnf))
    assert len(alnf) == len(ALL), sorted(alnf)


@pytest.mark.parametrize("tag", ROWS14)
def test_the_14_row_pass_leaves_room_for_a_fifth_wave(alnf, tag):
    (r,) = [r for n, r in alnf.items() if tag in n]
    print(tag, r["vgpr_count"], "VGPRs")
    assert entry.ALNF14_VGPR_LIMIT == 112
    assert r["vgpr_count"] <= 112, r
    allocated = -(-r["vgpr_count"] // 8) * 8
    assert 512 - 4 * allocated >= 64


@pytest.mark.parametrize("tag", ALL)
def test_no_instantiation_spills_or_uses_scratch(alnf, tag):
    (r,) = [r for n, r in alnf.items() if tag in n]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
