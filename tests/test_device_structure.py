"""The board kernels' shared idioms have one definition each (no GPU, no build: regular expressions over csrc).

A second spelling of one of these is how the two board layouts, or two kernels, drift apart bit by bit without any
test noticing before a parity run on a GPU does.
"""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "generalsreinforcementlearning_amd", "csrc")


def _sources():
    """{file name: text without // comments} of every csrc/*.hip and *.hpp"""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        with open(path) as f:
            out[os.path.basename(path)] = re.sub(r"//[^\n]*", "", f.read())
    return out


def _sites(pattern):
    return [(name, m.group(0)) for name, text in _sources().items() for m in re.finditer(pattern, text)]


def test_header_dims_are_unpacked_in_one_place():
    # H_DIMS = W | H<<8 | P<<16 | flags<<24: the P and flags fields are taken apart by unpack_dims alone
    assert [n for n, _ in _sites(r"dims\s*>>\s*16")] == ["gvec_device.hpp"]
    assert [n for n, _ in _sites(r"=\s*dims\s*>>\s*24")] == ["gvec_device.hpp"]
    # ... and put together by pack_hdr alone
    assert [n for n, _ in _sites(r"hflags\s*<<\s*24")] == ["gvec_device.hpp"]


def test_wave_to_item_index_is_written_once():
    # the wave-uniform item of a wavefront, blockIdx.x * WAVES_PER_BLOCK + its wave, is wave_item() of gvec_waves.hpp
    assert [n for n, _ in _sites(r"uni\(\s*\(int\)\s*\(?\s*blockIdx\.x\s*\*\s*WAVES_PER_BLOCK")] == ["gvec_waves.hpp"]
    assert [n for n, _ in _sites(r"threadIdx\.x\s*>>\s*6\)\s*,\s*lane")] == []  # the old prologue's first line
    # ... in 32 and in 64 bits; no unit multiplies blockIdx.x by a waves-per-workgroup constant of its own, and only
    # obs_memory_kernel and categorical_target_kernel spell the index out (with the shared constant: their comments say
    # what the shared call cost them)
    assert ([n for n, _ in _sites(r"blockIdx\.x\s*\*\s*(\(\w+\))?\s*\w*WAVES\w*")]
            == ["gvec_memory.hip", "gvec_qtarget.hip"] + ["gvec_waves.hpp"] * 2)
    assert [n for n, _ in _sites(r"constexpr\s+int\s+\w*WAVES\w*\s*=")] == ["gvec_waves.hpp"]


def test_gym_stage_size_is_written_once():
    assert [n for n, _ in _sites(r"NSLOT\s*\*\s*64\s*\*\s*5")] == ["gvec_device.hpp"]


def test_army_forms_and_ballot_planes_have_one_definition():
    # the narrow / wide choice at a store, and the pair of v_writelane that lands a ballot in a flat plane
    assert [n for n, _ in _sites(r"hflags\s*\|=\s*HF_WIDE")] == ["gvec_device.hpp"]
    assert [n for n, _ in _sites(r"gvec_llvm_writelane\(\(int\)\(uint32_t\)\(ballot\s*>>\s*32\)")] == ["gvec_device.hpp"]
    assert len(_sites(r"gvec_llvm_writelane\([^;]*>>\s*32\)")) == 1
