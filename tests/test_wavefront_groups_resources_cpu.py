"""CPU: k_mon_spots of the last build (optable_amd/csrc/build/optable_hip.o, cross-compiled for gfx950) by its code-object metadata
alone.  The wavefront mode's group mode (ot_monitor_wavefront_groups_many) is a fourth loop of that kernel behind a launch-uniform
test, not a kernel: one symbol, no scratch and no vector spill.  Before the mode existed the kernel took 107 vector registers, three
of them the lanes its 161 scalar spills are kept in; with the fourth loop it has 283 scalar spills, which take five, and 109 vector
registers — the vector registers of the loops themselves are as many as before.  109 is pinned, and with it what
matters about it: at most 128, so four workgroups of four waves still fit a compute unit's 512 registers a lane."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
OBJECT = os.path.join(ROOT, "optable_amd", "csrc", "build", "optable_hip.o")
KEYS = ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


@pytest.fixture(scope="module")
def spots_kernel():
    if not os.path.exists(OBJECT):
        import __graft_entry__ as g

        g.build()
    assert os.path.exists(OBJECT), "no objects: run `make -C optable_amd/csrc`"
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", OBJECT, fat])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fat}", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--output={co}"])
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    found = []
    for block in notes.split("\n  - .agpr_count")[1:]:
        block = ".agpr_count" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if re.match(r"_Z11k_mon_spotsPK", name):
            found.append({key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) for key in KEYS})
    assert len(found) == 1, found  # one kernel: the group mode is a mode of it, not a symbol
    return found[0]


def test_no_scratch_and_no_vector_spill(spots_kernel):
    assert spots_kernel["private_segment_fixed_size"] == 0 and spots_kernel["vgpr_spill_count"] == 0, spots_kernel


def test_lds_is_the_launch_s(spots_kernel):
    assert spots_kernel["group_segment_fixed_size"] == 0, spots_kernel  # the rows are dynamic LDS: 32 KB at least, 56 KB at most


def test_vector_registers(spots_kernel):
    assert spots_kernel["agpr_count"] == 0 and spots_kernel["vgpr_count"] <= 109, spots_kernel
    assert 4 * 4 * spots_kernel["vgpr_count"] <= 4 * 512  # four workgroups a compute unit: four waves a SIMD at 128 registers or fewer
