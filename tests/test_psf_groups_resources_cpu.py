"""CPU: k_mon_psf of the last build (optable_amd/csrc/build/optable_hip.o, cross-compiled for gfx950) by its code-object metadata
alone.  The two partition passes of ot_monitor_psf_groups_many live inside it behind one launch-uniform branch, and the sum must not
pay for them: the kernel keeps the 51,200 bytes of static LDS the sum declares (the passes' counters lie in it), takes no more
registers than before the passes existed (400, 144 of them accumulation registers), and has no scratch and no vector spill."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
OBJECT = os.path.join(ROOT, "optable_amd", "csrc", "build", "optable_hip.o")


@pytest.fixture(scope="module")
def psf_kernel():
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
        if re.match(r"_Z9k_mon_psfPK", name):
            found.append({key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) for key in (
                "agpr_count", "vgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert len(found) == 1, found  # one kernel: the partition is two modes of it, not two symbols
    return found[0]


def test_static_lds_is_the_sums(psf_kernel):
    assert psf_kernel["group_segment_fixed_size"] == 51200, psf_kernel


def test_no_more_registers_than_the_sum_alone(psf_kernel):
    assert psf_kernel["vgpr_count"] <= 400 and psf_kernel["agpr_count"] <= 144, psf_kernel


def test_no_scratch_and_no_vector_spill(psf_kernel):
    assert psf_kernel["private_segment_fixed_size"] == 0 and psf_kernel["vgpr_spill_count"] == 0, psf_kernel
