"""CPU: the tiled lane-per-ray kernels of the last build (optable_amd/csrc/build/inst_fused_f64.o, cross-compiled for gfx950), whose
segment stores are one element per lane (kernels.h k_trace_fused, OUT = SegTiles).  The mirror / lens kernel built for four waves
per SIMD (cfg 2's) stays within 128 vector registers with no scratch and no vector spill, and neither it nor the refracting kernel
(cfg 4's) keeps more scalars in vector lanes than with the paired stores (4 and 11)."""
import glob
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
BUILD = os.path.join(ROOT, "optable_amd", "csrc", "build")


@pytest.fixture(scope="module")
def tiled_f64():
    obj = os.path.join(BUILD, "inst_fused_f64.o")
    if not os.path.exists(obj):
        import __graft_entry__ as g

        g.build()
    assert os.path.exists(obj), "no objects: run `make -C optable_amd/csrc`"
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fat}", "--unbundle",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    for block in notes.split("\n  - .agpr_count")[1:]:
        def field(name):
            m = re.search(rf"\.{name}:\s+(\S+)", block)
            return m.group(1) if m else None
        if "8SegTilesIdE" in field("name"):
            out.append({"name": field("name"), "scratch": int(field("private_segment_fixed_size")), "vgpr": int(field("vgpr_count")),
                        "vgpr_spill": int(field("vgpr_spill_count")), "sgpr_spill": int(field("sgpr_spill_count"))})
    assert out
    return out


def _of(kernels, pattern):
    ks = [k for k in kernels if re.match(pattern, k["name"])]
    assert ks, pattern
    return ks


def test_cfg2_kernel_stays_within_four_waves_per_simd(tiled_f64):
    for k in _of(tiled_f64, r"_Z13k_trace_fusedIdLj24ELb1ELi4ELb[01]E8SegTilesIdE"):  # FA, image in LDS, MINW = 4, either store kind
        assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["vgpr_spill"] == 0, k


def test_scalar_spills_do_not_exceed_the_paired_kernels(tiled_f64):
    for k in _of(tiled_f64, r"_Z13k_trace_fusedIdLj24ELb1ELi[14]ELb[01]E8SegTilesIdE"):  # FA (mirrors and lenses): cfg 2
        assert k["sgpr_spill"] <= 4 and k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    for k in _of(tiled_f64, r"_Z13k_trace_fusedIdLj28ELb1ELi1ELb[01]E8SegTilesIdE"):     # FB (+ refraction): cfg 4
        assert k["sgpr_spill"] <= 11 and k["scratch"] == 0 and k["vgpr_spill"] == 0, k
