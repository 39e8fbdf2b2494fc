"""CPU: every lane-per-ray kernel of the last build (optable_amd/csrc/build/inst_fused_f64.o and _f32.o, cross-compiled for gfx950) by
its code-object metadata alone.  The segment loop keeps its counter in a scalar register and advances the ray in place (kernels.h
k_trace_fused, trace_core.h advance): no instantiation pays for that with scratch or a vector spill, no double-precision mirror /
lens (FA) or Snell (FB) kernel takes more vector registers or keeps more scalars in vector lanes than before the change, and the
double-precision Snell kernels, built without a register cap, stay within the 128 registers of four waves per SIMD."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
BUILD = os.path.join(ROOT, "optable_amd", "csrc", "build")

# (vector registers, scalars spilled to vector lanes) of the fp64 FA / FB kernels BEFORE the change (DESIGN.md 4.1 "Segment loop"):
# by preset (24 = FA, 28 = FB), register cap (MINW) and layout; the same with either store kind
BEFORE = {("24", "1", "SegsT"): (134, 2), ("24", "4", "SegsT"): (124, 2), ("24", "1", "SegTiles"): (123, 0), ("24", "4", "SegTiles"): (123, 0),
          ("28", "1", "SegsT"): (152, 8), ("28", "1", "SegTiles"): (152, 0)}
NAME = re.compile(r"_Z13k_trace_fusedI([df])Lj(\d+)ELb([01])ELi([14])ELb([01])E\d+(SegsT|SegTiles)I")


@pytest.fixture(scope="module")
def fused():
    objs = [os.path.join(BUILD, f"inst_fused_{p}.o") for p in ("f64", "f32")]
    if not all(os.path.exists(o) for o in objs):
        import __graft_entry__ as g

        g.build()
    out = []
    for obj in objs:
        assert os.path.exists(obj), "no objects: run `make -C optable_amd/csrc`"
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
            m = NAME.match(field("name"))
            if m:
                out.append({"name": field("name"), "real": m.group(1), "preset": m.group(2), "minw": m.group(4), "layout": m.group(6),
                            "scratch": int(field("private_segment_fixed_size")), "vgpr": int(field("vgpr_count")),
                            "vgpr_spill": int(field("vgpr_spill_count")), "sgpr_spill": int(field("sgpr_spill_count"))})
    assert len(out) == 40, [k["name"] for k in out]  # 16 fp64 + 24 fp32 instantiations (inst_fused.hip)
    return out


def test_no_instantiation_has_scratch_or_vector_spills(fused):
    for k in fused:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k


def test_fp64_mirror_lens_and_snell_kernels_take_no_more_than_before(fused):
    seen = set()
    for k in fused:
        key = (k["preset"], k["minw"], k["layout"])
        if k["real"] == "d" and k["preset"] in ("24", "28"):
            vgpr, sgpr_spill = BEFORE[key]
            assert k["vgpr"] <= vgpr and k["sgpr_spill"] <= sgpr_spill, (k, BEFORE[key])
            seen.add(key)
    assert seen == set(BEFORE)


def test_fp64_snell_kernels_fit_four_waves_per_simd_uncapped(fused):
    ks = [k for k in fused if k["real"] == "d" and k["preset"] == "28"]
    assert len(ks) == 4 and all(k["minw"] == "1" for k in ks)  # two layouts x two store kinds, none built with the cap
    for k in ks:
        assert k["vgpr"] <= 128, k
