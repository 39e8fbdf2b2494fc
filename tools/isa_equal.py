#!/usr/bin/env python3
"""usage: isa_equal.py <build dir A> <build dir B> [-v]

Are the gfx950 kernels of two builds the same machine code?  For every *.o of both directories (one code object per
translation unit, as tools/kernel_resources.sh reads them) the device code object is unbundled and disassembled
(`llvm-objdump -d --no-show-raw-insn`), the disassembly is split per kernel symbol, and addresses and the absolute branch
targets objdump prints behind them are stripped: what is left depends on the instructions alone, not on where the linker
put the kernel.  Two more things say nothing about a kernel's own instructions and are left out (`normalise`): the displacement
literal of a PC-relative address (the s_add_u32 / s_addc_u32 pair behind a s_getpc_b64 that forms the address of a function that
was not inlined: it moves when code in front of either changes size) and the s_nop padding after a symbol's last instruction.
Symbols of .text that are no kernels (device functions that were not inlined) are compared the same way; an
object without kernels, or a kernel without instructions, is an error.  Next to it, the kernel's metadata note: registers,
spills, LDS, private segment, the kernel-argument offsets and sizes.  Prints `same` or `differs` per kernel name (-v: the first differing lines) and exits non-zero on any
difference, or when a kernel exists on one side only.

The check a refactor of the device code stands on: equal code objects compute the same and run as fast.
Build both sides with the same hipcc and the same flags (`make B=<dir>`).
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size", ".kernarg_segment_size", ".kernarg_segment_align", ".max_flat_workgroup_size",
             ".wavefront_size", ".uses_dynamic_stack")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def device_object(obj, tmp):
    fat, dev = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    tool("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    tool("clang-offload-bundler", "--type=o", f"--input={fat}", "--unbundle", f"--targets={TARGET}", f"--output={dev}")
    return dev


SYMBOL = re.compile(r"^[0-9a-f]+ <([^>]+)>:$")
ADDRESS = re.compile(r"^\s*[0-9a-f]+:\s*")          # (only with raw instructions shown; kept for other objdump versions)
TRAILER = re.compile(r"\s*//\s*[0-9A-Fa-f]+:.*$")   # "// 000000001A2C: <kernel+0x12c>" behind every instruction


PC_RELATIVE_ADD = re.compile(r"^(s_addc?_u32\s+\S+\s+\S+\s+)-?(?:0x[0-9a-fA-F]+|\d+)$")


def normalise(lines):
    """One symbol's instruction lines without what depends on where the linker put it and its callees:
    - the displacement of a PC-relative address (the call of a function that was not inlined): the immediate operands of the
      s_add_u32 / s_addc_u32 pair that follows a s_getpc_b64 become `<pc-relative>`; a register operand there is left alone;
    - the s_nop padding after the symbol's last instruction."""
    out, pair = [], 0
    for line in lines:
        if line.startswith("s_getpc_b64"):
            pair = 2
        elif pair:
            m = PC_RELATIVE_ADD.match(line)
            pair = pair - 1 if m else 0
            if m:
                line = m.group(1) + "<pc-relative>"
        out.append(line)
    while out and out[-1].split()[0] == "s_nop":
        out.pop()
    return out


def kernels_text(dev):
    """{symbol: [instruction lines]} of the code object's .text, normalised"""
    out, cur = {}, None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", dev).splitlines():
        m = SYMBOL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(TRAILER.sub("", ADDRESS.sub("", line)).strip())
    return {name: normalise(lines) for name, lines in out.items()}


def kernels_meta(dev):
    """{kernel name: [metadata lines]} from the NT_AMDGPU_METADATA note: the listed keys and every argument's offset, size and kind"""
    out, cur, in_args, arg = {}, None, False, {}
    entries = []  # (name, lines) in note order; a kernel's .name comes after its .args
    lines = []

    def flush_arg():
        if arg:
            lines.append("arg offset=%s size=%s kind=%s" % (arg.get(".offset"), arg.get(".size"), arg.get(".value_kind")))
            arg.clear()

    for raw in tool("llvm-readelf", "--notes", dev).splitlines():
        m = re.match(r"^(\s*)(- )?(\.[a-z_]+):\s*(.*)$", raw)
        if not m:
            continue
        indent, dash, key, val = len(m.group(1)), m.group(2), m.group(3), m.group(4).strip().strip("'")
        if dash and indent < 6:  # "  - .agpr_count: ..." opens a kernel's entry: its keys, .args among them, follow in alphabetical order
            flush_arg()
            if lines or cur:
                entries.append((cur, lines))
            cur, lines, in_args = None, [], False
        if key == ".args":
            in_args = True
            continue
        if in_args and indent >= 6:
            if dash:
                flush_arg()
            arg[key] = val
            continue
        if in_args:
            flush_arg()
            in_args = False
        if key == ".name" and indent <= 6:
            cur = val
        elif key in META_KEYS:
            lines.append(f"{key}={val}")
    flush_arg()
    if lines or cur:
        entries.append((cur, lines))
    for name, ls in entries:
        if name:
            out[name] = ls
    return out


def read_build(directory):
    text, meta = {}, {}
    objs = sorted(f for f in os.listdir(directory) if f.endswith(".o"))
    if not objs:
        sys.exit(f"{directory}: no *.o")
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            dev = device_object(os.path.join(directory, o), tmp)
            m = kernels_meta(dev)
            t = kernels_text(dev)
            if not m:
                sys.exit(f"{directory}/{o}: no kernel in the metadata note (has the llvm-readelf format changed?)")
            for name in sorted(set(m) | set(t)):  # kernels, and whatever else .text holds (device functions that were not inlined)
                if name in m and not t.get(name):
                    sys.exit(f"{directory}/{o}: kernel {name} has no instructions in the disassembly")
                key = f"{o}:{name}" if name in text else name
                meta[key] = m.get(name, ["(no kernel: a device function)"])
                text[key] = t[name]
    return text, meta


def main(argv):
    verbose = "-v" in argv
    dirs = [a for a in argv if not a.startswith("-")]
    if len(dirs) != 2:
        sys.exit(__doc__)
    (ta, ma), (tb, mb) = read_build(dirs[0]), read_build(dirs[1])
    bad = 0
    for name in sorted(set(ta) | set(tb)):
        if name not in ta or name not in tb:
            print(f"{name}: only in {dirs[0] if name in ta else dirs[1]}")
            bad += 1
            continue
        same_text, same_meta = ta[name] == tb[name], ma[name] == mb[name]
        if same_text and same_meta:
            print(f"{name}: same")
            continue
        bad += 1
        print(f"{name}: differs ({', '.join(w for w, s in (('code', same_text), ('metadata', same_meta)) if not s)})")
        if verbose:
            for what, a, b in (("code", ta[name], tb[name]), ("metadata", ma[name], mb[name])):
                for line in list(difflib.unified_diff(a, b, lineterm="", n=0))[2:22]:
                    print(f"    {what} {line}")
    print(f"{len(set(ta) | set(tb))} kernels, {bad} differ")  # (device functions left in .text are compared and counted too)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
