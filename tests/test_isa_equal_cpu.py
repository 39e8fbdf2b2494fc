"""CPU: what tools/isa_equal.py treats as equal before it compares two builds of a kernel.  A kernel that calls a function that
was not inlined forms the callee's address relative to the program counter, and the displacement moves whenever code in front of
either changes size; the assembler pads the end of a function with s_nop.  Neither says anything about the kernel's own
instructions.  The listings are written out here: no build is needed."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _normalise():
    spec = importlib.util.spec_from_file_location("isa_equal", os.path.join(ROOT, "tools", "isa_equal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.normalise


# a kernel's tail as llvm-objdump prints it once addresses and trailers are stripped: two calls, then the end
LISTING = """\
s_load_dwordx2 s[4:5], s[0:1], 0x0
v_mul_f64 v[0:1], v[2:3], v[4:5]
s_getpc_b64 s[16:17]
s_add_u32 s16, s16, 0x1a2c
s_addc_u32 s17, s17, 0
s_swappc_b64 s[30:31], s[16:17]
v_add_f64 v[6:7], v[0:1], v[6:7]
s_getpc_b64 s[18:19]
s_add_u32 s18, s18, 0xfffff3d4
s_addc_u32 s19, s19, -1
s_swappc_b64 s[30:31], s[18:19]
s_add_u32 s8, s8, 0x100
global_store_dwordx2 v8, v[6:7], s[4:5]
s_nop 0
s_endpgm
""".splitlines()


def _with(listing, old, new):
    assert sum(line == old for line in listing) == 1, old
    return [new if line == old else line for line in listing]


def test_displacements_and_trailing_padding_compare_equal():
    normalise = _normalise()
    moved = _with(_with(_with(LISTING, "s_add_u32 s16, s16, 0x1a2c", "s_add_u32 s16, s16, 0x2b40"),
                        "s_add_u32 s18, s18, 0xfffff3d4", "s_add_u32 s18, s18, 0x58"), "s_addc_u32 s19, s19, -1", "s_addc_u32 s19, s19, 0")
    padded = moved + ["s_nop 0", "s_nop 0"]
    assert moved != LISTING
    assert normalise(LISTING) == normalise(moved) == normalise(padded)
    # what is left is the listing itself, the four displacement operands replaced and nothing else touched
    left = normalise(LISTING)
    assert len(left) == len(LISTING)
    changed = [(a, b) for a, b in zip(LISTING, left) if a != b]
    assert [a for a, _ in changed] == ["s_add_u32 s16, s16, 0x1a2c", "s_addc_u32 s17, s17, 0", "s_add_u32 s18, s18, 0xfffff3d4", "s_addc_u32 s19, s19, -1"]
    assert all(b.startswith(a.rsplit(" ", 1)[0]) for a, b in changed)
    # a function that ends in padding alone (no s_endpgm: a device function returns through s_setpc_b64)
    callee = ["v_exp_f32_e32 v0, v0", "s_setpc_b64 s[30:31]"]
    assert normalise(callee + ["s_nop 0"] * 5) == normalise(callee) == callee


def test_a_real_operand_still_differs():
    normalise = _normalise()
    base = normalise(LISTING)
    for old, new in (("v_mul_f64 v[0:1], v[2:3], v[4:5]", "v_mul_f64 v[0:1], v[2:3], v[6:7]"),     # another register
                     ("s_load_dwordx2 s[4:5], s[0:1], 0x0", "s_load_dwordx2 s[4:5], s[0:1], 0x8"),   # another kernel-argument offset
                     ("s_add_u32 s8, s8, 0x100", "s_add_u32 s8, s8, 0x140"),                         # an add that follows no s_getpc_b64
                     ("s_add_u32 s16, s16, 0x1a2c", "s_add_u32 s16, s20, 0x1a2c"),                   # the pair's register operands
                     ("s_addc_u32 s17, s17, 0", "s_addc_u32 s17, s17, s21"),                         # a register where the literal stood
                     ("s_nop 0", "s_nop 1"),                                                          # padding INSIDE the function
                     ("s_swappc_b64 s[30:31], s[18:19]", "s_swappc_b64 s[30:31], s[16:17]")):
        assert normalise(_with(LISTING, old, new)) != base, (old, new)
    assert normalise(LISTING[:-1]) != base                 # the last instruction is missing
    assert normalise(LISTING + ["s_endpgm"]) != base      # an instruction after the padding: the padding is no longer trailing
