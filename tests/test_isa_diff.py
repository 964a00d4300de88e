"""tools/isa_diff.py (CPU): the normaliser and the per-symbol splitters on a short canned disassembly and notes block.

The tool answers "are two builds instruction-identical?"; what can go wrong without a GPU or a compiler is its text
handling: addresses and the per-source __hip_cuid_ symbol must not count as differences, an instruction, an encoding or
a register count must, and a change must be pinned on the kernel it is in."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DISASM = """
a.co:\tfile format elf64-amdgpu

Disassembly of section .text:

0000000000001700 <_Z5k_oneILi0EEvPf>:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0                         // 000000001700: C0060080 00000000
\tv_lshlrev_b32_e32 v1, 2, v0                                // 000000001708: 24020082
\ts_cbranch_execnz 65527                                     // 00000000170C: BF89FFF7 <_Z5k_oneILi0EEvPf+0x4>
\ts_endpgm                                                   // 000000001710: BF810000

0000000000001800 <_Z5k_twoPf>:
\tv_mov_b32_e32 v2, 0                                        // 000000001800: 7E040280
\ts_endpgm                                                   // 000000001804: BF810000
"""

NOTES = """
Displaying notes found in: .note
  Owner                Data size \tDescription
  AMDGPU               0x0000023f\tNT_AMDGPU_METADATA (AMDGPU Metadata)
    AMDGPU Metadata:
        ---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
    .group_segment_fixed_size: 1024
    .name:           _Z5k_oneILi0EEvPf
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .vgpr_count:     3
    .vgpr_spill_count: 0
  - .agpr_count:     0
    .name:           _Z5k_twoPf
    .symbol:         _Z5k_twoPf.kd
    .vgpr_count:     3
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
"""


def test_normalise_drops_addresses_and_cuid():
    mod = _load()
    lines = mod.normalise(DISASM + "0000000000002000 <__hip_cuid_bc377877ecb4e91c>:\n")
    assert not any("__hip_cuid_" in l for l in lines)
    assert "\ts_endpgm                                                   // BF810000" in lines
    assert not any("000000001700:" in l for l in lines)
    # the encoding and a branch's relative target survive
    assert any(l.endswith("// BF89FFF7 <_Z5k_oneILi0EEvPf+0x4>") for l in lines)


def test_split_symbols_and_notes():
    mod = _load()
    code = mod.split_symbols(mod.normalise(DISASM))
    assert sorted(code) == ["_Z5k_oneILi0EEvPf", "_Z5k_twoPf"]
    assert len(code["_Z5k_oneILi0EEvPf"]) == 4 and len(code["_Z5k_twoPf"]) == 2
    assert code["_Z5k_twoPf"][0].startswith("v_mov_b32_e32 v2, 0")
    meta = mod.split_notes(mod.normalise(NOTES))
    assert sorted(meta) == ["_Z5k_oneILi0EEvPf", "_Z5k_twoPf"]
    assert any(".group_segment_fixed_size: 1024" in l for l in meta["_Z5k_oneILi0EEvPf"])
    assert not any("amdhsa.target" in l for l in meta["_Z5k_twoPf"])
    assert not any(".sgpr_count" in l for l in meta["_Z5k_twoPf"])


def test_compare_same_under_relocation_and_cuid():
    mod = _load()
    moved = DISASM.replace("0000000000001700", "0000000000002700").replace("000000001700:", "000000002700:")
    moved = moved.replace("000000001708:", "000000002708:") + "0000000000003000 <__hip_cuid_0123456789abcdef>:\n"
    rows = mod.compare(mod.kernels_of_text(DISASM, NOTES), mod.kernels_of_text(moved, NOTES))
    assert [(s, same) for s, same, _ in rows] == [("_Z5k_oneILi0EEvPf", True), ("_Z5k_twoPf", True)]


def _renamed(disasm, notes):
    """k_two as an instance k_two<1> of a template with one more argument: another name (in its notes and in its own
    branch target too), another kernarg layout, the object's trailing padding under it."""
    new = "_Z5k_twoILi1EEvPfPKi"
    disasm = disasm.replace("v_mov_b32_e32 v2, 0  ", "s_cbranch_scc1 2      ").replace("7E040280", "BF850002 <_Z5k_twoPf+0x10>")
    notes = notes.replace("    .name:           _Z5k_twoPf\n", "    .name:           _Z5k_twoPf\n    .sgpr_count:     9\n")
    d2 = disasm.replace("_Z5k_twoPf", new) + "\t...\n"
    n2 = notes.replace("_Z5k_twoPf", new).replace("  - .agpr_count:     0\n    .name:           " + new,
                                                   "  - .agpr_count:     0\n    .args:\n      - .offset:         8\n"
                                                   "    .name:           " + new)
    return disasm, notes, d2, n2, new


def test_compare_renamed_pair():
    mod = _load()
    d1, n1, d2, n2, new = _renamed(DISASM, NOTES)
    a, b = mod.kernels_of_text(d1, n1), mod.kernels_of_text(d2, n2)
    assert any("_Z5k_twoPf+0x10" in l for l in a["_Z5k_twoPf"][0]) and any(".offset" in l for l in b[new][1])
    # unmapped: the kernel is missing on either side
    assert {s: same for s, same, _ in mod.compare(a, b)} == {"_Z5k_oneILi0EEvPf": True, "_Z5k_twoPf": False, new: False}
    # mapped by symbol or by a substring: name, own branch target, kernarg layout and trailing padding do not count
    for old_pat, new_pat in (("_Z5k_twoPf", new), ("k_twoPf", "k_twoILi1E")):
        rows = mod.compare(a, b, [(old_pat, new_pat)])
        assert [(s, same) for s, same, _ in rows] == [(f"_Z5k_twoPf -> {new}", True), ("_Z5k_oneILi0EEvPf", True)]
    # an instruction or a register count of the mapped pair still does
    rows = mod.compare(a, mod.kernels_of_text(d2.replace("s_cbranch_scc1 2", "s_cbranch_scc0 2"), n2), [("k_twoPf", "k_twoILi1E")])
    assert [same for _, same, _ in rows] == [False, True] and any("instructions" in l for l in rows[0][2])
    rows = mod.compare(a, mod.kernels_of_text(d2, n2.replace(".sgpr_count:     9", ".sgpr_count:     10")), [("k_twoPf", "k_twoILi1E")])
    assert [same for _, same, _ in rows] == [False, True] and any("resources" in l for l in rows[0][2])
    # one old kernel may stand in several pairs; a pattern that names no symbol, or several, pairs nothing
    rows = mod.compare(a, b, [("k_twoPf", "k_twoILi1E"), ("k_twoPf", "k_oneILi0E")])
    assert [(s, same) for s, same, _ in rows] == [(f"_Z5k_twoPf -> {new}", True), ("_Z5k_twoPf -> _Z5k_oneILi0EEvPf", False),
                                                  ("_Z5k_oneILi0EEvPf", False)]
    assert mod.resolve("k_", a) is None and mod.resolve("k_three", a) is None and mod.resolve("k_one", a) == "_Z5k_oneILi0EEvPf"
    assert {s: same for s, same, _ in mod.compare(a, b, [("k_", new)])} == {"_Z5k_oneILi0EEvPf": True, "_Z5k_twoPf": False, new: False}


def test_read_map(tmp_path):
    mod = _load()
    path = tmp_path / "renames.txt"
    path.write_text("# old new\nk_twoPf   k_twoILi1E   # the instance\n\nk_a k_b\n")
    assert mod.read_map(str(path)) == [("k_twoPf", "k_twoILi1E"), ("k_a", "k_b")]
    path.write_text("k_twoPf\n")
    try:
        mod.read_map(str(path))
    except ValueError as e:
        assert "OLD NEW" in str(e)
    else:
        raise AssertionError("a line with one word was accepted")


def test_compare_pins_a_difference_on_its_kernel():
    mod = _load()
    base = mod.kernels_of_text(DISASM, NOTES)
    # one register number (and with it the encoding) in k_two
    other = DISASM.replace("v_mov_b32_e32 v2, 0", "v_mov_b32_e32 v3, 0").replace("7E040280", "7E060280")
    rows = mod.compare(base, mod.kernels_of_text(other, NOTES))
    assert {s: same for s, same, _ in rows} == {"_Z5k_oneILi0EEvPf": True, "_Z5k_twoPf": False}
    # the same text with another encoding only
    rows = mod.compare(base, mod.kernels_of_text(DISASM.replace("24020082", "24020083"), NOTES))
    assert {s: same for s, same, _ in rows} == {"_Z5k_oneILi0EEvPf": False, "_Z5k_twoPf": True}
    # a register count in the notes only
    rows = mod.compare(base, mod.kernels_of_text(DISASM, NOTES.replace(".sgpr_count:     12", ".sgpr_count:     14")))
    assert {s: same for s, same, _ in rows} == {"_Z5k_oneILi0EEvPf": False, "_Z5k_twoPf": True}
    assert any("notes" in l for _, same, detail in rows if not same for l in detail)
    # a kernel present on one side only
    only = dict(base)
    del only["_Z5k_twoPf"]
    rows = mod.compare(base, only)
    assert {s: same for s, same, _ in rows} == {"_Z5k_oneILi0EEvPf": True, "_Z5k_twoPf": False}
