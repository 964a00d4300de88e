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
