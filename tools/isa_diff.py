#!/usr/bin/env python3
"""isa_diff.py A B: are the gfx950 kernels of two build directories instruction-identical?

For every *.o present in both directories: the gfx950 code object (llvm-objcopy --dump-section=.hip_fatbin, then
clang-offload-bundler --unbundle, the route of tests/test_isa_guard.py), its disassembly (llvm-objdump -d) and its
code-object notes (llvm-readelf --notes: registers, LDS, scratch, spills per kernel).  Instruction addresses and the
lines naming the per-source __hip_cuid_<hash> symbol are dropped; what is left is compared per kernel symbol.
Prints `same` or `DIFF` per symbol and exits 1 on any difference (2: a directory holds no objects).  It judges
nothing beyond equality.

A kernel that was renamed is paired by hand: --map OLD=NEW (repeatable) or --map-file FILE (lines `OLD NEW`, `#`
comments), each side a symbol or a substring that names exactly one symbol of an object of its side; one symbol may
stand in several pairs (a kernel that became two instances).  A mapped pair is compared by its instructions (its own
name in branch targets aside) and, of the notes, by the register, LDS, scratch and spill fields only: the name, the
symbol and the kernarg layout differ by design.

    python tools/isa_diff.py <parent checkout>/csrc/build <this checkout>/csrc/build
    python tools/isa_diff.py <parent checkout>/csrc/build_debug <this checkout>/csrc/build_debug     (make DEBUG=1)
    python tools/isa_diff.py --map k_stream_specENS=k_stream_specILi1ELb0E --map-file renames.txt A B
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("AVSE_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SYMBOL = re.compile(r"^[0-9a-f]+ <([^>]+)>:\s*$")
ADDRESS = re.compile(r"//\s*[0-9A-Fa-f]+:")          # "// 000000001700: C00E0500" -> "// C00E0500"
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
KERNEL_ENTRY = re.compile(r"^  - \.")                 # first key of one amdhsa.kernels entry
KERNEL_NAME = re.compile(r"^\s+\.name:\s+(\S+)")
# the note fields a renamed kernel is still held to
RESOURCE = re.compile(r"^\s+\.(agpr_count|sgpr_count|vgpr_count|sgpr_spill_count|vgpr_spill_count|"
                      r"group_segment_fixed_size|private_segment_fixed_size|uses_dynamic_stack):")


def normalise(text):
    """Disassembly or notes text -> lines without instruction addresses, __hip_cuid_ lines and trailing blanks."""
    out = []
    for line in text.splitlines():
        if CUID.search(line):
            continue
        line = ADDRESS.sub("//", line).rstrip()
        if line:
            out.append(line)
    return out


def split_symbols(lines):
    """Normalised disassembly lines -> {symbol: [instruction lines]} (lines before the first symbol are dropped)."""
    out, cur = {}, None
    for line in lines:
        m = SYMBOL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith("Disassembly of section"):
            cur = None
        elif cur is not None:
            cur.append(line.strip())
    return out


def split_notes(lines):
    """Normalised `llvm-readelf --notes` lines -> {kernel name: [the lines of its amdhsa.kernels entry]}."""
    out, entry = {}, None
    for line in lines + ["end"]:
        if KERNEL_ENTRY.match(line) or not line.startswith("  "):
            if entry:
                names = [m.group(1) for m in map(KERNEL_NAME.match, entry) if m]
                if names:
                    out[names[0]] = entry
            entry = [line] if KERNEL_ENTRY.match(line) else None
        elif entry is not None:
            entry.append(line)
    return out


def code_object(obj, tmp):
    """The object's gfx950 code object, or None for a host-only object."""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, os.path.basename(obj) + ".co")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], capture_output=True, text=True)
    if r.returncode != 0 and "not found" in r.stderr:
        return None
    r.check_returncode()
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}",
                    f"--output={co}", "--unbundle"], check=True, capture_output=True)
    return co


def kernels_of_text(disasm, notes):
    """{symbol: (instruction lines, note lines)} from `llvm-objdump -d` and `llvm-readelf --notes` output."""
    code, meta = split_symbols(normalise(disasm)), split_notes(normalise(notes))
    return {s: (code.get(s, []), meta.get(s, [])) for s in sorted(set(code) | set(meta))}


def kernels(obj, tmp):
    """{symbol: (instruction lines, note lines)} of one object's gfx950 code."""
    co = code_object(obj, tmp)
    if co is None:
        return {}
    run = lambda *cmd: subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    return kernels_of_text(run(f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co),
                           run(f"{LLVM}/llvm-readelf", "--notes", co))


def _detail(pairs):
    detail = []
    for what, x, y in pairs:
        if x != y:
            d = [l for l in difflib.unified_diff(x, y, "A", "B", lineterm="", n=0) if not l.startswith(("---", "+++"))]
            detail += [f"{what}: {sum(l[0] in '+-' for l in d)} lines differ"] + d[:12]
    return detail


def resolve(pattern, symbols):
    """The one symbol `pattern` names (itself, or as a substring), or None when it names none or several."""
    if pattern in symbols:
        return pattern
    hits = [s for s in symbols if pattern in s]
    return hits[0] if len(hits) == 1 else None


def compare(ka, kb, renames=()):
    """[(symbol or "old -> new", same, detail lines)]: the pairs of `renames` ((old, new) patterns, see resolve) that
    both sides hold, then the union of the symbols of two kernels() results that stand in no such pair."""
    rows, paired_a, paired_b = [], set(), set()
    for old, new in renames:
        sa, sb = resolve(old, ka), resolve(new, kb)
        if sa is None or sb is None:
            continue
        paired_a.add(sa)
        paired_b.add(sb)
        # (a closing "...": the section's trailing padding, which the disassembler prints under the object's last kernel)
        own = lambda sym, lines: [l.replace(sym, "<self>") for l in (lines[:-1] if lines[-1:] == ["..."] else lines)]
        res = lambda lines: [l.strip() for l in lines if RESOURCE.match(l)]
        detail = _detail((("instructions", own(sa, ka[sa][0]), own(sb, kb[sb][0])),
                          ("resources", res(ka[sa][1]), res(kb[sb][1]))))
        rows.append((f"{sa} -> {sb}", not detail, detail))
    in_a, in_b = set(ka) - paired_a, set(kb) - paired_b
    for s in sorted(in_a | in_b):
        if s not in in_a or s not in in_b:
            rows.append((s, False, ["only in " + ("A" if s in in_a else "B")]))
            continue
        detail = _detail((("instructions", ka[s][0], kb[s][0]), ("notes", ka[s][1], kb[s][1])))
        rows.append((s, not detail, detail))
    return rows


def read_map(path):
    """[(old, new)] of a rename file: one `OLD NEW` per line, blank lines and `#` comments skipped."""
    out = []
    with open(path) as f:
        for line in f:
            words = line.split("#")[0].split()
            if len(words) == 2:
                out.append((words[0], words[1]))
            elif words:
                raise ValueError(f"{path}: expected `OLD NEW`, got {line.rstrip()!r}")
    return out


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="pair a renamed kernel (repeatable)")
    ap.add_argument("--map-file", action="append", default=[], metavar="FILE", help="lines `OLD NEW`")
    ap.add_argument("a")
    ap.add_argument("b")
    args = ap.parse_args(argv[1:])
    a, b = args.a, args.b
    renames = [tuple(m.split("=", 1)) for m in args.map if "=" in m]
    if len(renames) != len(args.map):
        print("--map takes OLD=NEW")
        return 2
    for path in args.map_file:
        renames += read_map(path)
    used = set()
    names = sorted(set(f for f in os.listdir(a) if f.endswith(".o")) & set(f for f in os.listdir(b) if f.endswith(".o")))
    if not names:
        print("no object file present in both directories")
        return 2
    ndiff = nsym = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for name in names:
            ka, kb = kernels(os.path.join(a, name), ta), kernels(os.path.join(b, name), tb)
            used |= {r for r in renames if resolve(r[0], ka) is not None and resolve(r[1], kb) is not None}
            for sym, same, detail in compare(ka, kb, renames):
                nsym += 1
                ndiff += not same
                print(f"{'same' if same else 'DIFF'}  {name}  {sym}")
                for line in detail:
                    print("        " + line)
    for old, new in renames:
        if (old, new) not in used:
            ndiff += 1
            print(f"DIFF  --map {old}={new}: names no pair of symbols (none, or several, on a side)")
    print(f"{nsym} kernel symbols in {len(names)} objects: {ndiff} differ")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
