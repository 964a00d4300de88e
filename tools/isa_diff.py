#!/usr/bin/env python3
"""isa_diff.py A B: are the gfx950 kernels of two build directories instruction-identical?

For every *.o present in both directories: the gfx950 code object (llvm-objcopy --dump-section=.hip_fatbin, then
clang-offload-bundler --unbundle, the route of tests/test_isa_guard.py), its disassembly (llvm-objdump -d) and its
code-object notes (llvm-readelf --notes: registers, LDS, scratch, spills per kernel).  Instruction addresses and the
lines naming the per-source __hip_cuid_<hash> symbol are dropped; what is left is compared per kernel symbol.
Prints `same` or `DIFF` per symbol and exits 1 on any difference (2: a directory holds no objects).  It judges
nothing beyond equality.

    python tools/isa_diff.py <parent checkout>/csrc/build <this checkout>/csrc/build
    python tools/isa_diff.py <parent checkout>/csrc/build_debug <this checkout>/csrc/build_debug     (make DEBUG=1)
"""
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


def compare(ka, kb):
    """[(symbol, same, detail lines)] over the union of two kernels() results."""
    rows = []
    for s in sorted(set(ka) | set(kb)):
        if s not in ka or s not in kb:
            rows.append((s, False, ["only in " + ("A" if s in ka else "B")]))
            continue
        detail = []
        for what, x, y in (("instructions", ka[s][0], kb[s][0]), ("notes", ka[s][1], kb[s][1])):
            if x != y:
                d = [l for l in difflib.unified_diff(x, y, "A", "B", lineterm="", n=0) if not l.startswith(("---", "+++"))]
                detail += [f"{what}: {sum(l[0] in '+-' for l in d)} lines differ"] + d[:12]
        rows.append((s, not detail, detail))
    return rows


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = argv[1], argv[2]
    names = sorted(set(f for f in os.listdir(a) if f.endswith(".o")) & set(f for f in os.listdir(b) if f.endswith(".o")))
    if not names:
        print("no object file present in both directories")
        return 2
    ndiff = nsym = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for name in names:
            for sym, same, detail in compare(kernels(os.path.join(a, name), ta), kernels(os.path.join(b, name), tb)):
                nsym += 1
                ndiff += not same
                print(f"{'same' if same else 'DIFF'}  {name}  {sym}")
                for line in detail:
                    print("        " + line)
    print(f"{nsym} kernel symbols in {len(names)} objects: {ndiff} differ")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
