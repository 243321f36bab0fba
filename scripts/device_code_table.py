"""Compare the gfx950 device code of two builds, kernel by kernel.

    python scripts/device_code_table.py PARENT/csrc/_obj HEAD/csrc/_obj > profiles/<name>/device_code.md

For every object file of the two ``csrc/_obj`` directories: the gfx950 code object is pulled out of ``.hip_fatbin``
(llvm-objcopy --dump-section, clang-offload-bundler --unbundle) and one row per kernel symbol states, parent | head: code
size, SHA-256[:16] of the kernel's bytes, registers (the unified VGPR + AGPR allocation, and the AGPRs in it), SGPRs,
VGPR / SGPR spills, private and group segment bytes -- from ``llvm-readelf -S -s`` and the metadata note
(``--notes``).  Sizes, hashes and metadata only: no instruction is looked at.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"]


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def kernels(obj):
    """{kernel symbol: {"size", "sha", metadata fields}} of one host object"""
    if ".hip_fatbin" not in tool("llvm-readelf", "-S", "--wide", obj):
        return {}  # host code only
    with tempfile.TemporaryDirectory() as tmp:
        fb, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code_object")
        tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(tmp, "unused.o"))
        tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb, "--targets=" + TARGET, "--output=" + co)
        image = open(co, "rb").read()
        sections = tool("llvm-readelf", "-S", "--wide", co)
        symbols = tool("llvm-readelf", "-s", "--wide", co)
        notes = tool("llvm-readelf", "--notes", co)
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", sections)
    if not m:
        return {}
    text_addr, text_off = int(m.group(1), 16), int(m.group(2), 16)
    out = {}
    for line in symbols.split("Symbol table '.symtab'")[0].splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[1] != "0000000000000000":
            start = int(f[1], 16) - text_addr + text_off
            out[f[7]] = {"size": int(f[2]), "sha": hashlib.sha256(image[start:start + int(f[2])]).hexdigest()[:16]}
    for block in notes.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name and name.group(1) in out:
            for key in FIELDS:
                out[name.group(1)][key] = int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
    return out


def short(symbol):
    cxxfilt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    if cxxfilt is None:
        return symbol
    name = subprocess.run([cxxfilt, symbol], check=True, capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):  # drop the argument list: cut at the first '(' outside the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def main(parent_dir, head_dir):
    print("| object | kernel | bytes | code size | sha256[:16] | VGPR+AGPR | AGPR | SGPR | VGPR spills | SGPR spills | private | group |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    same = changed = one_sided = 0
    for obj in sorted(set(os.listdir(parent_dir)) | set(os.listdir(head_dir))):
        if not obj.endswith(".o"):
            continue
        sides = [kernels(os.path.join(d, obj)) if os.path.exists(os.path.join(d, obj)) else {} for d in (parent_dir, head_dir)]
        for sym in sorted(set(sides[0]) | set(sides[1])):
            p, h = sides[0].get(sym), sides[1].get(sym)
            identical = p is not None and h is not None and p["sha"] == h["sha"] and p["size"] == h["size"]
            same += identical
            one_sided += p is None or h is None
            changed += not identical and p is not None and h is not None
            cell = lambda key: "%s \\| %s" % tuple("-" if side is None else side.get(key, "?") for side in (p, h))
            print("| %s | `%s` | %s | %s |" % (obj[:-2], short(sym), "same" if identical else "CHANGED" if p and h else "parent only" if p else "head only",
                                               " | ".join(cell(k) for k in ["size", "sha"] + FIELDS)))
    print("\n%d kernels byte-identical, %d changed, %d on one side only (cells: parent \\| head)" % (same, changed, one_sided))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
