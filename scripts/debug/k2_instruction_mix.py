"""Instruction mix of one K2 tile, parent against tree, from two `hipcc -S` outputs of particle_net.hip.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize --cuda-device-only -S -o parent.s particle_net.hip
    (the same in this tree -> tree.s; the flags are build.py's for this file)
    python scripts/debug/k2_instruction_mix.py parent.s tree.s [-o profiles/k2_vector/instruction_mix.txt]

A tile is the straight-line stretch of a kernel from its first first-layer MFMA (v_mfma_f32_32x32x2_f32) to its last
f16 MFMA (v_mfma_f32_32x32x16_f16): the pipelined kernels hold exactly one copy of it.  Counted per mnemonic: vector-ALU
(every v_* that is neither an MFMA nor a v_accvgpr move is listed), MFMA, LDS reads and s_nop.  No GPU is needed.
"""
import argparse
import collections
import re
import subprocess
import sys

# the instantiations of the headline step: the measurement launch and the run-table dynamics launch (d = 3), and d = 2
KERNELS = [
    "particle_net_kernel<3, 2, 1, 2, 1, 2, true, false>",
    "particle_net_kernel<3, 3, 0, 2, 1, 2, true, true>",
    "particle_net_kernel<2, 2, 1, 2, 1, 2, true, false>",
    "particle_net_kernel<2, 3, 0, 2, 1, 2, true, true>",
]
FIRST = "v_mfma_f32_32x32x2_f32"
LAST = "v_mfma_f32_32x32x16_f16"
# v_cmp_* and v_cndmask_* come in many spellings (operand class, encoding): one row each
FAMILIES = [("v_cmp_", "v_cmp_*"), ("v_cmpx_", "v_cmp_*"), ("v_cndmask_", "v_cndmask_*")]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernel_bodies(path):
    """{demangled kernel name: [mnemonic, ...]} for every particle_net_kernel in the file"""
    bodies, name, cur = {}, None, None
    label = re.compile(r"^(_Z\w+):")
    with open(path) as f:
        for line in f:
            m = label.match(line)
            if m:
                name, cur = m.group(1), []
                continue
            if name is None:
                continue
            if line.startswith(".Lfunc_end"):
                bodies[name] = cur
                name = None
                continue
            text = line.split(";")[0].strip()
            if not text or text.startswith(".") or text.endswith(":"):
                continue
            cur.append(text.split()[0])
    names = demangle([n for n in bodies if "particle_net_kernel" in n])
    short = {}
    for mangled, full in names.items():
        m = re.search(r"particle_net_kernel<[^>]*>", full)
        if m:
            short[m.group(0)] = bodies[mangled]
    return short


def family(mnemonic):
    for prefix, row in FAMILIES:
        if mnemonic.startswith(prefix):
            return row
    for suffix in ("_e32", "_e64", "_sdwa", "_dpp"):
        if mnemonic.endswith(suffix):
            return mnemonic[: -len(suffix)]
    return mnemonic


def tile_mix(body):
    first = next(i for i, m in enumerate(body) if m.startswith(FIRST))
    last = max(i for i, m in enumerate(body) if m.startswith(LAST))
    valu, other = collections.Counter(), collections.Counter()
    for m in body[first : last + 1]:
        if m.startswith("v_mfma"):
            other["MFMA f16" if m.startswith(LAST) else "MFMA f32"] += 1
        elif m.startswith("v_accvgpr"):
            other["v_accvgpr_*"] += 1
        elif m.startswith("v_"):
            valu[family(m)] += 1
        elif m.startswith("ds_read") or m.startswith("ds_load"):
            other[m] += 1
        elif m == "s_nop":
            other["s_nop"] += 1
    return valu, other


def table(kernel, parent, tree):
    pv, po = tile_mix(parent)
    tv, to = tile_mix(tree)
    lines = [kernel, f"  {'mnemonic':28s} {'parent':>7s} {'tree':>7s} {'change':>7s}"]

    def row(name, a, b):
        lines.append(f"  {name:28s} {a:7d} {b:7d} {b - a:+7d}")

    row("vector-ALU, all", sum(pv.values()), sum(tv.values()))
    for name in sorted(set(pv) | set(tv), key=lambda n: (-max(pv[n], tv[n]), n)):
        row(name, pv[name], tv[name])
    for name in sorted(set(po) | set(to)):
        row(name, po[name], to[name])
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("-o", "--output")
    args = ap.parse_args()
    parent, tree = kernel_bodies(args.parent), kernel_bodies(args.tree)
    head = ("One tile of the pipelined f16x3 K2 kernels, first first-layer MFMA .. last f16 MFMA, per mnemonic.\n"
            "hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize --cuda-device-only -S particle_net.hip, "
            "parent and tree;\nscripts/debug/k2_instruction_mix.py.  "
            "particle_net_kernel<D, NRES, KIND, CT, PREC, WPS, PIPE, RUNS>: KIND 0 dynamics, 1 measurement.\n")
    text = head + "\n" + "\n\n".join(table(k, parent[k], tree[k]) for k in KERNELS) + "\n"
    if args.output:
        with open(args.output, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
