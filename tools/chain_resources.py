"""Resource usage and fp64 arithmetic of the four chain kernels (k_hmc_run, k_nuts_run, k_rwalk, k_paths_hmc_run), every
instantiation, before and after a change - from the compiler's own text, no GPU needed.  In each of two directories:
   for u in gp_consumers gp_paths; do
     hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
           -o DIR/$u.s bobe_amd/csrc/$u.hip 2> DIR/$u.remarks; done
   python tools/chain_resources.py BEFORE_DIR AFTER_DIR [TABLE]     TABLE defaults to profiles/chain_core_unify_resources.txt

Per kernel: VGPRs, AGPRs, scratch, occupancy and static LDS from the remarks; the instruction count and the count of every
opcode whose name contains `f64` between the kernel's label and its end from the assembly.  Exit status 1 when any scratch is
above 0, or occupancy, static LDS or an f64 opcode count differs between the two."""
import collections
import os
import re
import sys

KERNELS = ("k_hmc_run", "k_nuts_run", "k_rwalk", "k_paths_hmc_run")
FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("scratch", "ScratchSize [bytes/lane]"), ("occ", "Occupancy [waves/SIMD]"),
          ("LDS", "LDS Size [bytes/block]"))


def kernel_of(symbol):
    """('k_rwalk', 'rbf' | 'matern', d cap) of a mangled name, or None"""
    m = re.match(r"_ZN4bobe\d+(k_\w+?)ILi([01])ELi(8|16|32)EEE", symbol)
    if not m or m.group(1) not in KERNELS:
        return None
    return m.group(1), ("rbf", "matern")[int(m.group(2))], int(m.group(3))


def remarks(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = kernel_of(text.split(":", 1)[1].strip())
            if cur:
                out[cur] = {}
        elif cur and ":" in text:
            k, v = text.rsplit(":", 1)
            out[cur][k.strip()] = v.strip()
    return out


def opcodes(path):
    out, cur = {}, None
    for line in open(path):
        if cur is None:
            m = re.match(r"(_ZN4bobe\w+):", line)
            if m and kernel_of(m.group(1)):
                cur = kernel_of(m.group(1))
                out[cur] = collections.Counter()
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"\t([a-z]\w+)", line)
        if m:
            out[cur]["instructions"] += 1
            if "f64" in m.group(1):
                out[cur][m.group(1)] += 1
    return out


def read(directory):
    rem, ops = {}, {}
    for unit in ("gp_consumers", "gp_paths"):
        rem.update(remarks(os.path.join(directory, unit + ".remarks")))
        ops.update(opcodes(os.path.join(directory, unit + ".s")))
    return rem, ops


def main(before, after, table):
    (rb, ob), (ra, oa) = read(before), read(after)
    keys = sorted(rb, key=lambda k: (KERNELS.index(k[0]), k[2], k[1] != "rbf"))
    assert set(rb) == set(ra) == set(ob) == set(oa) and len(keys) == 6 * len(KERNELS), (len(rb), len(ra), len(ob), len(oa))
    lines = ["# the chain kernels before -> after, gfx950, from -Rpass-analysis=kernel-resource-usage and the device assembly",
             "# (tools/chain_resources.py).  f64: the number of instructions whose opcode contains `f64`; `same` = every such opcode",
             "# occurs as often after as before.",
             f"{'kernel':16s} {'family':6s} {'cap':>3s} | {'VGPRs':>9s} | {'AGPRs':>10s} | {'scratch':>7s} | {'occ':>6s} | "
             f"{'static LDS':>12s} | {'instructions':>14s} | f64"]
    bad = []
    for k in keys:
        b, a = rb[k], ra[k]
        cell = {name: f"{b[field]} -> {a[field]}" for name, field in FIELDS}
        fb = {o: c for o, c in ob[k].items() if o != "instructions"}
        fa = {o: c for o, c in oa[k].items() if o != "instructions"}
        diff = {o: (fb.get(o, 0), fa.get(o, 0)) for o in sorted(set(fb) | set(fa)) if fb.get(o, 0) != fa.get(o, 0)}
        f64 = f"{sum(fb.values())} -> {sum(fa.values())} " + ("same" if not diff else "DIFFER " + str(diff))
        lines.append(f"{k[0]:16s} {k[1]:6s} {k[2]:3d} | {cell['VGPRs']:>9s} | {cell['AGPRs']:>10s} | {cell['scratch']:>7s} | "
                     f"{cell['occ']:>6s} | {cell['LDS']:>12s} | {ob[k]['instructions']:6d} -> {oa[k]['instructions']:5d} | {f64}")
        if diff or int(a[FIELDS[2][1]]) or int(b[FIELDS[2][1]]) or any(b[f] != a[f] for _, f in FIELDS[3:]):
            bad.append(k)
    lines.append("")
    lines.append("# per-opcode f64 counts (after)")
    for k in keys:
        lines.append(f"{k[0]} {k[1]} {k[2]}: " + ", ".join(f"{o} {c}" for o, c in sorted(oa[k].items()) if o != "instructions"))
    lines.append("")
    lines.append("every kernel: scratch 0, occupancy, static LDS and every f64 opcode count unchanged" if not bad
                 else "NOT HELD by: " + ", ".join(f"{k[0]}<{k[1]}, {k[2]}>" for k in bad))
    text = "\n".join(lines) + "\n"
    open(table, "w").write(text)
    print(text, end="")
    return 1 if bad else 0


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else
                  os.path.join(root, "profiles", "chain_core_unify_resources.txt")))
