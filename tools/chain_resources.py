"""Resource usage and fp64 arithmetic of a set of kernels, every instantiation, before and after a change - from the compiler's
own text, no GPU needed.  In each of two directories, for every unit U of the set:
     hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
           -o DIR/U.s bobe_amd/csrc/U.hip 2> DIR/U.remarks
   python tools/chain_resources.py BEFORE_DIR AFTER_DIR [TABLE [SET]]
SET: `chain` (the default: k_hmc_run, k_nuts_run, k_rwalk, k_paths_hmc_run of gp_consumers and gp_paths; TABLE defaults to
profiles/chain_core_unify_resources.txt) or `few` (the few-candidate gradient chains' k_wg_cross*, k_wg_rows*, k_wg_final* of
gp_sweep and gp_criteria; a kernel is matched across a rename: k_wg_rows<K, D> and k_wg_rows_w<K, D, NV> before are
k_wg_rows<K, D, 2> and k_wg_rows<K, D, NV> after).

Per kernel: VGPRs, AGPRs, scratch, occupancy and static LDS from the remarks; the instruction count and the count of every
opcode whose name contains `f64` between the kernel's label and its end from the assembly.  Exit status 1 when any scratch is
above 0, or occupancy, static LDS or an f64 opcode count differs between the two."""
import collections
import os
import re
import sys

SETS = {"chain": (("gp_consumers", "gp_paths"), ("k_hmc_run", "k_nuts_run", "k_rwalk", "k_paths_hmc_run")),
        "few": (("gp_sweep", "gp_criteria"), ("k_wg_cross", "k_wg_cross_w", "k_wg_rows", "k_wg_final", "k_wg_final_w"))}
KERNELS = SETS["chain"][1]
FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("scratch", "ScratchSize [bytes/lane]"), ("occ", "Occupancy [waves/SIMD]"),
          ("LDS", "LDS Size [bytes/block]"))


def kernel_of(symbol):
    """('k_rwalk', 'rbf' | 'matern' | '-', d cap, third template argument) of a mangled name - 0 where there is none -, or None"""
    m = re.match(r"_ZN4bobe(\d+)(\w+)", symbol)
    if not m:
        return None
    name, rest = m.group(2)[:int(m.group(1))], m.group(2)[int(m.group(1)):]
    t = re.match(r"ILi([01])ELi(8|16|32)E(?:Li(\d)E)?E", rest)
    third = int(t.group(3) or 0) if t else 0
    if name == "k_wg_rows_w":                          # (the few set's rename)
        name = "k_wg_rows"
    elif name == "k_wg_rows" and not third:
        third = 2
    if name not in KERNELS:
        return None
    return (name, ("rbf", "matern")[int(t.group(1))], int(t.group(2)), third) if t else (name, "-", 0, 0)


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


def read(directory, units):
    """(unit, kernel) -> the remarks' fields, -> the opcode counts"""
    rem, ops = {}, {}
    for unit in units:
        rem.update({(unit,) + k: v for k, v in remarks(os.path.join(directory, unit + ".remarks")).items()})
        ops.update({(unit,) + k: v for k, v in opcodes(os.path.join(directory, unit + ".s")).items()})
    return rem, ops


def label(k):
    return k[1] + (f"<., ., {k[4]}>" if k[4] else "")


def main(before, after, table, which):
    global KERNELS
    units, KERNELS = SETS[which]
    (rb, ob), (ra, oa) = read(before, units), read(after, units)
    keys = sorted(rb, key=lambda k: (KERNELS.index(k[1]), k[0] != units[0], k[4], k[3], k[2] != "rbf"))
    assert set(rb) == set(ra) == set(ob) == set(oa) and keys, (len(rb), len(ra), len(ob), len(oa))
    assert which != "chain" or len(keys) == 6 * len(KERNELS)
    many = len({k[0] for k in keys if k[1] == "k_wg_rows"}) > 1
    lines = ["# the " + which + " kernels before -> after, gfx950, from -Rpass-analysis=kernel-resource-usage and the device assembly",
             "# (tools/chain_resources.py).  f64: the number of instructions whose opcode contains `f64`; `same` = every such opcode",
             "# occurs as often after as before."]
    if many:
        lines.append("# k_wg_rows: in gp_sweep the parent's k_wg_rows<K, D> against k_wg_rows<K, D, 2>, in gp_criteria the parent's "
                     "k_wg_rows_w<K, D, NV> against k_wg_rows<K, D, NV>")
    lines.append(f"{'kernel':20s} {'family':6s} {'cap':>3s} | {'VGPRs':>9s} | {'AGPRs':>10s} | {'scratch':>7s} | {'occ':>6s} | "
                 f"{'static LDS':>12s} | {'instructions':>14s} | f64")
    bad = []
    for k in keys:
        b, a = rb[k], ra[k]
        cell = {name: f"{b[field]} -> {a[field]}" for name, field in FIELDS}
        fb = {o: c for o, c in ob[k].items() if o != "instructions"}
        fa = {o: c for o, c in oa[k].items() if o != "instructions"}
        diff = {o: (fb.get(o, 0), fa.get(o, 0)) for o in sorted(set(fb) | set(fa)) if fb.get(o, 0) != fa.get(o, 0)}
        f64 = f"{sum(fb.values())} -> {sum(fa.values())} " + ("same" if not diff else "DIFFER " + str(diff))
        name = label(k) + (f" ({k[0][3:]})" if many and k[1] == "k_wg_rows" else "")
        lines.append(f"{name:20s} {k[2]:6s} {k[3]:3d} | {cell['VGPRs']:>9s} | {cell['AGPRs']:>10s} | {cell['scratch']:>7s} | "
                     f"{cell['occ']:>6s} | {cell['LDS']:>12s} | {ob[k]['instructions']:6d} -> {oa[k]['instructions']:5d} | {f64}")
        if diff or int(a[FIELDS[2][1]]) or int(b[FIELDS[2][1]]) or any(b[f] != a[f] for _, f in FIELDS[3:]):
            bad.append(k)
    lines.append("")
    lines.append("# per-opcode f64 counts (after)")
    for k in keys:
        if many and k[1] == "k_wg_rows" and k[0] != units[1] and (units[1],) + k[1:] in oa:
            continue                                   # (the same instantiation in both units: listed once)
        lines.append(f"{label(k)} {k[2]} {k[3]}: " + ", ".join(f"{o} {c}" for o, c in sorted(oa[k].items()) if o != "instructions"))
    lines.append("")
    lines.append("every kernel: scratch 0, occupancy, static LDS and every f64 opcode count unchanged" if not bad
                 else "NOT HELD by: " + ", ".join(f"{label(k)} {k[2]} {k[3]} ({k[0]})" for k in bad))
    text = "\n".join(lines) + "\n"
    open(table, "w").write(text)
    print(text, end="")
    return 1 if bad else 0


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else
                  os.path.join(root, "profiles", "chain_core_unify_resources.txt"), sys.argv[4] if len(sys.argv) > 4 else "chain"))
