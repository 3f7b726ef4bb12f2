"""profiles/batch_terms_parity.txt from the output of `pytest tests/test_gpu_batch_terms.py -q -s -rxX` (a file: argv[1]).
Kept: every Layer A line, Layer B's line per run, its lines per stage of tile_edge wipstd on the first path run and, of the runs
that miss the rule, the stages marked * with the stage before the first of them (first path run), the duplicates' and the
no-variance pick's lines, the expected failures' reasons."""
import re
import sys

STAGE = re.compile(r"(\S+) (\S+) \S+ \(\S+\)\s+stage\s+(\d+)\s+device")
HEAD = """Output of tests/test_gpu_batch_terms.py (pytest -s -rxX) on an MI355X, abridged by tools/abridge_batch_terms.py.  Layer A:
every line the file prints - per case, path and run the worst ratio to the bound of each step and where it was found (stage j,
index).  Layer B: the file prints one line per stage (the device's error, float64 NumPy's running the recursion on the device's
stage-0 terms, the float64 literal refit's, the truth's gap; * = the rule is missed there) and one line per run.  Kept: the line
per run of every case, criterion and path; the lines per stage of tile_edge wipstd (63 downdates); of the runs that miss the
rule the stages marked * with the stage before the first of them - both on the first path run only.
"""
lines, runs = [], {}
for raw in open(sys.argv[1]):
    line = re.sub(r"^[.xFE]+(?=[A-Za-z])", "", raw.rstrip("\n")).rstrip()
    if not line or re.match(r"^[.xFE]*$", line) or "amdgpu.ids" in line:
        continue
    if line[0] in "=_" and "passed" not in line and "short test summary" not in line:
        continue
    lines.append(line)
out, i = [], 0
while i < len(lines):
    m = STAGE.match(lines[i])
    if not m:
        out.append(lines[i])
        i += 1
        continue
    j = i
    while j < len(lines) and STAGE.match(lines[j]):
        j += 1
    pair, block = m.group(1, 2), lines[i:j]
    runs[pair] = runs.get(pair, 0) + 1
    if runs[pair] == 1:
        if pair == ("tile_edge", "wipstd"):
            out += block
        elif any("*" in x for x in block):
            first = next(k for k, x in enumerate(block) if "*" in x)
            out += [x for k, x in enumerate(block) if "*" in x or k == first - 1]
    i = j
sys.stdout.write(HEAD + "\n" + "\n".join(out) + "\n")
