"""`make -C ray-tracing-v06_amd/csrc resources 2>&1 | python tools/resource_table.py` -> one line per kernel, sorted by name, every figure the compiler reports
(the form of the tables under profiles/); `python tools/resource_table.py A B` prints the kernels whose lines differ between two such tables, and those only one has."""
import re
import sys


def table(text):
    rows, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if m.group(1).startswith("Function Name: "):
            name = m.group(1)[len("Function Name: "):]
            rows[name] = []
        elif name:
            rows[name].append(m.group(1).strip())
    return {k: "; ".join(v) for k, v in rows.items()}


def read(path):
    return dict(line.rstrip("\n").split(": ", 1) for line in open(path) if not line.startswith("#") and ": " in line)


if __name__ == "__main__":
    if len(sys.argv) == 3:
        a, b = read(sys.argv[1]), read(sys.argv[2])
        for k in sorted(set(a) | set(b)):
            if a.get(k) != b.get(k):
                print(f"{k}\n  - {a.get(k, '(absent)')}\n  + {b.get(k, '(absent)')}")
        print(f"# {len(set(a) & set(b))} kernels in both, {sum(a[k] == b[k] for k in set(a) & set(b))} of them identical; {len(set(b) - set(a))} new, {len(set(a) - set(b))} gone")
    else:
        for k, v in sorted(table(sys.stdin.read()).items()):
            print(f"{k}: {v}")
