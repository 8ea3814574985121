"""`make -C ray-tracing-v06_amd/csrc resources 2>&1 | python tools/resource_table.py` -> one line per kernel, sorted by name, every figure the compiler reports
(the form of the tables under profiles/); `python tools/resource_table.py A B` prints the kernels whose lines differ between two such tables, and those only one has.
`python tools/resource_table.py A B --inserted N` is for a B whose render_kernel_stream has one template argument more than A's, a bool at position N (from 1):
a kernel of B with `false` there is compared under the name it had in A, one with `true` is new."""
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


def without_argument(name, position):
    """(the mangled name of a render_kernel_stream instantiation without its template argument `position`, that argument's text) — or (name, None)"""
    m = re.match(r"(_Z20render_kernel_streamI)((?:L[bi]\d+E)+)(Ev12StreamParams)$", name)
    if not m:
        return name, None
    args = re.findall(r"L[bi]\d+E", m.group(2))
    return m.group(1) + "".join(args[:position - 1] + args[position:]) + m.group(3), args[position - 1]


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[3] == "--inserted":
        a, b, position = read(sys.argv[1]), read(sys.argv[2]), int(sys.argv[4])
        same, new = 0, []
        for k in sorted(b):
            old, arg = without_argument(k, position)
            if arg == "Lb1E":
                new.append(k)
            elif a.get(old) == b[k]:
                same += 1
            else:
                print(f"{k}\n  - {a.get(old, '(absent)')}\n  + {b[k]}")
        print(f"# {len(a)} kernels in the first table, {len(b)} in the second; {same} identical modulo template argument {position}, {len(b) - same - len(new)} differ, {len(new)} new:")
        for k in new:
            print(f"{k}: {b[k]}")
    elif len(sys.argv) == 3:
        a, b = read(sys.argv[1]), read(sys.argv[2])
        for k in sorted(set(a) | set(b)):
            if a.get(k) != b.get(k):
                print(f"{k}\n  - {a.get(k, '(absent)')}\n  + {b.get(k, '(absent)')}")
        print(f"# {len(set(a) & set(b))} kernels in both, {sum(a[k] == b[k] for k in set(a) & set(b))} of them identical; {len(set(b) - set(a))} new, {len(set(a) - set(b))} gone")
    else:
        for k, v in sorted(table(sys.stdin.read()).items()):
            print(f"{k}: {v}")
