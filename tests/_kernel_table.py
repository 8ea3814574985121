"""The one reader of the kernel table of csrc/rt_device.hip (stream_kernel_for() and the two shape lists above it), for the CPU tests that hold a family of
instantiations against the recipes the GPU tests run.  A form is (world, exact, ext, big, wide), as the *_worlds modules key their FORMS.

    family(name) -> the set of forms the family ships;  count(name) -> how many case labels it has (a form listed twice would show here, and does not compile)
    plain()      -> the plain keys, as (exact, filter, world, ext, big, wide, tol)
    labels()     -> all case labels of the switch

Every line of the switch and of the shape lists must be one this module reads to its end: anything else raises, so that a table in another form fails the tests
that use it and never passes as a smaller set."""
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_device.hip")

MODE_48 = frozenset({"NEE", "LTREE", "ENVL"})   # what a form under mode 48 carries beside TRI and its own bits
# the families by the names the tests use, each with the RT_KEY_* bits its line of the table names
FAMILY_BITS = {
    "NEE": frozenset({"NEE"}), "TRI": frozenset({"TRI"}), "TRI_NEE": frozenset({"TRI", "NEE"}), "LIGHT_TREE": frozenset({"TRI", "NEE", "LTREE"}),
    "ENV_LIGHT": frozenset({"TRI", "NEE", "ENVL"}), "ENV_TREE": frozenset({"TRI"}) | MODE_48,
    "NORMAL_MAP": frozenset({"TRI", "NMAP"}), "MICROFACET": frozenset({"TRI", "MFAC"}),
    "INTERIOR": frozenset({"TRI", "MFAC", "INTR"}), "CUTOUT": frozenset({"TRI", "MFAC", "INTR", "CUT"}),
}
for _name in ("NORMAL_MAP", "MICROFACET", "INTERIOR", "CUTOUT"):
    FAMILY_BITS[_name + "_ENV_TREE"] = FAMILY_BITS[_name] | MODE_48

_BOOL = r"(true|false)"
_SHAPE = re.compile(r"S\(" + _BOOL + r", (RT_WORLD_\w+), (\d), " + _BOOL + ", " + _BOOL + r", bits\)\s*")
_PLAIN = re.compile(r"RT_KERNEL\(" + _BOOL + ", " + _BOOL + r", (RT_WORLD_\w+), (\d), " + _BOOL + ", " + _BOOL + ", " + _BOOL + r"\)\s*")
_FAMILY = re.compile(r"RT_FAMILY_(16|8)\(((?:RT_KEY_[A-Z]+)(?: \| RT_KEY_[A-Z]+)*)\)\s*")
_XCHG = re.compile(r"case RT_KEY_XCHG: return reinterpret_cast<const void\*>\(&render_kernel_xchg<RT_XCHG_BLOCK>\);\s*")


def _read_all(pattern, text, what):
    """every match of `pattern` in `text`, which must consist of such matches alone"""
    found, at = [], 0
    text = text.strip()
    while at < len(text):
        m = pattern.match(text, at)
        if not m:
            raise AssertionError(f"tests/_kernel_table.py does not read this part of {what}: {text[at:at + 120]!r}")
        found.append(m.groups())
        at = m.end()
    return found


def _shape_list(src, n):
    m = re.search(r"^#define RT_SHAPES_%d\(S, bits\) \\\n((?:.*\\\n)*.*)\n" % n, src, re.M)
    if not m:
        raise AssertionError(f"tests/_kernel_table.py finds no RT_SHAPES_{n}(S, bits) in rt_device.hip")
    shapes = _read_all(_SHAPE, m.group(1).replace("\\\n", " "), f"RT_SHAPES_{n}")
    return [(world, int(exact == "true"), int(ext), int(big == "true"), int(wide == "true")) for exact, world, ext, big, wide in shapes]


@functools.lru_cache(maxsize=None)
def _table():
    src = open(SOURCE).read()
    shapes = {16: _shape_list(src, 16), 8: _shape_list(src, 8)}
    assert len(shapes[16]) == 16 and len(shapes[8]) == 8
    assert shapes[8] == [s for s in shapes[16] if s[2] == 2]   # the EXT 2 members, in the same order
    body = src[src.index("switch (key) {") + len("switch (key) {"):]
    body = body[:body.index("default: return nullptr;")]
    xchg, plain, families = 0, [], {}
    for line in body.split("\n"):
        line = line.strip()
        if not line or line.startswith("//"):
            continue
        if _XCHG.fullmatch(line):
            xchg += 1
        elif line.startswith("RT_KERNEL("):
            plain += [(int(e == "true"), int(f == "true"), world, int(ext), int(b == "true"), int(w == "true"), int(t == "true"))
                      for e, f, world, ext, b, w, t in _read_all(_PLAIN, line, "the plain keys")]
        else:
            for n, bits in _read_all(_FAMILY, line, "the family lines"):
                names = bits.replace("RT_KEY_", "").split(" | ")
                key = frozenset(names)
                assert len(key) == len(names) and key not in families, line   # a bit or a family named twice
                families[key] = shapes[int(n)]
    assert src.count("RT_FAMILY_16(RT_KEY_") + src.count("RT_FAMILY_8(RT_KEY_") == len(families)   # every use is one that was read
    assert set(families) == set(FAMILY_BITS.values()), set(families) ^ set(FAMILY_BITS.values())
    return xchg, plain, families


def count(name):
    return len(_table()[2][FAMILY_BITS[name]])


def family(name):
    return set(_table()[2][FAMILY_BITS[name]])


def plain():
    return list(_table()[1])


def labels():
    """(exchange labels, plain labels, {family name: labels})"""
    xchg, plain_keys, _ = _table()
    return xchg, len(plain_keys), {name: count(name) for name in FAMILY_BITS}
