"""The kernel table's totals and the ladder of the four per-material tables, without a GPU: the label counts of stream_kernel_for(), the key bits
of FORM_LADDER's rows against the families the table ships, and the refusals the rows compose against the literal texts they replaced."""
import os
import re

import _kernel_table as KT
from _common import ROOT

SRC = open(os.path.join(ROOT, "ray-tracing-v06_amd", "csrc", "rt_device.hip")).read()
RUNG_FAMILIES = ("NORMAL_MAP", "MICROFACET", "INTERIOR", "CUTOUT")


def ladder_rows():
    body = SRC[SRC.index("static const FormRung FORM_LADDER[N_RUNGS] = {"):]
    body = body[:body.index("\n};")]
    rows = re.findall(r'^    \{((?:RT_KEY_[A-Z]+)(?: \| RT_KEY_[A-Z]+)*), "([^"]*)", "([^"]*)", "([^"]*)", "([^"]*)", "([^"]*)"\},$', body, re.M)
    assert len(rows) == body.count("{RT_KEY_") == 4
    return [dict(bits=frozenset(r[0].replace("RT_KEY_", "").split(" | ")), api=r[1], a=r[2], table=r[3], surfaces_render=r[4], variant_5_6=r[5]) for r in rows]


def test_the_table_has_171_labels():
    xchg, plain, families = KT.labels()
    assert xchg == 1 and plain == 26 and len(set(KT.plain())) == 26
    sixteen, eight = ("NEE", "TRI", "TRI_NEE", "LIGHT_TREE"), ("ENV_LIGHT", "ENV_TREE")
    assert all(families[f] == 16 for f in sixteen) and all(families[f] == 8 for f in eight)
    material = [f + tail for f in RUNG_FAMILIES for tail in ("", "_ENV_TREE")]
    assert all(families[f] == 8 for f in material) and set(families) == set(sixteen + eight) | set(material)
    assert xchg + plain + sum(families.values()) == 1 + 26 + 4 * 16 + 2 * 8 + 8 * 8 == 171
    assert all(len(KT.family(f)) == n for f, n in families.items())   # no form twice in a family


def test_each_rungs_bits_are_its_familys():
    rows = ladder_rows()
    assert [r["bits"] for r in rows] == [frozenset({"NMAP"}), frozenset({"MFAC"}), frozenset({"MFAC", "INTR"}), frozenset({"MFAC", "INTR", "CUT"})]
    for row, name in zip(rows, RUNG_FAMILIES):
        assert row["bits"] | {"TRI"} == KT.FAMILY_BITS[name] and row["bits"] | {"TRI"} | KT.MODE_48 == KT.FAMILY_BITS[name + "_ENV_TREE"]
    assert [r["api"] for r in rows] == ["rt_renderer_normal_maps", "rt_renderer_microfacets", "rt_renderer_interiors", "rt_renderer_cutouts"]


# what the four setters, rt_renderer_light_sampling_enable and the resolver said before the ladder, per rung (nouns: table with article, table, surfaces + verb)
BEFORE = {
    "rt_renderer_normal_maps": ("a normal-map table", "normal-map table", "normal maps render", "kernel variant %u reads no texture table and no normal-map table"),
    "rt_renderer_microfacets": ("a microfacet table", "microfacet table", "microfacet surfaces render", "kernel variant %u reads no microfacet table"),
    "rt_renderer_interiors": ("an interior table", "interior table", "solid glass renders", "kernel variant %u reads no interior table"),
    "rt_renderer_cutouts": ("a cutout table", "cutout table", "alpha cutouts render", "kernel variant %u reads no cutout table"),
}


def texts_before(api):
    a_table, table, render, variant = BEFORE[api]
    return {
        f"{api}: null renderer",
        f"{api}: a table and its count go together (NULL, 0 turns it off)",
        f"{api}: the baseline kernel (variant 1) reads no {table}; use variant 0, 2 or 3",
        f"{api}: {variant}",
        f"{api}: a world with a queue or wide4 traversal renders on lane walks that read no {table} (RT_TRAVERSAL_STACK and lists do)",
        f"{api}: a bvh_node tree renders on a walk that reads no {table} (BVHs walked by the stack and lists do)",
        f"{api}: light-sampling mode %u is on, which has no kernel that reads {a_table}: {render} with light sampling off or in mode 48",
        f"{api}: %u records for a world of %u materials",
        f"{api}: this world's kernel has no form that reads {a_table}",
        f"rt_renderer_light_sampling_enable: the renderer has {a_table}, and light-sampling mode %u has no kernel that reads one: {render} with light sampling off or in mode 48 "
        f"(take the table away with {api}(NULL, 0) first)",
    }


def test_the_rows_compose_the_refusals_that_were_literal():
    """every rt_fail whose arguments name a row's words (f.api, FORM_LADDER[g].api, ...), with the words of each rung put in: the ten texts of before, byte for byte"""
    calls = re.findall(r'rt_fail\(RT_ERR_INVALID, "((?:[^"\\]|\\.)*)", ((?:f\.|FORM_LADDER\[g\]\.)\w+, [^;]*|(?:f\.|FORM_LADDER\[g\]\.)\w+)\);', SRC)
    assert len(calls) == 10
    for row in ladder_rows():
        composed = set()
        for fmt, args in calls:
            for arg in (a.strip() for a in args.split(", ")):
                word = re.fullmatch(r"(?:f|FORM_LADDER\[g\])\.(\w+)", arg)
                at = re.search(r"%[su]", fmt)
                assert at is not None and (at.group() == "%s") == (word is not None), (fmt, arg)
                fmt = fmt[:at.start()] + (row[word.group(1)] if word else "\0") + fmt[at.end():]   # (\0: a %u that stays)
            composed.add(fmt.replace("\0", "%u"))
        assert composed == texts_before(row["api"]), composed ^ texts_before(row["api"])
