#!/usr/bin/env python3
"""Compare two builds' gfx950 assembly, function by function.

Each of the two directories holds one `.s` file per `.hip` source, made with the Makefile's flags plus
`--cuda-device-only -S`.  For every file the tool compares, by symbol name,

* the text of every function (kernels and device functions that were not inlined),
* every kernel descriptor (`.amdhsa_kernel` ... `.end_amdhsa_kernel`),
* every kernel's entry of the `amdhsa.kernels` metadata (registers, LDS and scratch bytes, spills, the
  kernel-argument segment's size and layout, wavefront size, max flat workgroup size), as text,

after removing comments and the numbers of compiler-generated labels (`.LBB12_3` -> `.LBB_3`), which change when
a function is added in front of another.  It prints one JSON document: per file the counts of identical, changed,
missing and new symbols, and for every changed function both instruction counts; `common_files_identical` says that
every file of the parent is unchanged, `identical` that the tree also adds no file of its own.

    python3 tools/asm_compare.py PARENT_DIR TREE_DIR [--group NAME=REGEX ...] [-o OUT.json]

`--group` tallies the symbols whose (mangled) name matches REGEX separately, so that a change which means to touch
only some kernels can state what happened to those and to all the others.
"""
import argparse
import json
import os
import re
import sys

_LABEL_NUM = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)\d+")
_FUNC_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
_FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
_KD_BEGIN = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_KD_END = re.compile(r"^\s*\.end_amdhsa_kernel")
_MD_NAME = re.compile(r"^\s+\.name:\s+(\S+)")


def normalise(lines):
    out = []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if line:
            out.append(_LABEL_NUM.sub(lambda m: ".L" + m.group(1), line))
    return out


def instruction_count(norm_lines):
    return sum(1 for l in norm_lines if not l.startswith(".") and not l.endswith(":"))


def parse(path):
    """-> (functions, descriptors, metadata): dicts of symbol name -> normalised lines."""
    with open(path, "r", errors="replace") as f:
        lines = f.read().split("\n")
    functions, descriptors, metadata = {}, {}, {}
    i, n = 0, len(lines)
    pending = None  # the name a `.type NAME,@function` announced; its text starts at `NAME:`
    while i < n:
        line = lines[i]
        m = _FUNC_TYPE.match(line)
        if m:
            pending = m.group(1)
        elif pending and line.startswith(pending + ":"):
            j = i + 1
            while j < n and not _FUNC_END.match(lines[j]):
                j += 1
            body = lines[i + 1:j]
            # (a kernel's descriptor stands between its last instruction and its end label)
            for k, l in enumerate(body):
                m = _KD_BEGIN.match(l)
                if m:
                    e = next(x for x in range(k, len(body)) if _KD_END.match(body[x]))
                    descriptors[m.group(1)] = normalise(body[k + 1:e])
                    body = body[:k] + body[e + 1:]
                    break
            functions[pending] = normalise(body)
            pending = None
            i = j
        else:
            m = _KD_BEGIN.match(line)
            if m:
                j = i + 1
                while j < n and not _KD_END.match(lines[j]):
                    j += 1
                descriptors[m.group(1)] = normalise(lines[i + 1:j])
                i = j
            elif line.startswith("amdhsa.kernels:"):
                j = i + 1
                entry = []

                def flush():
                    for l in entry:
                        mm = _MD_NAME.match(l)
                        if mm:
                            metadata[mm.group(1)] = [x.rstrip() for x in entry]
                            return

                while j < n and (lines[j].startswith(" ") or lines[j] == ""):
                    if lines[j].startswith("  - ") and entry:
                        flush()
                        entry = []
                    entry.append(lines[j])
                    j += 1
                if entry:
                    flush()
                i = j - 1
        i += 1
    return functions, descriptors, metadata


def compare_file(parent, tree, groups):
    pf, pd, pm = parse(parent)
    tf, td, tm = parse(tree)

    def tally(names):
        r = {"functions": 0, "functions_identical": 0, "descriptors": 0, "descriptors_identical": 0,
             "metadata_entries": 0, "metadata_identical": 0, "missing": [], "differs": []}
        for name in names:
            if name in pf:
                r["functions"] += 1
                if name not in tf:
                    r["missing"].append(name)
                elif pf[name] == tf[name]:
                    r["functions_identical"] += 1
                else:
                    r["differs"].append({"name": name, "what": "instructions",
                                         "parent_instructions": instruction_count(pf[name]),
                                         "tree_instructions": instruction_count(tf[name])})
            if name in pd:
                r["descriptors"] += 1
                if pd[name] == td.get(name):
                    r["descriptors_identical"] += 1
                else:
                    r["differs"].append({"name": name, "what": "descriptor"})
            if name in pm:
                r["metadata_entries"] += 1
                if pm[name] == tm.get(name):
                    r["metadata_identical"] += 1
                else:
                    r["differs"].append({"name": name, "what": "metadata"})
        return r

    parent_names = sorted(set(pf) | set(pd) | set(pm))
    out = {"all": tally(parent_names),
           "new": sorted((set(tf) | set(td) | set(tm)) - set(parent_names))}
    for gname, rx in groups:
        inside = [x for x in parent_names if rx.search(x)]
        outside = [x for x in parent_names if not rx.search(x)]
        out[gname] = tally(inside)
        out["not_" + gname] = tally(outside)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_dir")
    ap.add_argument("tree_dir")
    ap.add_argument("--group", action="append", default=[], metavar="NAME=REGEX")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    groups = []
    for g in a.group:
        name, rx = g.split("=", 1)
        groups.append((name, re.compile(rx)))
    names = sorted(x for x in os.listdir(a.parent_dir) if x.endswith(".s"))
    result = {"method": "two directories of gfx950 assembly (one .s per .hip: the Makefile's flags plus "
                        "--cuda-device-only -S); functions, kernel descriptors and amdhsa.kernels metadata entries "
                        "compared by symbol name as text, after removing comments and the numbers of "
                        "compiler-generated labels",
              "files": {}}
    same = True
    for x in names:
        t = os.path.join(a.tree_dir, x)
        if not os.path.exists(t):
            result["files"][x] = {"missing_file": True}
            same = False
            continue
        r = compare_file(os.path.join(a.parent_dir, x), t, groups)
        result["files"][x] = r
        same = same and not r["all"]["differs"] and not r["all"]["missing"] and not r["new"]
    result["tree_only_files"] = sorted(x for x in os.listdir(a.tree_dir) if x.endswith(".s") and x not in names)
    # common_files_identical: every file of the parent exists in the tree with every symbol identical and none new;
    # identical: that, and the tree has no file of its own (a new translation unit alone makes it false)
    result["common_files_identical"] = same
    result["identical"] = same and not result["tree_only_files"]
    text = json.dumps(result, indent=1) + "\n"
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
