#!/usr/bin/env python3
"""Per-kernel resource figures from the device assembly hipcc keeps with -save-temps.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I <csrc> -save-temps -c attn_flash.hip -o /tmp/x.o
    python scripts/isa_stats.py attn_flash-hip-amdgcn-amd-amdhsa-gfx950.s [other.s]

One row per kernel: VGPR / AGPR / SGPR counts, LDS bytes, scratch bytes (from the amdhsa
metadata) and the number of instructions in its body.  With two files (parent build, new build)
the kernels present in both are printed side by side and the rows that differ are flagged - the
evidence that a template parameter added for a new instantiation left the existing ones alone.
"""
from __future__ import annotations

import re
import subprocess
import sys

FIELDS = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"),
          ("lds", ".group_segment_fixed_size"), ("scratch", ".private_segment_fixed_size"))


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    text = open(path).read().splitlines()
    stats, cur = {}, None
    # amdhsa.kernels metadata: one "- .agpr_count:" ... ".name:" block per kernel
    for ln in text:
        s = ln.strip()
        if s.startswith("- .agpr_count:") or s.startswith("- .args:"):
            cur = {}
        if cur is None:
            continue
        for key, tag in FIELDS:
            m = re.match(r"(?:- )?%s:\s+(\d+)" % re.escape(tag), s)
            if m:
                cur[key] = int(m.group(1))
        m = re.match(r"\.name:\s+(\S+)", s)
        if m:
            stats[m.group(1)] = cur
        if s.startswith(".wavefront_size:"):
            cur = None
    # instruction counts: lines of the body that are neither labels, directives nor comments
    for name in stats:
        n, inside = 0, False
        for ln in text:
            if ln.startswith(name + ":"):
                inside = True
                continue
            if inside:
                s = ln.strip()
                if s.startswith(".Lfunc_end"):
                    break
                if s and not s.startswith((".", ";")) and not s.endswith(":"):
                    n += 1
        stats[name]["insts"] = n
    return stats


def stream(path, name):
    """The instruction stream of one kernel body: comments and directives dropped, the local labels
    (.LBB<function>_<block>) renumbered by first appearance, so two builds compare line by line."""
    out, inside, labels = [], False, {}
    ren = lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels))
    for ln in open(path):
        if ln.startswith(name + ":"):
            inside = True
            continue
        if not inside:
            continue
        s = ln.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            break
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        out.append(re.sub(r"\.LBB\d+_\d+", ren, s))
    return out


def plain_name(d):
    """Every trailing `false` template argument dropped (kernel<A, false, false> and the parent's
    kernel<A, false> are both kernel<A>), and with it the empty argument struct that such a switch
    adds to the parameter list (`, rtdc::XentAux<false>`): the name the kernel had before."""
    d = re.sub(r", rtdc::XentAux<false>\)", ")", d)
    # flash attention: the row groups per wave became the kernels' fourth template argument, so
    # name2_kernel<D, NS[, true]> is name_kernel<D, NS, doc, 2> and name_kernel<D, NS[, true]> is
    # name_kernel<D, NS, doc, 1>; both trees are keyed by the four-argument name (a pair that is
    # still two kernels in both trees lines up under those names as well)
    m = re.match(r"(.*\bfa::(?:fwd|bwd_dq|bwd_dkdv))(2?)_kernel<(\d+), (\d+)(?:, (true|false|\d+))?(?:, (\d+))?(?:, (true|false))?>(.*)$",
                 d)
    if m:
        # the mask switch was a bool (false / true = documents) before it became the int MASK
        # (0 none, 1 documents, 2 sliding window): 0 / 1 are listed under the bool's names
        mask = {"0": "false", "1": "true", "2": "window"}.get(m.group(5) or "0", m.group(5))
        # a trailing bool is the attention-dropout switch DROP: false keeps the four-argument name
        return "%s_kernel<%s, %s, %s, %d%s>%s" % (m.group(1), m.group(3), m.group(4), mask,
                                                  2 if m.group(2) else int(m.group(6) or 1),
                                                  ", drop" if m.group(7) == "true" else "", m.group(8))
    while True:
        n = re.sub(r", false>", ">", d)
        if n == d:
            return d
        d = n


def short(d):
    d = re.sub(r"^void rtdc::fa::", "", d)
    return re.sub(r"\(rtdc::fa::Args\)$", "", d)


def main(argv):
    if not 1 <= len(argv) <= 2:
        print(__doc__)
        return 2
    tabs = [parse(p) for p in argv]
    # key by the demangled name; a defaulted trailing `false` template argument (the parent's
    # kernel<DH, NS> is the new kernel<DH, NS, false>) names the same kernel
    mangled = [{}, {}]
    for i, t in enumerate(tabs):
        d = demangle(sorted(t))
        mangled[i] = {plain_name(d[k]): k for k in t}
        tabs[i] = {plain_name(d[k]): v for k, v in t.items()}
    names = sorted(set().union(*tabs))
    dm = {n: n for n in names}
    cols = [k for k, _ in FIELDS] + ["insts"]
    print("%-52s %s" % ("kernel", "  ".join("%-15s" % c if len(tabs) == 2 else "%7s" % c for c in cols)))
    bad = 0
    for n in sorted(names, key=lambda x: dm[x]):
        rows = [t.get(n) for t in tabs]
        if len(tabs) == 1:
            print("%-52s %s" % (short(dm[n]), "  ".join("%7d" % rows[0].get(c, -1) for c in cols)))
            continue
        cells, diff = [], False
        for c in cols:
            a = rows[0].get(c, -1) if rows[0] else None
            b = rows[1].get(c, -1) if rows[1] else None
            diff |= a is not None and b is not None and a != b
            cells.append("%-15s" % ("%s -> %s" % ("-" if a is None else a, "-" if b is None else b)))
        bad += diff
        print("%-52s %s%s" % (short(dm[n]), "  ".join(cells), "   DIFFERS" if diff else ""))
    if len(tabs) == 2:
        print("kernels in both builds that differ: %d" % bad)
        # beyond the counts: the instruction streams of the kernels present in both builds
        print()
        for n in names:
            if n in tabs[0] and n in tabs[1]:
                a, b = stream(argv[0], mangled[0][n]), stream(argv[1], mangled[1][n])
                nd = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
                bad += nd != 0
                print("%-46s %5d insts  %s" % (short(n), len([x for x in a if not x.endswith(":")]),
                                              "identical instruction stream" if nd == 0 else "%d lines differ" % nd))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
