"""Compare the gfx950 device code of the three top-N scans between two trees, kernel by kernel.

    python tools/isa_compare.py BEFORE_DIR AFTER_DIR [NAME ...]

Each directory holds, per source scan / scan_quorum / scan_spread (or the NAMEs given, e.g.
partners), NAME.s and NAME.rpass: the device
assembly and the stderr of the build's own command line with
    --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o NAME.s csrc/NAME.hip
A kernel's body runs from its label to its .Lfunc_end; comments and directives are dropped and the
local labels renumbered in order of appearance before the instruction sequences are compared.  The
resource row is everything the remark prints for the kernel (registers, spills, scratch, LDS,
occupancy).  Kernels pair by mangled name; the merge kernels (one per file) pair with each other
whatever their names.  Prints one line per kernel family and exits 1 on any difference; a kernel
that only the second tree has is listed and counts as one.
"""
import collections
import os
import re
import sys

SOURCES = ("scan", "scan_quorum", "scan_spread")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(path):
    """{mangled name: normalised instruction list}"""
    out, name, body = {}, None, None
    for ln in open(path):
        if name is None:
            m = re.match(r"(_Z\w+):", ln)
            if m:
                name, body = m.group(1), []
            continue
        if ln.startswith(".Lfunc_end"):
            out[name] = renumber(body)
            name = None
            continue
        code = ln.split(";")[0].strip()
        if not code or (code.startswith(".") and not code.endswith(":")):
            continue
        body.append(code)
    return out


def renumber(body):
    ids = {}
    return [LABEL.sub(lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), ln) for ln in body]


def resources(path):
    """{mangled name: tuple of the remark's rows}"""
    out, name = collections.OrderedDict(), None
    for ln in open(path):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]", ln)
        if not m:
            continue
        row = m.group(1).strip()
        if row.startswith("Function Name: "):
            name = row.split(": ", 1)[1]
            out[name] = []
        elif name:
            out[name].append(row)
    return {k: tuple(v) for k, v in out.items()}


def family(name):
    if "merge_kernel" in name:
        return "merge kernel"
    m = re.search(r"\d+((?:scan|partners|screen)_[a-z_]*kernel)", name)
    return m.group(1) if m else name


def main(before, after, sources=SOURCES):
    bad = 0
    for src in sources:
        kb, ka = (kernels(os.path.join(d, src + ".s")) for d in (before, after))
        rb, ra = (resources(os.path.join(d, src + ".rpass")) for d in (before, after))
        assert set(kb) == set(rb) and set(ka) == set(ra), "assembly and remarks name other kernels"
        merge_b, merge_a = ([k for k in d if family(k) == "merge kernel"] for d in (kb, ka))
        pairs = [(k, k) for k in kb if k not in merge_b] + list(zip(merge_b, merge_a))
        missing = set(ka) - {a for _, a in pairs}
        count, diff = collections.Counter(), collections.defaultdict(list)
        for b, a in pairs:
            count[family(b)] += 1
            if a not in ka:
                diff[family(b)].append(b + ": missing")
            elif kb[b] != ka[a]:
                diff[family(b)].append("%s: instructions differ (%d -> %d)" % (b, len(kb[b]), len(ka[a])))
            elif rb[b] != ra[a]:
                diff[family(b)].append("%s: resource row differs" % b)
        for fam in count:
            print("%-16s %-28s %3d instantiations  %s" % (src + ".hip", fam, count[fam],
                                                          "DIFFER" if diff[fam] else "equal"))
            for d in diff[fam]:
                print("    " + d)
        for k in sorted(missing):
            print("    only after: " + k)
        bad += len(missing) + sum(len(v) for v in diff.values())
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], tuple(sys.argv[3:]) or SOURCES))
