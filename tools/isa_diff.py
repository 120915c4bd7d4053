#!/usr/bin/env python3
"""Compare two device assembly listings kernel by kernel (no GPU needed).

    hipcc --offload-arch=gfx950 <the file's flags> -S --offload-device-only f.hip -o new.s
    python tools/isa_diff.py old.s new.s [--map OLD_SUBSTRING=NEW_SUBSTRING ...] [--map-file FILE]

For every kernel symbol (``.amdhsa_kernel``) the instruction lines of its body are compared:
comments, directives and blank lines are dropped, and block labels (``.LBB12_3``) are renumbered
in order of appearance, so a kernel that merely moved in the file compares equal.  ``--map``
rewrites substrings of the OLD listing's symbols first, for kernels whose mangled name changed
(``--map-file``: one OLD=NEW per line).  Prints one line per kernel -- same / differ / only in
old / only in new -- and a unified diff of the first kernel that differs.  Exit status 1 when a
kernel present in both differs.  The compile flags of a file are the ones ``_build.py`` gives it
(``tools/kernel_resources.py`` shows how its ``sml-build:`` line is read).  The comparison is
textual: it knows nothing about the instruction set.
"""
import argparse
import difflib
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(text):
    """{symbol: [instruction lines]} for the kernels of one listing."""
    lines = text.splitlines()
    names = {ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel")}
    out, cur = {}, None
    for ln in lines:
        s = ln.split(";", 1)[0].strip()
        if not s:
            continue
        if cur is None:
            if s.endswith(":") and s[:-1] in names:
                cur = out.setdefault(s[:-1], [])
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        elif s.startswith(".") and not s.endswith(":"):
            continue   # a directive
        else:
            cur.append(" ".join(s.split()))
    for body in out.values():   # block labels by order of appearance
        seen = {}
        body[:] = [LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), ln) for ln in body]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", nargs="+", default=[], metavar="OLD=NEW")
    ap.add_argument("--map-file")
    args = ap.parse_args()
    maps = list(args.map)
    if args.map_file:
        with open(args.map_file) as f:
            maps += [ln.strip() for ln in f if "=" in ln and not ln.startswith("#")]
    with open(args.old) as f:
        old_text = f.read()
    for m in maps:
        a, b = m.split("=", 1)
        old_text = old_text.replace(a, b)
    with open(args.new) as f:
        old, new = kernels(old_text), kernels(f.read())
    differ = []
    for name in sorted(set(old) | set(new)):
        if name not in new:
            status = "only in old"
        elif name not in old:
            status = "only in new"
        elif old[name] == new[name]:
            status = "same (%d instruction lines)" % len(new[name])
        else:
            status = "differ (%d -> %d instruction lines)" % (len(old[name]), len(new[name]))
            differ.append(name)
        print("%-12s %s" % (status.split(" (")[0] + ":", name + (" (" + status.split(" (", 1)[1] if " (" in status else "")))
    both = len(set(old) & set(new))
    print("%d kernels in both: %d same, %d differ; %d only in old, %d only in new" %
          (both, both - len(differ), len(differ), len(set(old) - set(new)), len(set(new) - set(old))))
    if differ:
        n = differ[0]
        sys.stdout.writelines(difflib.unified_diff([ln + "\n" for ln in old[n]], [ln + "\n" for ln in new[n]],
                                                   "old " + n, "new " + n, n=2))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
