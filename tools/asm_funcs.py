#!/usr/bin/env python3
"""Compare the device code of two builds function by function: asm_funcs.py OLD_DIR NEW_DIR.

Each directory holds the .s files of `make -C hkd-mpc_amd/csrc hazards` (build/asm/).  A function
is the text from its `.type NAME,@function` line to its `.Lfunc_endN:` line, taken over all files
of a directory together, with comments (from `;` on) dropped and the running numbers of local labels
(.LBB<n>_, .Ltmp<n>, .Lfunc_begin<n>, .Lfunc_end<n>, .LJTI<n>, .Lpost_getpc<n>) stripped: function order and label
numbers change with the file a kernel sits in and with the order in which launchers instantiate
it, the instructions do not.  Text only; no instruction is inspected.

Prints the counts and every name that is only on one side or whose body differs; exit status 1 if
there is any."""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end|LJTI|Lpost_getpc)\d+")


def functions(directory):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        name, body = None, []
        for line in open(path):
            m = re.match(r"\s*\.type\s+(\S+),@function", line)
            if m:
                name, body = m.group(1), []
            if name is None:
                continue
            text = LABEL.sub(r".\1", line.split(";", 1)[0]).rstrip()
            if text:
                body.append(text)
            if re.match(r"\.Lfunc_end\d+:", line):
                assert name not in out, f"{name} defined twice under {directory}"
                out[name] = (os.path.basename(path), "\n".join(body))
                name = None
    return out


def main(old_dir, new_dir):
    old, new = functions(old_dir), functions(new_dir)
    lost, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if old[n][1] != new[n][1])
    print(f"{len(old)} functions in {old_dir}, {len(new)} in {new_dir}: "
          f"{len(set(old) & set(new)) - len(differ)} identical, {len(differ)} differ, {len(lost)} lost, {len(added)} added")
    for title, names, side in (("lost", lost, old), ("added", added, new), ("differ", differ, new)):
        for n in names:
            lines = f"{old[n][1].count(chr(10)) + 1} -> {new[n][1].count(chr(10)) + 1} lines" if title == "differ" else ""
            print(f"{title}: {n} ({side[n][0]}) {lines}".rstrip())
    return 1 if lost or added or differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
