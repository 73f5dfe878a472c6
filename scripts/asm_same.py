#!/usr/bin/env python3
"""Compares the device assembly of two builds function by function (make asm -> build/rt_render.s).

    python3 scripts/asm_same.py PARENT.s THIS.s [REGEX ...]

Each REGEX is deleted from every line of THIS.s first: a change that only renames kernels (a new
template parameter or argument type in the mangled names) is then compared under the parent's names.

A function is the text from its `name:` label to its .Lfunc_end label.  Comments, blank lines and
the numbers of local labels (.LBBn_m, .Ltmpn, .Lfunc_endn: they count functions of the whole file,
so a new kernel shifts them) are ignored.  Prints the functions only one side has and those whose
text differs; the exit status is 1 if a function of PARENT is missing from THIS or differs."""
import re
import sys


def functions(path, strip=()):
    out, name, body = {}, None, []
    for line in open(path):
        for rx in strip:
            line = re.sub(rx, "", line)
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*$", line)
        if m and not m.group(1).startswith(".L") and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[name] = body
                name = None
                continue
            body.append(re.sub(r"\.L(BB|tmp|func_end|func_begin)\d+(_\d+)?", r".L\1", line))
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2], sys.argv[3:])
    gone = sorted(set(a) - set(b))
    new = sorted(set(b) - set(a))
    diff = sorted(k for k in a if k in b and a[k] != b[k])
    print(f"{len(a)} functions in the parent, {len(b)} here; {len(a) - len(gone) - len(diff)} identical")
    for k in gone:
        print("missing here:", k)
    for k in diff:
        print("differs:", k)
    for k in new:
        print("new:", k)
    return 1 if gone or diff else 0


if __name__ == "__main__":
    sys.exit(main())
