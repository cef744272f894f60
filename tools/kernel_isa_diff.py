#!/usr/bin/env python3
"""Two gfx950 assembly files of the library (the hipcc line of tools/kernel_resources.sh with -o A.s / B.s), function by
function: same / different with the instruction-line counts. Comments, .loc / .file / .cfi lines, blank lines and local
labels' numbers do not count.  tools/kernel_isa_diff.py A.s B.s"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = re.sub(r'\s*(;|//).*$', '', line.rstrip('\n')).strip()
        if not line or re.match(r'\.(loc|file|cfi_\w+|p2align|ident)\b', line):
            continue
        m = re.match(r'\.type\s+(\S+),@function', line)
        if m:
            name, body = m.group(1), []
            continue
        if name and re.match(r'\.Lfunc_end\d+:', line):
            out[name], name = body, None
            continue
        if name and not line.startswith('.L') and not line.endswith(':'):
            body.append(re.sub(r'\.L\w+', '.L', line))
    return out


a, b = functions(sys.argv[1]), functions(sys.argv[2])
short = lambda n: re.sub(r'^_ZN5hsdev\d*', '', n)[:60]
n_same = 0
for n in sorted(set(a) | set(b)):
    if n not in a or n not in b:
        print("%-60s only in %s (%d lines)" % (short(n), sys.argv[2] if n in b else sys.argv[1], len(b.get(n) or a.get(n))))
    elif a[n] == b[n]:
        n_same += 1
    else:
        print("%-60s different  %5d -> %5d lines" % (short(n), len(a[n]), len(b[n])))
print("%d of %d functions the same" % (n_same, len(set(a) | set(b))))
