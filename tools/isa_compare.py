"""Compare the device ISA of two `hipcc --cuda-device-only -S` outputs line by line, without comments, directives
and the per-compile __hip_cuid_ symbol.

    isa_compare.py a.s b.s                 the whole files
    isa_compare.py --symbols a.s b.s       each mangled _Z... symbol replaced by its ordinal of first appearance (the
                                           name of a kernel changes with the name of an argument's type)
    isa_compare.py --per-kernel a.s b.s    kernel by kernel (--symbols within each kernel), paired by the kernel
                                           template's name and arguments; prints every differing kernel and a count
"""
import difflib
import re
import sys

SYM = re.compile(r"_Z\w+")


def norm(path):
    out = []
    for l in open(path):
        l = l.split(';')[0].rstrip()
        if not l.strip() or l.strip().startswith('.') and not l.strip().startswith('.LBB'):
            continue
        if '__hip_cuid_' in l:
            continue
        out.append(l)
    return out


def ordinals(lines):
    seen = {}
    return [SYM.sub(lambda m: "sym%d" % seen.setdefault(m.group(0), len(seen)), l) for l in lines]


def kernels(lines):
    """{key: lines} of the functions of a file; the key is a template's name and arguments (step_ruleILi1ELi0E),
    which do not change with the argument types' names, or else the symbol."""
    out, cur = {}, None
    for l in lines:
        m = re.match(r"(_Z\w+):$", l)
        if m:
            t = re.search(r"\d+([a-z_]+I(?:L[ib]\d+E)+)E", m.group(1))
            cur = out.setdefault(t.group(1) if t else m.group(1), [])
        if cur is not None:
            cur.append(l)
    return out


def report(a, b):
    print(len(a), len(b), 'identical' if a == b else 'DIFFER')
    if a != b:
        d = list(difflib.unified_diff(a, b, lineterm='', n=0))
        print(len(d))
        print('\n'.join(d[:40]))


def main(argv):
    flags = [x for x in argv if x.startswith('--')]
    paths = [x for x in argv if not x.startswith('--')]
    a, b = norm(paths[0]), norm(paths[1])
    if '--per-kernel' in flags:
        ka, kb = kernels(a), kernels(b)
        if sorted(ka) != sorted(kb):
            print('DIFFER: the kernels are not the same set', sorted(set(ka) ^ set(kb)))
            return
        differing = 0
        for k in ka:
            if ordinals(ka[k]) != ordinals(kb[k]):
                differing += 1
                print('DIFFER', k, len(ka[k]), len(kb[k]))
        print(len(a), len(b), '%d kernels,' % len(ka), 'identical' if not differing else '%d DIFFER' % differing)
    elif '--symbols' in flags:
        report(ordinals(a), ordinals(b))
    else:
        report(a, b)


if __name__ == '__main__':
    main(sys.argv[1:])
