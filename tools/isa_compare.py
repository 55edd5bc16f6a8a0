#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two builds of one source of csrc/ (kernels.hip unless --source names another; gfx950 ISA as
the compiler emits it), no GPU needed: the proof that a refactor left the generated code alone.

    python tools/isa_compare.py OLD NEW --work DIR [--source NAME.hip] [--out TABLE.txt]

OLD / NEW: a `.s` file (hipcc -S --cuda-device-only), or a source tree, whose csrc/NAME.hip is compiled into DIR with the flags
of mycroft_precise_amd/_build.py.  For every kernel, keyed by mangled name: `identical` when the instruction streams agree
after label normalisation; otherwise the instruction counts, next_free_vgpr / next_free_sgpr / group_segment_fixed_size /
private_segment_fixed_size of both sides and the opcodes whose counts differ -- `same-shape` when all of those agree (only
registers or the order of instructions moved), `DIFFERENT` when not.  Kernels on one side only are listed by name.
Exit status 1 if any kernel is DIFFERENT or has scratch where the old one had none."""
import argparse, ast, collections, os, re, shutil, subprocess, sys

RESOURCES = ('next_free_vgpr', 'next_free_sgpr', 'group_segment_fixed_size', 'private_segment_fixed_size')


def build_flags(tree):
    text = open(os.path.join(tree, 'mycroft_precise_amd', '_build.py')).read()
    flags = ast.literal_eval(re.search(r'^FLAGS = (\[.*?\])', text, re.M | re.S).group(1))
    return [f for f in flags if f not in ('-fPIC', '-Wall', '-Wno-unused-function')]


def assembly(path, work, tag, source):
    if os.path.isfile(path):
        return open(path).read()
    out = os.path.join(work, tag + '_' + os.path.splitext(source)[0] + '.s')
    src = os.path.join(path, 'mycroft_precise_amd', 'csrc', source)
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'          # (as _build.py finds it)
    subprocess.run([hipcc] + build_flags(path) + ['--cuda-device-only', '-S', src, '-o', out], check=True)
    return open(out).read()


def kernels(text):
    """mangled name -> (normalised instruction lines, resources)"""
    res = collections.defaultdict(dict)
    for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', text, re.S):
        for key in RESOURCES:
            v = re.search(r'\.amdhsa_%s (\S+)' % key, m.group(2))
            res[m.group(1)][key] = v.group(1) if v else '?'
    out = {}
    for name in res:
        m = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:' % re.escape(name), text, re.M | re.S)
        labels, lines = {}, []
        for line in m.group(1).split('\n'):
            line = re.sub(r'\s*;.*', '', line).strip()
            if not line or line.startswith('.') and not line.endswith(':'):
                continue
            if line.endswith(':'):
                labels.setdefault(line[:-1], 'L%d' % len(labels))
                line = labels[line[:-1]] + ':'
            lines.append(line)
        # branch targets by order of first definition (the numbering of .LBB labels depends on the kernel's place in the file)
        lines = [re.sub(r'\.?LBB\w+', lambda t: labels.get(t.group(0), t.group(0)), l) for l in lines]
        out[name] = (lines, res[name])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old'), ap.add_argument('new')
    ap.add_argument('--work', required=True, help='directory for the compiled .s files')
    ap.add_argument('--source', default='kernels.hip', help='the file of mycroft_precise_amd/csrc to compile (default kernels.hip)')
    ap.add_argument('--out', help='also write the table here')
    args = ap.parse_args()
    os.makedirs(args.work, exist_ok=True)
    old, new = (kernels(assembly(p, args.work, tag, args.source)) for p, tag in ((args.old, 'old'), (args.new, 'new')))
    rows, tally, bad = [], collections.Counter(), 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict, detail = ('only-new' if name in new else 'only-old'), ''
        else:
            (lo, ro), (ln, rn) = old[name], new[name]
            ops_o = collections.Counter(l.split()[0] for l in lo if not l.endswith(':'))
            ops_n = collections.Counter(l.split()[0] for l in ln if not l.endswith(':'))
            if lo == ln and ro == rn:
                verdict, detail = 'identical', ''
            else:
                same = ops_o == ops_n and ro == rn
                verdict = 'same-shape' if same else 'DIFFERENT'
                changed = sum(1 for a, b in zip(lo, ln) if a != b) + abs(len(lo) - len(ln))
                detail = 'instructions %d / %d, lines that differ %d; ' % (sum(ops_o.values()), sum(ops_n.values()), changed)
                detail += ' '.join('%s %s / %s' % (k.replace('_fixed_size', ''), ro[k], rn[k]) for k in RESOURCES)
                diff = ['%s %d / %d' % (op, ops_o[op], ops_n[op]) for op in sorted(set(ops_o) | set(ops_n)) if ops_o[op] != ops_n[op]]
                detail += '; opcode counts ' + ('equal' if not diff else ', '.join(diff))
                if not same or (ro['private_segment_fixed_size'] == '0' and rn['private_segment_fixed_size'] != '0'):
                    bad += 1
        tally[verdict] += 1
        demangled = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
        demangled = re.sub(r'\(.*', '', demangled).replace('void pe::', '')
        rows.append('%-10s %s\n           %s%s' % (verdict, name, demangled, ('\n           ' + detail) if detail else ''))
    head = 'kernels: %d old, %d new; %s   (old / new in every pair of numbers)' % (
        len(old), len(new), ', '.join('%d %s' % (n, v) for v, n in sorted(tally.items())))
    table = head + '\n' + '\n'.join(rows) + '\n'
    sys.stdout.write(table)
    if args.out:
        open(args.out, 'w').write(table)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
