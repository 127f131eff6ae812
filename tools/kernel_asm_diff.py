"""Did a move of kernel code change any kernel?  Compiles the HIP units of two checkouts to gfx950 device assembly with the build's own
flags and compares them per kernel symbol: instruction text (comments stripped, local labels renumbered) and resources (the
.amdhsa_kernel descriptor and the symbol's .set lines: VGPRs, SGPRs, LDS, scratch).  Needs hipcc, no GPU.

    python tools/kernel_asm_diff.py OLD NEW [--units conv_igemm.hip,conv_strip.hip] [--keep DIR]

OLD / NEW: repository roots (their pggan-pytorch_amd/csrc/*.hip are compiled) or directories of *.s files kept by an earlier run.
--units: the units of OLD to account for (default: all).  Every kernel of theirs must exist exactly once in NEW, in any unit, with
identical text and resources, and the units of NEW that hold them may hold no other kernel.  Exit status 1 on any difference."""
import argparse
import collections
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge


def assemble(root, out):
    """root/pggan-pytorch_amd/csrc/*.hip -> out/*.s (all units in parallel, like build())."""
    srcs = sorted(glob.glob(os.path.join(root, 'pggan-pytorch_amd', 'csrc', '*.hip')))
    assert srcs, 'no HIP sources under ' + root
    flags = [f for f in ge.FLAGS if not f.startswith('-I')] + ['-I' + os.path.join(root, 'include')]
    procs = []
    for src in srcs:
        base = os.path.basename(src)
        cmd = [ge.HIPCC] + flags + ge.FILE_FLAGS.get(base, []) + ['-S', '--cuda-device-only', src, '-o', os.path.join(out, base[:-4] + '.s')]
        procs.append((base, subprocess.Popen(cmd, stderr=subprocess.PIPE, universal_newlines=True)))
    for base, p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, (base, err[-2000:])


def kernels(path):
    """{symbol: (text lines, resource lines)} of one .s file."""
    lines = [ln.split(';')[0].rstrip() for ln in open(path)]
    names = [ln.split()[1] for ln in lines if ln.strip().startswith('.amdhsa_kernel ')]
    res = {}
    for name in names:
        begin = lines.index(name + ':')
        end = next(i for i in range(begin, len(lines)) if lines[i].startswith('.Lfunc_end'))
        body, desc, in_desc = [], [], False
        for ln in lines[begin + 1:end]:
            s = ln.strip()
            if s.startswith('.amdhsa_kernel '):
                in_desc = True
            elif s == '.end_amdhsa_kernel':
                in_desc = False
            elif in_desc:
                desc.append(s)
            elif s and not s.startswith(('.section', '.p2align')):
                body.append(s)
        labels = {}                                   # local labels in order of first appearance: their numbers depend on the unit
        text = [re.sub(r'\.L[A-Za-z_]+\d+(_\d+)?', lambda m: labels.setdefault(m.group(0), '.L%d' % len(labels)), ln) for ln in body]
        desc += [ln.strip() for ln in lines if ln.strip().startswith('.set ' + name + '.')]
        res[name] = (text, desc)
    return res


def load(where, keep, tag):
    if not glob.glob(os.path.join(where, '*.s')):
        out = os.path.join(keep, tag) if keep else tempfile.mkdtemp(prefix='asm_' + tag + '_')
        os.makedirs(out, exist_ok=True)
        assemble(where, out)
        where = out
    return {os.path.basename(f)[:-2] + '.hip': kernels(f) for f in sorted(glob.glob(os.path.join(where, '*.s')))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--units', default='')
    ap.add_argument('--keep', default='')
    a = ap.parse_args()
    old, new = load(a.old, a.keep, 'old'), load(a.new, a.keep, 'new')
    units = [u for u in a.units.split(',') if u] or sorted(old)
    where = collections.defaultdict(list)
    for unit, ks in new.items():
        for name in ks:
            where[name].append(unit)
    bad, homes = 0, set()
    for unit in units:
        same = 0
        for name, (text, desc) in sorted(old[unit].items()):
            if len(where[name]) != 1:
                print('%s: %s is in %s' % (unit, name, where[name] or 'no unit'))
                bad += 1
                continue
            homes.add(where[name][0])
            ntext, ndesc = new[where[name][0]][name]
            if (text, desc) == (ntext, ndesc):
                same += 1
                continue
            bad += 1
            print('%s -> %s: %s DIFFERS (%d -> %d instructions and labels)' % (unit, where[name][0], name, len(text), len(ntext)))
            sys.stdout.writelines(ln + '\n' for ln in difflib.unified_diff(desc + text, ndesc + ntext, 'old', 'new', lineterm='', n=2))
        print('%-22s %3d kernels, %3d identical' % (unit, len(old[unit]), same))
    known = set(name for unit in units for name in old[unit])
    for unit in sorted(homes):
        extra = sorted(set(new[unit]) - known)
        print('%-22s %3d kernels%s' % ('-> ' + unit, len(new[unit]), ', NEW SYMBOLS: ' + ' '.join(extra) if extra else ''))
        bad += len(extra)
    print('DIFFERENT' if bad else 'identical')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
