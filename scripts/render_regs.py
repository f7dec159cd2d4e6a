"""Registers, LDS and scratch of every kernel of csrc/shaperender.hip, texture.hip and detail.hip at two states of the tree, side by
side: the three files are compiled with build_native.FLAGS plus -save-temps and the kernels' resource lines (.vgpr_count, .sgpr_count,
.group_segment_fixed_size, .private_segment_fixed_size) are read from the metadata the compiler writes; nothing else of its output is
looked at.  Needs hipcc only, no GPU.

    python scripts/render_regs.py [<commit, default HEAD>] [--out profiles/render_regs.txt]

Left: the commit; right: the working tree.  The waves per SIMD are 512 // (VGPRs rounded up to 8), at most 8.  Exit status 1 when a
kernel of the working tree has scratch where the commit has none, more LDS, or fewer waves per SIMD.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILES = ('shaperender.hip', 'texture.hip', 'detail.hip')
KEYS = ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')


def resources(csrc, b):
    """{file: {demangled kernel: (vgpr, sgpr, lds, scratch)}} of the three files under `csrc`."""
    out = {}
    for name in FILES:
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.run([b._hipcc()] + b.FLAGS + ['-save-temps', '-c', os.path.join(csrc, name), '-o', os.path.join(tmp, 'x.o')],
                           cwd=tmp, check=True, capture_output=True)
            asm, = [f for f in os.listdir(tmp) if f.endswith('.s') and 'amdgcn' in f]
            text = open(os.path.join(tmp, asm)).read()
        meta = text[text.index('amdhsa.kernels:'):]
        rows = {}
        for block in re.split(r'(?m)^  - ', meta)[1:]:
            if '.vgpr_count:' not in block:              # the lists after the kernels (amdhsa.version)
                continue
            get = lambda key: re.search(r'(?m)^\s+%s:\s+(\S+)' % re.escape(key), '    ' + block).group(1)
            kernel = subprocess.run(['c++filt', get('.name')], capture_output=True, text=True).stdout.strip()
            kernel = re.sub(r'^void ', '', re.sub(r'sgdfr::\(anonymous namespace\)::', '', kernel))
            rows[re.sub(r'\(.*', '', kernel)] = tuple(int(get(k)) for k in KEYS)
        out[name] = rows
    return out


def waves(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def main():
    from stylegan_directions_face_reenactment_amd import build_native as b
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    if out in args:
        args.remove(out)
    commit = args[0] if args else 'HEAD'
    rel = os.path.relpath(b.CSRC, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run('git archive %s %s include | tar -x -C %s' % (commit, rel, tmp), shell=True, check=True, cwd=ROOT)
        old = resources(os.path.join(tmp, rel), b)
    new = resources(b.CSRC, b)
    sha = subprocess.run(['git', 'rev-parse', '--short', commit], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    fmt = lambda r: '%4d %4d %6d %4d %2d' % (r + (waves(r[0]),)) if r else '%24s' % '-'
    lines = ['kernel resources, %s: commit %s | working tree; columns: VGPRs SGPRs LDS-bytes scratch-bytes waves/SIMD' % (' '.join(b.FLAGS), sha)]
    bad = 0
    for name in FILES:
        lines.append(name)
        for k in sorted(set(old[name]) | set(new[name])):
            p, q = old[name].get(k), new[name].get(k)
            worse = bool(p and q and ((q[3] > 0 and p[3] == 0) or q[2] > p[2] or waves(q[0]) < waves(p[0])))
            bad += worse
            lines.append('  %-66s %s | %s%s' % (k[:66], fmt(p), fmt(q), '   WORSE' if worse else ''))
    print('\n'.join(lines))
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
