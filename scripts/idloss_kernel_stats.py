"""Kernel table of a `rocprofv3 --kernel-trace --stats` pass over `scripts/idloss_time.py --only-b16` (three B=16 calls of the HIP
IDLoss with x and y live, then three of the stock module): per-kernel totals as CSV, and each HIP conv family's achieved TFLOP/s
(useful FLOPs from the layer shapes / kernel time) against the 157.3 TF exact-f32 MFMA peak.

    python scripts/idloss_kernel_stats.py <results.db> profiles/idloss_kernel_stats.csv
"""
import csv
import re
import sqlite3
import sys

CALLS, B, R = 3, 16, 32          # calls per module in the pass; x rows; x + y rows
UNITS = [(c, d, 2 if u == 0 else 1) for c, d, n in ((64, 64, 3), (64, 128, 4), (128, 256, 14), (256, 512, 3))
         for u, c in zip(range(n), [c] + [d] * (n - 1))]


def family_flops():
    """Useful FLOPs of one call per idl_conv_kernel<TAP, KS, LOAD, EXT> instance."""
    f = {'<0, 3, 0, false>': 2 * R * 112 * 112 * 64 * 27, '<0, 3, 1, false>': 0, '<0, 3, 2, false>': 0,
         '<0, 1, 0, false>': 2 * R * 25088 * 512 + 2 * B * 25088 * 512, '<1, 3, 1, false>': 0, '<1, 3, 0, false>': 0,
         '<1, 3, 0, true>': 0}
    h = 112
    for cin, d, s in UNITS:
        ho = (h - 1) // s + 1
        f['<0, 3, 1, false>'] += 2 * R * h * h * d * cin * 9
        f['<0, 3, 2, false>'] += 2 * R * ho * ho * d * d * 9
        f['<1, 3, 1, false>'] += 2 * B * ho * ho * d * d * 9
        if cin != d:
            f['<0, 1, 0, false>'] += 2 * R * ho * ho * d * cin
            f['<1, 3, 0, true>'] += 2 * B * h * h * cin * d * 9 + 2 * B * ho * ho * d * cin
        else:
            f['<1, 3, 0, false>'] += 2 * B * h * h * cin * d * 9
        h = ho
    return f


NAMES = {'<0, 3, 0, false>': 'stem conv', '<0, 3, 1, false>': 'conv1 (BN1 in load)', '<0, 3, 2, false>': 'conv2 (PReLU in load)',
         '<0, 1, 0, false>': 'shortcut 1x1 + head GEMMs', '<1, 3, 1, false>': 'conv2 dgrad (SE adjoint in load)',
         '<1, 3, 0, false>': 'conv1 dgrad', '<1, 3, 0, true>': 'conv1 + shortcut dgrad'}


def short(n):
    n = n.replace('(anonymous namespace)::', '').replace('void ', '')
    return re.sub(r'\(.*', '', n)[:120]


def main():
    db, out = sys.argv[1], sys.argv[2]
    c = sqlite3.connect(db)
    rows = c.execute('select name, count(*), sum(duration) from kernels group by name order by sum(duration) desc').fetchall()
    hip = [(n, k, t) for n, k, t in rows if 'idl_' in n]
    stock = [(n, k, t) for n, k, t in rows if 'idl_' not in n and 'pack' not in n]
    with open(out, 'w', newline='') as fh:
        w = csv.writer(fh)
        w.writerow(['module', 'kernel', 'dispatches_per_call', 'us_per_call', 'share'])
        for tag, group in (('hip', hip), ('stock', stock)):
            tot = sum(t for _, _, t in group)
            for n, k, t in group:
                w.writerow([tag, short(n), k / CALLS, round(t / CALLS / 1e3, 1), round(t / tot, 4)])
    tot_h = sum(t for _, _, t in hip) / CALLS / 1e6
    tot_s = sum(t for _, _, t in stock) / CALLS / 1e6
    print('kernel time per B=16 call (x and y live, forward + dL/dx): HIP %.2f ms, stock %.2f ms' % (tot_h, tot_s))
    fl = family_flops()
    for key, name in NAMES.items():
        t = sum(tt for n, _, tt in hip if 'idl_conv_kernel' in n and key.replace(' ', '') in n.replace(' ', '')) / CALLS
        if t:
            tf = fl[key] / (t * 1e-9) / 1e12
            print('  %-34s %7.2f ms  %6.1f GFLOP  %5.1f TFLOP/s  (%.2f of 157.3)' % (name, t / 1e6, fl[key] / 1e9, tf, tf / 157.3))
    for n, k, t in hip:
        if 'idl_conv_kernel' not in n:
            print('  %-34s %7.2f ms  %d dispatches' % (short(n).split('::')[-1][:34], t / CALLS / 1e6, k // CALLS))


if __name__ == '__main__':
    main()
