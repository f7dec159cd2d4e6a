"""Times one shape-loss call (both decodes, the three terms, backward to the reenacted coefficients) at rows = 16, the trainer's
per-rank batch, on one GPU: flame.ShapeLoss against the stock-PyTorch fp32 composition with the same tables (flame_stock.py), each
eager and replayed as a hipGraph, in one process, alternating.  Device-event times over enough calls to fill a second per leg; the
whole set is repeated and the spread of the repeats is printed.  Device kernels per call come from torch.profiler.

    python scripts/shape_loss_time.py [--out profiles/shape_loss_time.txt] [--rows 16] [--repeats 5]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from stylegan_directions_face_reenactment_amd import synthetic as S                     # noqa: E402
from stylegan_directions_face_reenactment_amd import flame as FL                        # noqa: E402
from flame_stock import StockShapeLoss                                                   # noqa: E402
from lpips_time import capture, graph_nodes                                              # noqa: E402

SEED = 12


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def kernels_per_call(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
    return len(names), sum('flame_' in n for n in names)


def main():
    arg = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d      # noqa: E731
    out, rows, repeats = arg('--out', ''), arg('--rows', 16), arg('--repeats', 5)
    sd = S.synthetic_flame_state(SEED)
    m = FL.FLAME()
    m.load_state_dict(sd)
    hip = FL.ShapeLoss(m.cuda())
    stock = StockShapeLoss({k: v for k, v in sd.items() if k not in ('eye_pose', 'neck_pose')}).cuda()
    gt = {k: v.cuda() for k, v in S.synthetic_flame_coeffs(SEED, 'slt.gt', rows, [0.1 * (i - rows / 2) for i in range(rows)]).items()}
    reen = {k: v.cuda().requires_grad_(k != 'cam') for k, v in
            S.synthetic_flame_coeffs(SEED, 'slt.re', rows, [0.09 * (rows / 2 - i) for i in range(rows)]).items()}
    leaves = [reen[k] for k in ('shape', 'exp', 'pose')]

    def step_of(loss_of):
        def step():
            for t in leaves:
                t.grad = None
            loss_of().backward()
        return step

    steps = {'HIP ShapeLoss': step_of(lambda: hip(gt, reen)[0]), 'stock composition': step_of(lambda: stock(gt, reen))}
    lines = ['shape / mouth / eye loss forward + backward to the reenacted coefficients, rows = %d, synthetic FLAME (%s)'
             % (rows, torch.cuda.get_device_name(0))]
    vals, grads = {}, {}
    for name, step in steps.items():
        step()
        vals[name] = float(hip(gt, reen)[0]) if name.startswith('HIP') else float(stock(gt, reen))
        grads[name] = torch.cat([t.grad.flatten() for t in leaves]).double()
    a, b = grads['HIP ShapeLoss'], grads['stock composition']
    lines.append('loss: HIP %.7g, stock %.7g (rel %.2e); gradient rel %.2e' % (vals['HIP ShapeLoss'], vals['stock composition'],
                 abs(vals['HIP ShapeLoss'] - vals['stock composition']) / abs(vals['stock composition']), float((a - b).abs().max() / b.abs().max())))
    legs = {}
    for name, step in steps.items():
        total, own = kernels_per_call(step)
        g = capture(step, clear=leaves)
        k, n = graph_nodes(g)
        lines.append('%-18s %3d device kernels per eager call (%d from csrc/flame.hip); captured graph: %d kernel nodes (%d nodes)'
                     % (name, total, own, k, n))
        legs[name + ', eager'] = step
        legs[name + ', replayed'] = g.replay
    calls = {}
    for name, fn in legs.items():
        one = event_ms(fn, 20)
        calls[name] = max(20, int(1000.0 / max(one, 1e-3)))
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():                    # alternating: every leg once per repeat
            times[name].append(event_ms(fn, calls[name]))
    for name, ts in times.items():
        ts = sorted(ts)
        lines.append('%-30s median %8.4f ms   min %8.4f   max %8.4f   (%d calls x %d repeats)' % (name, ts[len(ts) // 2], ts[0], ts[-1], calls[name], repeats))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    lines.append('ratio stock / HIP: eager %.2f, replayed %.2f; HIP eager against stock replayed %.2f'
                 % (med['stock composition, eager'] / med['HIP ShapeLoss, eager'], med['stock composition, replayed'] / med['HIP ShapeLoss, replayed'],
                    med['stock composition, replayed'] / med['HIP ShapeLoss, eager']))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
