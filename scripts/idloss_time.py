"""Times the ArcFace identity loss forward + dL/dx on one GPU: the HIP IDLoss (id_loss.IDLoss) against the stock-PyTorch module
with the same weights (loss_heads.IdLoss, MIOpen convs), timed in the same process leg by leg, eager and replayed as a hipGraph:
B=1 with a cached target, B=16 with x and y live (utils_train.py:423), B=16 with y cached.  Then the trainer's direction step
(the body of `bench.py --config trainer`: generator, DECA stand-in, LpipsShaped, Adam) with only the id head swapped, eager as
the bench runs it.
Kernel nodes are counted in the captured graph.  Synthetic weights throughout.

    python scripts/idloss_time.py [--out profiles/idloss_time.txt] [--steps 30] [--only-b16]

--only-b16 runs one B=16 live leg per module (for a rocprofv3 --kernel-trace --stats pass of its own).
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from stylegan_directions_face_reenactment_amd import synthetic as S                     # noqa: E402
from stylegan_directions_face_reenactment_amd import functional as F_                   # noqa: E402
from stylegan_directions_face_reenactment_amd.id_loss import IDLoss                     # noqa: E402
import loss_heads as LH                                                                  # noqa: E402
from lpips_time import graph_nodes, timeit, capture                                     # noqa: E402

SEED = 11


def heads():
    sd = S.synthetic_arcface_state(SEED)
    hip = IDLoss()
    hip.load_state_dict(sd)
    hip = hip.cuda().eval()
    stock = LH.IdLoss()
    stock.facenet.load_state_dict(sd)
    stock = stock.cuda().eval()
    for p in stock.parameters():
        p.requires_grad_(False)
    return hip, stock


def leg(name, loss_of, x, steps, lines):
    xs = x.clone().requires_grad_(True)

    def step():
        xs.grad = None
        loss_of(xs).backward()

    eager = timeit(step, n=steps)
    g = capture(step, clear=[xs])
    rep = timeit(g.replay, n=steps)
    k, n = graph_nodes(g)
    lines.append('%-40s eager %7.3f ms   replayed %7.3f ms   %3d kernel nodes (%d nodes)' % (name, eager, rep, k, n))


def trainer_step_ms(id_head, steps):
    """bench.py run_trainer's step (one GPU, B=16, fp16x3 generator) with `id_head` as the id loss, replayed as one graph."""
    import bench
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    B, dev = 16, torch.device('cuda')
    G, template = bench.generator_state_template(256, 1)
    G.load_state_dict(S.synthetic_state_dict(template, seed=bench.SEED))
    G = G.eval().to(dev)
    for p in G.parameters():
        p.requires_grad_(False)
    torch.manual_seed(bench.SEED)
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False).to(dev)
    lpips, deca = LH.LpipsShaped().to(dev).eval(), LH.ShapeModelStandIn().to(dev).eval()
    for m in (lpips, deca):
        for p in m.parameters():
            p.requires_grad_(False)
    F_.set_precision('fp16x3')
    with torch.no_grad():
        trunc = G.style(S.synthetic_z(bench.SEED, 4096, key='trunc.z').to(dev)).mean(0, keepdim=True)
    opt = torch.optim.Adam(A.parameters(), lr=1e-4, weight_decay=5e-4)                 # trainer.py:145
    shifts = ShiftVectors('voxceleb', 15, 6.0, ranges=bench._direction_ranges())
    zs = S.synthetic_z(bench.SEED, B, key='train.zs').to(dev)
    zt = S.synthetic_z(bench.SEED, B, key='train.zt').to(dev)
    zst = torch.cat([zs, zt])
    out = {}

    def step():
        with torch.no_grad():
            both = generate_image(G, zst, 0.7, trunc, input_is_latent=False, return_latents=False)
            src, tgt = both[:B], both[B:]
            ps, ans = deca(src)
            pt, ant = deca(tgt)
            sv, _ = shifts.make_shift_vector_50(ps, pt, ans, ant)
        img, _ = generate_image(G, zs, 0.7, trunc, shift_code=A(sv), input_is_latent=False, return_latents=True)
        psh, _ = deca(img)
        gt = {'pose': torch.cat([pt['pose'][:B // 2], ps['pose'][B // 2:]]),
              'alpha_exp': torch.cat([pt['alpha_exp'][:B // 2], ps['alpha_exp'][B // 2:]]), 'alpha_shp': ps['alpha_shp']}
        loss = deca.landmark_loss(gt, psh) + 10.0 * id_head(img, src) + 10.0 * lpips(img, src)
        A.zero_grad()
        loss.backward()
        opt.step()
        out['loss'] = loss

    ms = timeit(step, n=steps)
    F_.set_precision('fp32')
    return ms, float(out['loss'])


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 30
    hip, stock = heads()
    x1 = torch.tanh(S.counter_tensor(SEED, 'it.x1', (1, 3, 256, 256))).cuda()
    y1 = torch.tanh(S.counter_tensor(SEED, 'it.y1', (1, 3, 256, 256))).cuda()
    x16 = torch.tanh(S.counter_tensor(SEED, 'it.x16', (16, 3, 256, 256))).cuda()
    y16 = torch.tanh(S.counter_tensor(SEED, 'it.y16', (16, 3, 256, 256))).cuda()
    if '--only-b16' in sys.argv:
        for m in (hip, stock):
            xs = x16.clone().requires_grad_(True)
            for _ in range(3):
                xs.grad = None
                m(xs, y16).backward()
        torch.cuda.synchronize()
        return
    lines = ['ArcFace IR-SE-50 id loss forward + dL/dx, 256x256 -> crop -> 112x112, synthetic weights (%s)' % torch.cuda.get_device_name(0)]
    with torch.no_grad():
        a, b = float(hip(x16, y16)), float(stock(x16, y16))
    lines.append('B=16 loss: HIP %.7g, stock %.7g (rel %.2e)' % (a, b, abs(a - b) / abs(b)))
    t1, t16 = hip.target(y1), hip.target(y16)
    leg('HIP IDLoss B=1, cached target', lambda x: hip(x, t1), x1, steps, lines)
    leg('stock IdLoss B=1 (y recomputed)', lambda x: stock(x, y1), x1, steps, lines)
    leg('HIP IDLoss B=16, x and y live', lambda x: hip(x, y16), x16, steps, lines)
    leg('stock IdLoss B=16, x and y live', lambda x: stock(x, y16), x16, steps, lines)
    leg('HIP IDLoss B=16, cached target', lambda x: hip(x, t16), x16, steps, lines)
    with torch.no_grad():
        yf = stock.feats(y16)
    leg('stock IdLoss B=16, y features cached', lambda x: (1 - torch.nn.functional.cosine_similarity(
        stock.feats(x), yf, dim=1, eps=1e-6)).mean(), x16, steps, lines)
    for name, head in (('HIP IDLoss', hip), ('stock IdLoss', stock)):
        ms, loss = trainer_step_ms(head, max(10, steps // 2))
        lines.append('trainer step B=16 (bench.py --config trainer body, eager), id head %-13s %7.3f ms/step  (loss %.6g)' % (name, ms, loss))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
