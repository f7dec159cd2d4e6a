"""Times LPIPS-alex forward + dL/dx on one GPU: the HIP LPIPS (lpips.LPIPS) against the stock-PyTorch restatement with the same
math (loss_heads.LpipsShaped), eager and replayed as a hipGraph, at B=1 with a cached target (PTI) and at B=16 with both inputs
live (the trainer's shape); then the replayed PTI step (finetune.optimize_g's step) with the L2 stand-in, with PtiLoss and with
LpipsShaped in PtiLoss's place.  Launch counts are the kernel nodes of the captured graph.  Synthetic weights throughout.

    python scripts/lpips_time.py [--out profiles/lpips_time.txt]
"""
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from stylegan_directions_face_reenactment_amd import synthetic as S, finetune          # noqa: E402
from stylegan_directions_face_reenactment_amd import functional as F_                  # noqa: E402
from stylegan_directions_face_reenactment_amd.lpips import LPIPS                       # noqa: E402
from stylegan_directions_face_reenactment_amd.model import Generator                   # noqa: E402
from loss_heads import LpipsShaped                                                      # noqa: E402

_hip = None


def graph_nodes(g):
    """Kernel nodes of a captured torch CUDAGraph (hipGraphGetNodes + hipGraphNodeGetType)."""
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL('libamdhip64.so')
    raw = ctypes.c_void_p(g.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    _hip.hipGraphGetNodes(raw, None, ctypes.byref(n))
    nodes = (ctypes.c_void_p * n.value)()
    _hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n))
    kern = 0
    for nd in nodes:
        t = ctypes.c_int(-1)
        _hip.hipGraphNodeGetType(ctypes.c_void_p(nd), ctypes.byref(t))
        kern += int(t.value == 0)           # hipGraphNodeTypeKernel
    return kern, n.value


def timeit(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def capture(step, clear=()):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for t in clear:
        t.grad = None
    g = torch.cuda.CUDAGraph(keep_graph=True)        # keep the hipGraph_t for the node count
    with F_.capture_graph(g):
        step()
    g.instantiate()
    return g


def loss_leg(name, loss_of, x, lines):
    xs = x.clone().requires_grad_(True)

    def step():
        xs.grad = None
        loss_of(xs).backward()

    eager = timeit(step)
    g = capture(step, clear=[xs])
    rep = timeit(g.replay)
    k, n = graph_nodes(g)
    lines.append('%-44s eager %7.3f ms   replayed %7.3f ms   %3d kernel nodes (%d nodes)' % (name, eager, rep, k, n))
    return rep


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    torch.manual_seed(0)
    sd = S.synthetic_lpips_state(7)
    hip = LPIPS()
    hip.load_state_dict(sd)
    hip = hip.cuda()
    ref = LpipsShaped().cuda()
    with torch.no_grad():
        for t, i in enumerate((0, 3, 6, 8, 10)):
            conv = ref.slices[t][1] if t in (1, 2) else ref.slices[t][0]
            conv.weight.copy_(sd['net.layers.%d.weight' % i])
            conv.bias.copy_(sd['net.layers.%d.bias' % i])
            ref.lin[t].weight.copy_(sd['lin.%d.1.weight' % t])
    for p in ref.parameters():
        p.requires_grad_(False)
    lines = ['LPIPS-alex forward + dL/dx, 256x256, synthetic weights (%s)' % torch.cuda.get_device_name(0)]
    x1 = torch.tanh(S.counter_tensor(7, 'lt.x1', (1, 3, 256, 256))).cuda()
    y1 = torch.tanh(S.counter_tensor(7, 'lt.y1', (1, 3, 256, 256))).cuda()
    x16 = torch.tanh(S.counter_tensor(7, 'lt.x16', (16, 3, 256, 256))).cuda()
    y16 = torch.tanh(S.counter_tensor(7, 'lt.y16', (16, 3, 256, 256))).cuda()
    with torch.no_grad():
        a, b = float(hip(x16, y16)), float(ref(x16, y16))
    lines.append('B=16 loss: HIP %.7g, LpipsShaped %.7g (rel %.2e)' % (a, b, abs(a - b) / abs(b)))
    tgt = hip.target(y1)
    loss_leg('HIP LPIPS B=1, cached target', lambda x: hip(x, tgt), x1, lines)
    loss_leg('LpipsShaped B=1 (y recomputed)', lambda x: ref(x, y1), x1, lines)
    loss_leg('HIP LPIPS B=16, x and y live', lambda x: hip(x, y16), x16, lines)
    loss_leg('LpipsShaped B=16', lambda x: ref(x, y16), x16, lines)

    # the PTI step: generator forward, backward, one-launch Adam, replayed as one graph
    G0 = Generator(256, 512, 8, channel_multiplier=1)
    G0.load_state_dict(S.synthetic_state_dict(G0.state_dict(), seed=7))
    G0 = G0.train().cuda()
    trunc = S.counter_tensor(7, 'trunc', (1, 512)).cuda()
    latent = S.synthetic_latents(7, 1, n_latent=G0.n_latent, key='pti.w').cuda()
    target = torch.tanh(S.counter_tensor(7, 'pti.t', (1, 3, 256, 256))).cuda()

    def shaped_loss(imgs, real, lam):
        return torch.nn.functional.mse_loss(imgs, real) * lam + ref(imgs, real)

    import copy
    for name, make in (('L2 only (l2_loss_fn)', lambda: finetune.l2_loss_fn), ('PtiLoss (HIP LPIPS)', lambda: finetune.PtiLoss(hip, target)),
                       ('100 MSE + LpipsShaped', lambda: shaped_loss)):
        G = copy.deepcopy(G0)
        params, lam = finetune.pti_parameters(G)
        opt = finetune.FusedAdam(params, lr=3e-3)
        loss_fn = make()

        def step():
            img, _ = G([latent], input_is_latent=True, return_latents=False, truncation=0.7, truncation_latent=trunc)
            loss = loss_fn(img, target, lam)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        g = capture(step, clear=list(G.parameters()))
        rep = timeit(g.replay, n=40)
        k, n = graph_nodes(g)
        lines.append('PTI step replayed, %-26s %7.3f ms   %3d kernel nodes (%d nodes)' % (name, rep, k, n))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
