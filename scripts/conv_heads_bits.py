"""Do two builds of the library compute the same bits in the five conv heads (csrc/idloss.hip, deca.hip, fan.hip, s3fd.hip, e4e.hip on
csrc/conv_tile.h)?  One fresh child process per library runs the cases below through the package's entry points on synthetic.py
weights and saves every output as .npy; the parent compares the two sets as uint32 and exits non-zero on the first difference (or,
before that, on a child that did not end cleanly: nothing more is started then).  Each head runs convs split over K (finish kernel)
and whole (epilogue in the conv kernel), pixel-edge tiles (M no multiple of 64) and channel-edge tiles (N no multiple of the tile).

    python scripts/build_ref.py <commit>                  # csrc/libsgdfr_hip_ref.so from another commit
    python scripts/conv_heads_bits.py [csrc/libsgdfr_hip_ref.so] [--out DIR] [--heads idloss,deca,fan,s3fd,e4e]

Cases: id-loss forward + dL/dx at B = 1 and 33; DECA forward + dL/dx at B = 1 and 5; the FAN network with its debug taps at B = 1
and 5; S3FD with maps and debug taps at B = 1 on 32 x 48 and B = 3 on 72 x 104; the e4e encoder at R = 32, B = 1 and R = 64, B = 3.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261018
HEADS = ('idloss', 'deca', 'fan', 's3fd', 'e4e')


def flatten(prefix, v, out):
    """Every tensor of nested tuples / lists / dicts under a dotted name."""
    import torch
    if v is None:
        return
    if isinstance(v, torch.Tensor):
        out[prefix] = v
    elif isinstance(v, dict):
        for k in v:
            flatten('%s.%s' % (prefix, k), v[k], out)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            flatten('%s.%d' % (prefix, i), x, out)
    else:
        raise TypeError('%s: %r' % (prefix, type(v)))


def run_idloss(S, out):
    import torch
    from stylegan_directions_face_reenactment_amd import id_loss as I
    head = I.IDLoss()
    head.load_state_dict(S.synthetic_arcface_state(SEED))
    head = head.cuda().eval()
    for B in (1, 33):
        x = torch.tanh(S.counter_tensor(SEED, 'bits.id.x%d' % B, (B, 3, 256, 256))).cuda().requires_grad_(True)
        y = torch.tanh(S.counter_tensor(SEED, 'bits.id.y%d' % B, (B, 3, 256, 256))).cuda()
        ex, ey = I.embed(head.facenet, x, y)
        ex.backward(S.counter_tensor(SEED, 'bits.id.g%d' % B, (B, 512)).cuda())
        flatten('idloss.b%d' % B, {'ex': ex, 'ey': ey, 'dx': x.grad}, out)


def run_deca(S, out):
    import torch
    from stylegan_directions_face_reenactment_amd import deca as D
    E = D.ResnetEncoder()
    E.load_state_dict(S.synthetic_deca_encoder_state(SEED))
    E = E.cuda().eval()
    for B in (1, 5):
        x = torch.tanh(S.counter_tensor(SEED, 'bits.deca.x%d' % B, (B, 3, 256, 256))).cuda().requires_grad_(True)
        M = D.crop_matrix(torch.tensor([[60.0, 70.0, 196.0, 206.0]]).repeat(B, 1), (256, 256)).cuda()
        params, angles, crop = D.run(E, x, M)
        params.backward(S.counter_tensor(SEED, 'bits.deca.g%d' % B, (B, 236)).cuda())
        flatten('deca.b%d' % B, {'params': params, 'angles': angles, 'crop': crop, 'dx': x.grad}, out)


def run_fan(S, out):
    import torch
    from stylegan_directions_face_reenactment_amd import landmarks as L
    fan = L.FAN(4)
    fan.load_state_dict(S.synthetic_fan_state(SEED))
    fan = fan.cuda().eval()
    for B in (1, 5):
        x = S.counter_tensor(SEED, 'bits.fan.x%d' % B, (B, 3, 256, 256), 127.5, 60.0).clamp(0, 255).cuda()
        faces = torch.tensor([[52.0, 40.0, 204.0, 222.0]]).repeat(B, 1).cuda()
        flatten('fan.b%d' % B, L.run_debug(fan, x, faces), out)


def run_s3fd(S, out):
    import torch
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    det = FD.S3FD()
    det.load_state_dict(S.synthetic_s3fd_state(SEED))
    det = det.cuda()
    for B, H, W in ((1, 32, 48), (3, 72, 104)):
        x = S.counter_tensor(SEED, 'bits.s3fd.x%d' % B, (B, 3, H, W), 127.5, 60.0).clamp(0, 255).cuda()
        r = FD.run_debug(det, x)
        # the entry point defines boxes / index up to each image's `kept` count only; the tails are memory that was never written, so
        # they are zeroed in both children (a write past `kept` would therefore not be seen here)
        live = torch.arange(r['boxes'].shape[1], device=x.device)[None, :] < r['kept'][:, None]
        r['boxes'] = torch.where(live[:, :, None], r['boxes'], torch.zeros_like(r['boxes']))
        r['index'] = torch.where(live, r['index'], torch.zeros_like(r['index']))
        flatten('s3fd.b%d_%dx%d' % (B, H, W), r, out)


def run_e4e(S, out):
    import torch
    from stylegan_directions_face_reenactment_amd import encoder as E
    for R, B in ((32, 1), (64, 3)):
        enc = E.Encoder4Editing(50, 'ir_se', R).eval()
        enc.load_state_dict(S.synthetic_encoder_state(enc.state_dict(), seed=SEED), strict=True)
        enc = enc.cuda()
        x = S.counter_tensor(SEED, 'bits.e4e.x%d' % R, (B, 3, R, R), 0.0, 0.5).clamp_(-1, 1).cuda()
        with torch.no_grad():
            flatten('e4e.r%d_b%d' % (R, B), {'w': E.encode(enc, x)}, out)


def child(outdir, heads):
    import numpy as np
    import torch
    from stylegan_directions_face_reenactment_amd import synthetic as S
    for h in heads:
        out = {}
        globals()['run_' + h](S, out)
        torch.cuda.synchronize()
        for name, t in out.items():
            np.save(os.path.join(outdir, name + '.npy'), t.detach().cpu().contiguous().numpy())
        print('%s: %d arrays' % (h, len(out)), flush=True)


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    heads = arg('--heads', ','.join(HEADS)).split(',')
    assert all(h in HEADS for h in heads), heads
    if '--child' in sys.argv:
        return child(arg('--child', None), heads)
    import numpy as np
    from stylegan_directions_face_reenactment_amd import build_native as b
    ref = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith('--') else os.path.join(b.CSRC, 'libsgdfr_hip_ref.so')
    assert os.path.exists(ref), ref + ' (python scripts/build_ref.py <commit> builds it)'
    base = arg('--out', None) or tempfile.mkdtemp()
    dirs = {}
    for tag, lib in (('ref', os.path.abspath(ref)), ('new', None)):
        dirs[tag] = os.path.join(base, tag)
        os.makedirs(dirs[tag], exist_ok=True)
        env = dict(os.environ)
        env.pop('SGDFR_LIB', None)
        if lib:
            env.update(SGDFR_LIB=lib, SGDFR_ALLOW_LIB_OVERRIDE='1')
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', dirs[tag], '--heads', ','.join(heads)], env=env)
        if r.returncode != 0:
            print('%s: the child ended with status %d; nothing more is started' % (tag, r.returncode))
            return 2
    names = sorted(os.listdir(dirs['ref']))
    if names != sorted(os.listdir(dirs['new'])) or not names:
        print('the two runs saved different sets of arrays')
        return 1
    for n in names:
        p, q = np.load(os.path.join(dirs['ref'], n)), np.load(os.path.join(dirs['new'], n))
        same = p.shape == q.shape and p.dtype == q.dtype and np.array_equal(p.view(np.uint32) if p.dtype.itemsize == 4 else p,
                                                                            q.view(np.uint32) if q.dtype.itemsize == 4 else q)
        if not same:
            print('DIFFERENT: %s %s %s' % (n, p.shape, q.shape))
            return 1
    print('%d arrays (%s), %d values: all equal between %s and the current library' % (
        len(names), ', '.join(heads), sum(int(np.load(os.path.join(dirs['new'], n)).size) for n in names), os.path.basename(ref)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
