"""Do two builds of the library compute the same bits in the mesh kernels (csrc/shaperender.hip, texture.hip's UV pass, detail.hip's UV
space)?  One fresh child process per library runs the cases below through the package's entry points on seeded inputs and saves every
output tensor to one .npz; the parent compares the two files tensor by tensor on the raw bytes and prints one line each.  Exit status
1 on any difference, 2 when a child did not end cleanly (nothing more is started then).

    python scripts/build_ref.py <commit> && cp .../csrc/libsgdfr_hip_ref.so build/libsgdfr_hip_parent.so
    python scripts/render_bits.py [build/libsgdfr_hip_parent.so] [--out profiles/render_bits.txt]

Cases, the smallest that cross every seam of the raster kernel:
  lattice   tests/shape_render_cases.lattice_grid (513 faces: two chunks of 256), wound towards the camera, at S = 17 (a partial
            16 x 16 tile on both axes), rows 1 and 3: rasterize; render_shape with the default lights, with lights [1,5,6] and [B,8,6], over a background with
            gan_range off and on; the detail outputs at Su = 13 and 32; render_texture with SH lights, without, and with albedo=None;
            the attribute render at D = 1, 2, 3 and render_depth; world2uv, detail_normals (with the dense vertices) and uv_textures
            with and without an albedo at Su = 13 and 32
  flame     the synthetic FLAME mesh at S = 32, rows 2, through cam and through projected: render_shape (with the detail outputs)
            and render_texture
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEED = 20261020
SHAPE_ALL = ('shape', 'alpha', 'pix_to_face', 'zbuf', 'bary')
DETAIL_ALL = SHAPE_ALL + ('shape_detail', 'grid', 'detail_normal_images')
UV_ALL = ('uv_shading', 'uv_texture', 'uv_texture_gt', 'uv_pverts', 'uv_gt')


def run_cases(put):
    import torch
    import torch.nn.functional as F
    import shape_render_cases as C
    from stylegan_directions_face_reenactment_amd import detail as DT, flame as FL, shape_render as SR, synthetic as S, texture as TX
    draw = lambda key, shape, mean=0.0, std=1.0: S.counter_tensor(SEED, 'render_bits.' + key, shape, mean, std)

    def maps(tag, B, Su, size):
        light = draw(tag + '.light', (B, 9, 3), 0.0, 0.3)
        light[:, 0] += 2.5
        return (draw(tag + '.albedo', (B, 3, Su, Su), 0.5, 0.2).cuda(), F.normalize(draw(tag + '.uvn', (B, 3, Su, Su)), dim=1).cuda(), light.cuda(),
                draw(tag + '.images', (B, 3, size, size), 0.5, 0.2).cuda())

    def texture_cases(tag, verts, topo, L, albedo, light, **view):
        wanted = SR._WANT_TEXTURE
        put(tag + '.sh', SR.render_texture(verts, topo, L, albedo, lights=light, want=wanted, **view))
        put(tag + '.nolight', SR.render_texture(verts, topo, L, albedo, lights=None, want=wanted, **view))
        put(tag + '.noalbedo', SR.render_texture(verts, topo, L, None, lights=light,
                                                 want=[w for w in wanted if w not in ('images', 'albedo_images')], **view))

    # ---- the lattice grid
    pv, faces = C.lattice_grid()
    faces = faces[:, [0, 2, 1]]                          # wound so that the projected normals face the camera: alpha and pos_mask are 1
    V, size = pv.shape[0], 17
    topo = SR.MeshTopology(faces, V)
    uv = pv[:, :2] / 8.0 + 0.5
    for B in (1, 3):
        tag = 'lattice.b%d' % B
        p = pv.float()[None].repeat(B, 1, 1)
        p[:, :, :2] += 0.013 * torch.arange(B, dtype=torch.float32)[:, None, None]
        verts = (p * torch.tensor([1.0, -1.0, -1.0]) + draw(tag + '.bend', (B, V, 3), 0.0, 0.02)).cuda()
        p = p.cuda()
        bg = draw(tag + '.bg', (B, 3, size, size), 0.5, 0.4).cuda()
        put(tag + '.rasterize', SR.rasterize(p, topo, size))
        put(tag + '.shape', SR.render_shape(verts, topo, projected=p, size=size, want=SHAPE_ALL))
        for name, lights in (('l1x5', draw(tag + '.l5', (1, 5, 6))), ('lBx8', draw(tag + '.l8', (B, 8, 6)))):
            for gan in (False, True):
                put('%s.shape.%s.gan%d' % (tag, name, gan),
                    SR.render_shape(verts, topo, projected=p, size=size, images=bg, lights=lights.cuda(), gan_range=gan, want=SHAPE_ALL))
        for D in (1, 2, 3):
            put('%s.attr.d%d' % (tag, D), SR._render_attr('render_normal', p, draw('%s.values%d' % (tag, D), (B, V, D)).cuda(), topo, size, 0.0))
        put(tag + '.depth', SR.render_depth(p, topo, size))
        normals = SR.vertex_normals(verts, topo)
        for Su in (13, 32):
            sub = '%s.su%d' % (tag, Su)
            mask = (draw('mask%d' % Su, (Su, Su)) > -0.7).float()
            L = DT.UvLayout(faces, uv, faces, Su, mask, draw('fixed%d' % Su, (Su, Su), 0.0, 0.003), n_vertices=V)
            albedo, uvn, light, images = maps(sub, B, Su, size)
            put(sub + '.table', L.tables('cuda')[1:3])
            put(sub + '.detail', SR.render_shape(verts, topo, projected=p, size=size, images=bg, layout=L, detail_normals=uvn, want=DETAIL_ALL))
            put(sub + '.detail.gan', SR.render_shape(verts, topo, projected=p, size=size, gan_range=True, layout=L, detail_normals=uvn,
                                                    want=DETAIL_ALL))
            texture_cases(sub + '.texture', verts, topo, L, albedo, light, projected=p, size=size)
            put(sub + '.world2uv', DT.world2uv(L, verts))
            uv_z = draw(sub + '.uvz', (B, 1, Su, Su), 0.0, 0.01).cuda()
            dn = DT.detail_normals(L, uv_z, verts, normals, dense_vertices=True)
            put(sub + '.detail_normals', dn)
            put(sub + '.uv_textures', TX.uv_textures(L, albedo, dn[0], light, p, images, want=UV_ALL))
            put(sub + '.uv_textures.noalbedo', TX.uv_textures(L, None, dn[0], light, p, images, want=UV_ALL))

    # ---- the synthetic FLAME mesh
    B, size, Su = 2, 32, 32
    m = FL.FLAME()
    m.load_state_dict(S.synthetic_flame_state(11))
    c = S.synthetic_flame_coeffs(11, 'render_bits.flame', B, [0.3, -0.4])
    c['cam'][:, 0] = torch.tensor([2.5, 2.0])            # the soup over a fifth of the image, tens of faces under a pixel
    ffaces = m.faces_tensor.long()
    nf = ffaces.shape[0]
    f = torch.arange(nf, dtype=torch.float64)
    cell = torch.stack([f % 100, torch.div(f, 100, rounding_mode='floor')], 1) / 100.0
    corner = torch.tensor([[-0.41, -0.39], [1.73, -0.31], [-0.33, 1.69]], dtype=torch.float64) / 100.0
    L = DT.UvLayout(ffaces, (cell[:, None] + corner[None]).reshape(-1, 2), torch.arange(3 * nf).reshape(nf, 3), Su,
                    (draw('flame.mask', (Su, Su)) > -0.7).float(), draw('flame.fixed', (Su, Su), 0.0, 0.003), n_vertices=int(m.v_template.shape[0]))
    m = m.cuda()
    verts, _, _ = m(c['shape'].cuda(), c['exp'].cuda(), c['pose'].cuda())
    cam = c['cam'].cuda()
    topo = FL.topology(m)
    albedo, uvn, light, _ = maps('flame', B, Su, size)
    for tag, view in (('flame.cam', {'cam': cam}), ('flame.projected', {'projected': TX.orth_proj(verts, cam).contiguous()})):
        put(tag + '.shape', SR.render_shape(verts, topo, size=size, want=SHAPE_ALL, **view))
        put(tag + '.detail', SR.render_shape(verts, topo, size=size, layout=L, detail_normals=uvn, want=DETAIL_ALL, **view))
        texture_cases(tag + '.texture', verts, topo, L, albedo, light, size=size, **view)


def child(path):
    import numpy as np
    import torch
    out = {}

    def put(name, v):
        if torch.is_tensor(v):
            assert name not in out, name
            out[name] = v.detach().cpu().contiguous().numpy()
        else:
            for k, x in (v.items() if isinstance(v, dict) else enumerate(v)):
                put('%s.%s' % (name, k), x)

    with torch.no_grad():
        run_cases(put)
    torch.cuda.synchronize()
    from stylegan_directions_face_reenactment_amd import _native as N
    np.savez(path, __library__=np.array(os.path.abspath(N.LIB_PATH)), **out)
    print('%d tensors from %s' % (len(out), N.LIB_PATH), flush=True)


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    if '--child' in sys.argv:
        return child(arg('--child', None))
    import numpy as np
    ref = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith('--') else os.path.join(ROOT, 'build', 'libsgdfr_hip_parent.so')
    assert os.path.exists(ref), ref + ' (python scripts/build_ref.py <commit> builds one)'
    base = tempfile.mkdtemp()
    files = {}
    for tag, lib in (('ref', os.path.abspath(ref)), ('new', None)):
        files[tag] = os.path.join(base, tag + '.npz')
        env = dict(os.environ)
        env.pop('SGDFR_LIB', None)
        if lib:
            env.update(SGDFR_LIB=lib, SGDFR_ALLOW_LIB_OVERRIDE='1')
        try:
            status = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', files[tag]], env=env, timeout=240).returncode
        except subprocess.TimeoutExpired:
            status = 'none within 240 s'
        if status != 0:
            print('%s: the child ended with status %s; nothing more is started' % (tag, status))
            return 2
    p, q = np.load(files['ref']), np.load(files['new'])
    libs = [os.path.relpath(str(d['__library__']), ROOT) for d in (p, q)]
    assert libs[0] != libs[1], libs                      # each child says which library it loaded
    lines = ['render_bits: %s against %s, seed %d' % (libs[0], libs[1], SEED)]
    different = sorted(set(p.files) ^ set(q.files))
    for n in sorted((set(p.files) & set(q.files)) - {'__library__'}):
        a, b = p[n], q[n]
        same = a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        lines.append('%-9s %-62s %-8s %-12s %d of %d values are not 0 or -1' % ('equal' if same else 'DIFFERENT', n, a.dtype, 'x'.join(map(str, a.shape)),
                                                                                 int(np.count_nonzero((a != 0) & (a != -1))), a.size))
        if not same:
            different.append(n)
    lines.append('%d tensors, %d values: %s' % (len(p.files) - 1, sum(int(p[n].size) for n in p.files) - 1,
                                               'all equal' if not different else '%d DIFFERENT or missing: %s' % (len(different), different)))
    print('\n'.join(lines))
    out = arg('--out', None)
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 1 if different else 0


if __name__ == '__main__':
    sys.exit(main())
