"""tests/golden/kat20_sweeps.npz from the REAL reference's get_direction_info (libs/configs/config_directions.py:42-85) chained with the
two np.arange loops and one_hot exactly as libs/utilities/visualization.py:46-60 and run_facial_editing.py:172-189 chain them, on CPU
tensors.

Run:  python scripts/make_golden_sweep.py [--check]     (needs the reference checkout; CPU only, seconds)

The functions are imported through the helpers of oracle/make_golden_shift.py (placeholder modules for the packages the image lacks).
Settings: voxceleb D=15 sc=6 (int), ffhq D=12 sc=6.0, voxceleb D=15 sc=4.5, each with shifts_count 10 and 4, every direction 0..D-1 of
every source row.  Source rows: 8 from synthetic.synthetic_shape_params, then
  row 8    angles (0, 0, 0): start exactly 0, ladders of shifts_count + (shifts_count + 1) rows, the `+1e-5` endpoint included
  row 9    angles (30, 15, 15): start = 0.75 sc > sc/2 on every angle direction (empty `hi`)
  row 10   angles (-30, -15, -15): start < -sc/2 (empty `lo`)
  row 11   jaw and every expression coefficient a quarter of their range above its maximum: start beyond +sc (empty `hi`)
  row 12   (only if the search finds one) the first of 4096 further synthetic rows on which a jaw / expression direction puts
           (stop - first) / step within one float32 ulp of an integer; `<tag>.near_integer` records (found, pool row, direction, which
           ladder) per shifts_count -- the row is looked for with shifts_count 10 and then 4 and injected for both
Stored per setting: the inputs (ang, pose, exp), the direction kinds and names; per shifts_count the records start / min / max (as
float64: exact for the float32 values the reference gives on jaw and expression directions), step, the dtype names the reference
returned, n_lo / n_hi (the two arange lengths, int32), and `rows` [R, D] float32: the one_hot vectors in the order source row, direction,
`lo` ascending, `hi` ascending.  `versions` holds the NumPy and torch versions: the float32 arithmetic of the jaw / expression ladders
is NumPy >= 2 behaviour (weak Python scalars).  The script asserts that every kind (angle, jaw, exp), an empty `lo`, an empty `hi` and
ladders with both parts occur in every setting.  --check compares every array with the committed file bit for bit instead of writing.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import make_golden as MG                                   # noqa: E402
from oracle import make_golden_shift as MS                             # noqa: E402
from stylegan_directions_face_reenactment_amd import synthetic as S   # noqa: E402

SEED = MG.SEED
OUT = os.path.join(MG.OUT, 'kat20_sweeps.npz')
BASE_ROWS = 8
SEARCH_ROWS = 4096
SHIFTS_COUNTS = (10, 4)
SETTINGS = (('voxceleb', 15, 6, 'ranges_voxceleb.npy'), ('ffhq', 12, 6.0, 'ranges_FFHQ.npy'), ('voxceleb', 15, 4.5, 'ranges_voxceleb.npy'))
KIND = {'yaw': 1, 'pitch': 1, 'roll': 1, 'jaw': 2}                      # SGDFR_DIR_ANGLE / JAW; 'exp_%02d' -> 3 (SGDFR_DIR_EXP)


def tag_of(dataset, D, sc):
    return '%s_%d_%s' % (dataset, D, str(sc).replace('.', 'p'))


def ladder(GDI, one_hot, cfg, k, shifts_count, ang, pose, exp, n, D):
    """(type, start, min, max, step, lo rows, hi rows) of source row n along direction k, the reference's chain."""
    count_pose, directions_exp, jaw, angle_scales, angle_dirs, sc = cfg
    params = {'pose': pose[n:n + 1], 'alpha_exp': exp[n:n + 1]}
    typ, start, mn, mx, step = GDI(k, angle_dirs, jaw['a'], jaw['b'], directions_exp, sc, angle_scales, count_pose, shifts_count,
                                   params, ang[n:n + 1])
    min_shift = (-sc - start)                                           # visualization.py:50-51 (the same expressions again)
    max_shift = (sc - start) + 1e-5
    assert min_shift == mn and max_shift == mx and type(min_shift) is type(mn)
    lo = [one_hot(D, shift, k) for shift in np.arange(min_shift, start, step)]
    hi = [one_hot(D, shift, k) for shift in np.arange(start, max_shift, step)]
    return typ, start, mn, mx, step, lo, hi


def near_integer(cfg, pose, exp, shifts_count):
    """First (row, direction, part) of the pool whose float32 length quotient is within one ulp of an integer (jaw / expressions)."""
    count_pose, directions_exp, jaw, angle_scales, angle_dirs, sc = cfg
    step = np.float32(sc / shifts_count)
    lines = [(count_pose - 1, jaw['a'], jaw['b'], pose[:, 3])] + [(d['A_direction'], d['a'], d['b'], exp[:, d['exp_component']])
                                                                  for d in directions_exp]
    best = None
    for k, a, b, x in lines:
        start = (a * x + b).numpy()                                    # float32 tensor arithmetic, as get_direction_info
        mn, mx = np.float32(-sc) - start, (np.float32(sc) - start) + np.float32(1e-5)
        for part, q in ((0, (start - mn) / step), (1, (mx - start) / step)):
            hit = np.nonzero((q > 0) & (np.abs(q - np.rint(q)) <= np.spacing(np.rint(q).astype(np.float32))))[0]
            if hit.size and (best is None or hit[0] < best[0]):
                best = (int(hit[0]), int(k), part)
    return best


def main():
    check = '--check' in sys.argv                                       # (the import helper below cuts sys.argv for the reference's parsers)
    RI, UT, G = MS.import_reference_shift()
    from libs.configs.config_directions import get_direction_info as GDI
    from libs.utilities.utils import one_hot
    import libs.configs.config_directions as CD
    assert os.path.realpath(CD.__file__).startswith(os.path.realpath(MG.REF))
    torch.Tensor.cuda = lambda self, *a, **k: self                     # GPU-less host: keep everything on the CPU
    out = {'seed': np.int64(SEED), 'versions': np.array(['numpy ' + np.__version__, 'torch ' + torch.__version__])}
    cwd = os.getcwd()
    for dataset, D, sc, ranges_file in SETTINGS:
        tag = tag_of(dataset, D, sc)
        os.chdir(MG.REF)                                                # the ranges path is relative in the reference
        count_pose, num_exp, directions_exp, jaw, angle_scales, angle_dirs = G.initialize_directions(dataset, D, sc)
        os.chdir(cwd)
        cfg = (count_pose, directions_exp, jaw, angle_scales, angle_dirs, sc)
        ang, par = S.synthetic_shape_params(SEED, tag + '.sweep.src', BASE_ROWS)
        pose, exp = par['pose'], par['alpha_exp']
        extra_ang = torch.tensor([[0.0, 0.0, 0.0], [30.0, 15.0, 15.0], [-30.0, -15.0, -15.0], [5.0, -3.0, 2.0]])
        extra_pose, extra_exp = pose[:4].clone(), exp[:4].clone()
        extra_pose[3, 3] = float(jaw['max'] + 0.25 * (jaw['max'] - jaw['min']))
        for d in directions_exp:
            extra_exp[3, d['exp_component']] = float(d['max_shift'] + 0.25 * (d['max_shift'] - d['min_shift']))
        ang, pose, exp = torch.cat([ang, extra_ang]), torch.cat([pose, extra_pose]), torch.cat([exp, extra_exp])
        pool_ang, pool = S.synthetic_shape_params(SEED, tag + '.sweep.pool', SEARCH_ROWS)
        found = np.zeros((len(SHIFTS_COUNTS), 4), dtype=np.int64)       # (found, pool row, direction, part) per shifts_count
        hit = None
        for i, c in enumerate(SHIFTS_COUNTS):
            h = near_integer(cfg, pool['pose'], pool['alpha_exp'], c)
            if h is not None:
                found[i] = (1,) + h
                hit = hit if hit is not None else h
        if hit is not None:
            r = hit[0]
            ang, pose, exp = torch.cat([ang, pool_ang[r:r + 1]]), torch.cat([pose, pool['pose'][r:r + 1]]), torch.cat([exp, pool['alpha_exp'][r:r + 1]])
        N = ang.shape[0]
        out[tag + '.ang'], out[tag + '.pose'], out[tag + '.exp'] = MG.npy(ang), MG.npy(pose), MG.npy(exp)
        out[tag + '.near_integer'] = found
        for c in SHIFTS_COUNTS:
            key = '%s.c%d' % (tag, c)
            rec = {f: np.zeros((N, D), dtype=np.float64) for f in ('start', 'min', 'max')}
            n_lo, n_hi = np.zeros((N, D), dtype=np.int32), np.zeros((N, D), dtype=np.int32)
            rows, types, dtypes, steps = [], [], [], set()
            for n in range(N):
                for k in range(D):
                    typ, start, mn, mx, step, lo, hi = ladder(GDI, one_hot, cfg, k, c, ang, pose, exp, n, D)
                    rec['start'][n, k], rec['min'][n, k], rec['max'][n, k] = float(start), float(mn), float(mx)
                    assert np.asarray(start).dtype == np.asarray(mn).dtype == np.asarray(mx).dtype
                    n_lo[n, k], n_hi[n, k] = len(lo), len(hi)
                    rows += lo + hi
                    steps.add(step)
                    if n == 0:
                        types.append(typ)
                        dtypes.append(str(np.asarray(start).dtype))
                    else:
                        assert types[k] == typ and dtypes[k] == str(np.asarray(start).dtype)
            assert len(steps) == 1 and all(r.dtype == torch.float32 and tuple(r.shape) == (D,) for r in rows)
            kinds = np.array([KIND.get(t_, 3) for t_ in types], dtype=np.int32)
            # coverage: every kind, an empty lo, an empty hi, ladders with both parts; the zero-angle row's full ladders
            assert set(kinds.tolist()) == {1, 2, 3}
            assert (n_lo == 0).any() and (n_hi == 0).any() and ((n_lo > 0) & (n_hi > 0)).any()
            ang_k = np.nonzero(kinds == 1)[0]
            assert (rec['start'][BASE_ROWS, ang_k] == 0).all() and (n_lo[BASE_ROWS, ang_k] == c).all() and (n_hi[BASE_ROWS, ang_k] == c + 1).all()
            assert (n_hi[BASE_ROWS + 1, ang_k] == 0).all() and (n_lo[BASE_ROWS + 2, ang_k] == 0).all()
            assert (n_hi[BASE_ROWS + 3, kinds != 1] == 0).all() and (rec['start'][BASE_ROWS + 3, kinds != 1] > sc).all()
            out[key + '.start'], out[key + '.min'], out[key + '.max'] = rec['start'], rec['min'], rec['max']
            out[key + '.step'] = np.float64(steps.pop())
            out[key + '.n_lo'], out[key + '.n_hi'] = n_lo, n_hi
            out[key + '.start_dtype'] = np.array(dtypes)
            out[key + '.rows'] = torch.stack(rows).numpy()
            out[tag + '.types'], out[tag + '.kinds'] = np.array(types), kinds
            print('%-22s N=%d K=%d rows %d  lengths lo %d..%d hi %d..%d  near-integer row: %s' % (
                key, N, D, len(rows), n_lo.min(), n_lo.max(), n_hi.min(), n_hi.max(), found.tolist()))
    if check:
        old = np.load(OUT, allow_pickle=False)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for k, v in out.items():
            v = np.asarray(v)
            if k == 'versions':
                print('committed with %s, now %s' % (list(old[k]), list(v)))
                continue
            assert old[k].dtype == v.dtype and old[k].shape == v.shape and old[k].tobytes() == v.tobytes(), k
        print('%s: all %d arrays bit-identical' % (os.path.basename(OUT), len(out) - 1))
        return
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d arrays, %d bytes)' % (os.path.basename(OUT), len(out), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
