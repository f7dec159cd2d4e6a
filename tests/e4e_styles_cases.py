"""The fixture cases of the e4e encoder with the head count apart from the input side (tests/golden/kat24_e4e_styles.npz,
scripts/make_golden_e4e_styles.py): Encoder4Editing(50, 'ir_se', image_resolution) of the reference counts its heads from
image_resolution (16 at 512, 18 at 1024) and reads a smaller input, as the 512 and 1024 generators' encoders read the 256 x 256 crop.
Images and weights are regenerated from seeds, as in tests/e4e_restatement.py, whose `forward` counts the heads from the state's
keys and so restates these encoders as it stands.  HEAD_CASES are further encoders of that kind without a fixture, for the plan
sweep over head counts (tests/test_gpu_e4e_head_plans.py)."""
from collections import OrderedDict

import e4e_restatement as R

KAT = 'kat24_e4e_styles.npz'
# name -> (rows, input side, image_resolution, state seed, counter key of the images)
#   d: 18 heads, 11 of them fine: 88 R^2 floats per row of parked head maps against the 64 R^2 unit buffer; head convs on 1 x 1 maps
#   e: 16 heads, 9 fine: 72 R^2, the first count past the buffer; 5 / 10 / 20 maps, pixel counts off the 64-pixel tile
#   f: the real shape, 18 heads on the 256 x 256 crop: fixture only
CASES = OrderedDict([('d', (2, 32, 1024, R.SEED + 1024, 'e4e.styles.x32')), ('e', (3, 80, 512, R.SEED + 512, 'e4e.styles.x80')),
                     ('f', (1, 256, 1024, R.SEED + 2048, 'e4e.styles.x256'))])
# the head-count cases of tests/test_gpu_e4e_head_plans.py (plan_rules.E4E_HEADS_SMALL says what each adds): in no fixture, seeded
# as d and e are and kept apart from the fixture's list; their yardstick is the fp32 restatement's own deviation from the fp64 one
HEAD_CASES = OrderedDict([('h32n16', (2, 32, 512, R.SEED + 3216, 'e4e.heads.x32n16')), ('h48n18', (3, 48, 1024, R.SEED + 4818, 'e4e.heads.x48n18')),
                          ('h64n16', (3, 64, 512, R.SEED + 6416, 'e4e.heads.x64n16')), ('h64n14', (2, 64, 256, R.SEED + 6414, 'e4e.heads.x64n14')),
                          ('h96n18', (2, 96, 1024, R.SEED + 9618, 'e4e.heads.x96n18')), ('h128n8', (2, 128, 32, R.SEED + 12808, 'e4e.heads.x128n8'))])


def case(name):
    return CASES[name] if name in CASES else HEAD_CASES[name]


def heads(name):
    res = case(name)[2]
    return 2 * (res.bit_length() - 1) - 2


def by_side_and_heads():
    """(input side, head count) -> case name."""
    return OrderedDict(((case(name)[1], heads(name)), name) for name in list(CASES) + list(HEAD_CASES))


def fixture_inputs(S, name):
    """Images [B,3,R,R] float32 in [-1,1] of a case, regenerated from its counter key."""
    B, side, _, _, key = case(name)
    return S.counter_tensor(R.SEED, key, (B, 3, side, side), 0.0, 0.5).clamp_(-1, 1)


def fixture_state(S, name, template):
    """The seeded state of a case; `template` is a state dict with the module's keys and shapes at that image_resolution."""
    return S.synthetic_encoder_state(template, seed=case(name)[3])


_ENCODERS = {}


def build_encoder(S, name):
    """(module, state) of a case, built anew: 18 heads are 280 M values, a caller that keeps the device copy alone holds no other."""
    from stylegan_directions_face_reenactment_amd.encoder import Encoder4Editing
    _, side, res, _, _ = case(name)
    enc = Encoder4Editing(50, 'ir_se', res, input_size=side).eval()
    state = fixture_state(S, name, enc.state_dict())
    enc.load_state_dict(state, strict=True)
    return enc, state


def make_encoder(S, name):
    """(module, state) of a case, built once per process."""
    if name not in _ENCODERS:
        _ENCODERS[name] = build_encoder(S, name)
    return _ENCODERS[name]
