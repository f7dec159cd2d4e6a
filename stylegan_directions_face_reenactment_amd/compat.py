"""Mount this package at the reference's import paths so its scripts run unchanged:

    import stylegan_directions_face_reenactment_amd.compat as compat; compat.install()
    from libs.gan.StyleGAN2.model import Generator          # -> the MI355X generator
    from libs.models.direction_matrix import DirectionMatrix

Only the modules of the hot path are aliased; everything else under ``libs`` keeps
resolving to the reference checkout on sys.path.  ``install_lpips(state_dict)`` (opt-in) additionally mounts the HIP LPIPS at
``libs.criteria.lpips.lpips`` so that unchanged ``LPIPS(net_type='alex')`` calls get it with those weights (no torchvision, no
download); ``install_id_loss(path)`` (opt-in) mounts the HIP identity loss at ``libs.criteria.id_loss`` the same way.
``install_face_detector(state_dict)`` (opt-in) mounts the HIP S3FD detector at ``libs.face_models.sfd.sfd_detector`` so that an
unchanged ``SFDDetector(device, path)`` (landmarks_estimation.py:118) gets it.  ``install_face_crop()`` (opt-in) mounts the HIP
alignment crop at ``libs.face_models.ffhq_cropping`` (numpy in, numpy out, as preprocess_image calls it).  There is no ``install_landmarks``:
``LandmarksEstimation`` crops and runs one face at a time around the FAN network; call ``face_detector.detect_landmarks`` or
``landmarks.get_landmarks`` instead.  ``install_visualization()`` (opt-in) mounts the batched direction sweep's ``make_interpolation_chart`` at
``libs.utilities.visualization``.  ``libs.utilities.generic`` is NOT replaced wholesale
(it also holds DECA glue); call ``patch_generic(module)`` to swap in the two fused functions.
"""
import importlib
import os
import sys
import types

ALIASES = {
    'libs.gan.StyleGAN2.model': 'stylegan_directions_face_reenactment_amd.model',
    'libs.gan.StyleGAN2.op': 'stylegan_directions_face_reenactment_amd.op',
    'libs.gan.StyleGAN2.op.fused_act': 'stylegan_directions_face_reenactment_amd.op.fused_act',
    'libs.gan.StyleGAN2.op.upfirdn2d': 'stylegan_directions_face_reenactment_amd.op.upfirdn2d',
    'libs.models.direction_matrix': 'stylegan_directions_face_reenactment_amd.direction_matrix',
}


def install():
    for alias, target in ALIASES.items():
        sys.modules[alias] = importlib.import_module(target)
    return sorted(ALIASES)


def patch_generic(generic_module):
    from . import generic
    generic_module.get_shifted_latent_code = generic.get_shifted_latent_code
    generic_module.generate_image = generic.generate_image
    return generic_module


LPIPS_ALIAS = 'libs.criteria.lpips.lpips'


def install_lpips(state_dict):
    """Mount a module at libs.criteria.lpips.lpips whose LPIPS(net_type='alex', version='0.1') is the HIP LPIPS with
    `state_dict` loaded (any format lpips.LPIPS.load_state_dict accepts, complete) and moved to the GPU, as the reference's
    constructor does (lpips.py:21-26).  Parent packages that cannot be imported are created empty."""
    from . import lpips as hip_lpips
    sd = dict(state_dict)
    hip_lpips.LPIPS().load_state_dict(sd)           # fail here, not at the first LPIPS() of the caller
    _parent_packages(LPIPS_ALIAS)

    class LPIPS(hip_lpips.LPIPS):
        def __init__(self, net_type: str = 'alex', version: str = '0.1'):
            super().__init__(net_type, version)
            self.load_state_dict(sd)
            self.to('cuda')

    mod = types.ModuleType(LPIPS_ALIAS)
    mod.LPIPS = LPIPS
    mod.__doc__ = 'HIP LPIPS mounted by stylegan_directions_face_reenactment_amd.compat.install_lpips'
    _mount(LPIPS_ALIAS, mod)
    return LPIPS_ALIAS


def _parent_packages(alias):
    """Import the parent packages of `alias`; those that cannot be imported are created empty."""
    parts = alias.split('.')
    for i in range(1, len(parts)):
        name = '.'.join(parts[:i])
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                pkg = types.ModuleType(name)
                pkg.__path__ = []
                sys.modules[name] = pkg


def _mount(alias, mod):
    parent, _, leaf = alias.rpartition('.')
    sys.modules[alias] = mod
    setattr(sys.modules[parent], leaf, mod)


ID_LOSS_ALIAS = 'libs.criteria.id_loss'
ID_LOSS_DEFAULT_PATH = './pretrained_models/model_ir_se50.pth'     # id_loss.py:8


def install_id_loss(pretrained_model_path=None):
    """Mount a module at libs.criteria.id_loss whose IDLoss(pretrained_model_path) is the HIP IDLoss: an unchanged
    `id_loss.IDLoss().cuda().eval()` (utils_train.py:53) loads `pretrained_model_path` (default: the reference's
    ./pretrained_models/model_ir_se50.pth) itself, and a missing file prints and exits as id_loss.py:12-14 does.  Parent
    packages that cannot be imported are created empty."""
    from . import id_loss as hip_id_loss
    default = pretrained_model_path or ID_LOSS_DEFAULT_PATH
    _parent_packages(ID_LOSS_ALIAS)

    class IDLoss(hip_id_loss.IDLoss):
        def __init__(self, pretrained_model_path=default):
            print('Loading ResNet ArcFace for identity loss')
            if not os.path.exists(pretrained_model_path):
                print('ir_se50 model does not exist in {}'.format(pretrained_model_path))
                sys.exit()
            super().__init__(pretrained_model_path)

    mod = types.ModuleType(ID_LOSS_ALIAS)
    mod.IDLoss = IDLoss
    mod.Backbone = hip_id_loss.Backbone
    mod.__doc__ = 'HIP identity loss mounted by stylegan_directions_face_reenactment_amd.compat.install_id_loss'
    _mount(ID_LOSS_ALIAS, mod)
    return ID_LOSS_ALIAS


FACE_DETECTOR_ALIAS = 'libs.face_models.sfd.sfd_detector'


def install_face_detector(state_dict=None):
    """Mount a module at libs.face_models.sfd.sfd_detector whose SFDDetector(device, path_to_detector) is the HIP S3FD detector:
    an unchanged `SFDDetector(device, path)` loads `path` with torch.load as sfd_detector.py:24 does (or takes `state_dict` when one is
    given here and no path), moves the network to the GPU and answers detect_from_batch(tensor) with the reference's lists (which
    synchronises, as the reference does).  reference_scale / reference_x_shift / reference_y_shift are the reference's 195 / 0 / 0.
    Parent packages that cannot be imported are created empty."""
    import torch
    from . import face_detector as hip_fd
    sd0 = None if state_dict is None else dict(state_dict)
    if sd0 is not None:
        hip_fd.S3FD().load_state_dict(sd0)           # fail here, not at the first SFDDetector() of the caller
    _parent_packages(FACE_DETECTOR_ALIAS)

    class SFDDetector(object):
        def __init__(self, device, path_to_detector=None, verbose=False):
            self.device, self.verbose = device, verbose
            if path_to_detector is None and sd0 is None:
                raise ValueError('SFDDetector: no path_to_detector and no state dict given to install_face_detector')
            self.face_detector = hip_fd.S3FD()
            self.face_detector.load_state_dict(torch.load(path_to_detector) if path_to_detector is not None else sd0)
            self.face_detector.to('cuda')

        def detect_from_batch(self, tensor):
            return hip_fd.detect_from_batch(self.face_detector, tensor.float())

        reference_scale = property(lambda self: 195)
        reference_x_shift = property(lambda self: 0)
        reference_y_shift = property(lambda self: 0)

    mod = types.ModuleType(FACE_DETECTOR_ALIAS)
    mod.SFDDetector = SFDDetector
    mod.s3fd = hip_fd.S3FD
    mod.__doc__ = 'HIP S3FD face detector mounted by stylegan_directions_face_reenactment_amd.compat.install_face_detector'
    _mount(FACE_DETECTOR_ALIAS, mod)
    return FACE_DETECTOR_ALIAS


FACE_CROP_ALIAS = 'libs.face_models.ffhq_cropping'


def install_face_crop():
    """Mount a module at libs.face_models.ffhq_cropping whose crop_using_landmarks(image, landmarks) is the HIP alignment crop with
    the reference's signature: a [H,W,3] uint8 array and [68,2] landmarks in, the [256,256,3] uint8 crop out, None where the
    reference returns None (an empty box) and where the row is not valid (face_crop: a box beyond max(H, W) // 2 or a border wider
    than the frame).  It copies to the GPU and back per call; a pipeline that stays on the device calls
    reenact.preprocess_frames instead.  Parent packages that cannot be imported are created empty."""
    from . import face_crop as hip_fc
    _parent_packages(FACE_CROP_ALIAS)
    mod = types.ModuleType(FACE_CROP_ALIAS)
    mod.crop_using_landmarks = lambda image, landmarks: hip_fc.crop_image(image, landmarks)
    mod.__doc__ = 'HIP alignment crop mounted by stylegan_directions_face_reenactment_amd.compat.install_face_crop'
    _mount(FACE_CROP_ALIAS, mod)
    return FACE_CROP_ALIAS


VISUALIZATION_ALIAS = 'libs.utilities.visualization'
_visualization_saved = []


def install_visualization():
    """Mount a module at libs.utilities.visualization whose make_interpolation_chart is the batched sweep (sweep.py) with the
    reference's signature and return value, and whose get_shifted_image is the reference's single frame -- so an unchanged
    `from libs.utilities.visualization import make_interpolation_chart` (utils_train.py:653-691 log_interpolation) gets it.  Opt-in:
    install() does not call it.  uninstall_visualization() puts back whatever was mounted there before.  Parent packages that cannot
    be imported are created empty."""
    from . import generic, sweep
    parts = VISUALIZATION_ALIAS.split('.')
    before = set(sys.modules)
    _parent_packages(VISUALIZATION_ALIAS)
    created = [n for n in ('.'.join(parts[:i]) for i in range(1, len(parts))) if n not in before]
    parent, _, leaf = VISUALIZATION_ALIAS.rpartition('.')
    _visualization_saved.append((sys.modules.get(VISUALIZATION_ALIAS), getattr(sys.modules[parent], leaf, None), created))

    def get_shifted_image(G, A_matrix, source_code, shift, direction_index, truncation, trunc, w_plus, input_is_latent, num_layers_shift):
        import torch
        shift_vector = torch.zeros(A_matrix.input_dim)
        shift_vector[direction_index] = shift                            # utils.py:62-65 one_hot
        return generic.generate_image(G, source_code, truncation, trunc, w_plus, shift_code=A_matrix(shift_vector.cuda()),
                                      input_is_latent=input_is_latent, num_layers_shift=num_layers_shift)

    mod = types.ModuleType(VISUALIZATION_ALIAS)
    mod.make_interpolation_chart = sweep.make_interpolation_chart
    mod.get_shifted_image = get_shifted_image
    mod.__doc__ = 'HIP direction sweeps mounted by stylegan_directions_face_reenactment_amd.compat.install_visualization'
    _mount(VISUALIZATION_ALIAS, mod)
    return VISUALIZATION_ALIAS


def uninstall_visualization():
    """Undo the last install_visualization(): the module and the parent's attribute as they were before it (absent if they were),
    and the parent packages it had to create."""
    if not _visualization_saved:
        return False
    old_mod, old_attr, created = _visualization_saved.pop()
    parent, _, leaf = VISUALIZATION_ALIAS.rpartition('.')
    if old_mod is None:
        sys.modules.pop(VISUALIZATION_ALIAS, None)
    else:
        sys.modules[VISUALIZATION_ALIAS] = old_mod
    if parent in sys.modules:
        if old_attr is None:
            if hasattr(sys.modules[parent], leaf):
                delattr(sys.modules[parent], leaf)
        else:
            setattr(sys.modules[parent], leaf, old_attr)
    for name in created:
        sys.modules.pop(name, None)
    return True
