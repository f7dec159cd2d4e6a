"""Mount this package at the reference's import paths so its scripts run unchanged:

    import stylegan_directions_face_reenactment_amd.compat as compat; compat.install()
    from libs.gan.StyleGAN2.model import Generator          # -> the MI355X generator
    from libs.models.direction_matrix import DirectionMatrix

Only the modules of the hot path are aliased; everything else under ``libs`` keeps
resolving to the reference checkout on sys.path.  ``install_lpips(state_dict)`` (opt-in) additionally mounts the HIP LPIPS at
``libs.criteria.lpips.lpips`` so that unchanged ``LPIPS(net_type='alex')`` calls get it with those weights (no torchvision, no
download).  ``libs.utilities.generic`` is NOT replaced wholesale
(it also holds DECA glue); call ``patch_generic(module)`` to swap in the two fused functions.
"""
import importlib
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
    parts = LPIPS_ALIAS.split('.')
    for i in range(1, len(parts)):
        name = '.'.join(parts[:i])
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                pkg = types.ModuleType(name)
                pkg.__path__ = []
                sys.modules[name] = pkg

    class LPIPS(hip_lpips.LPIPS):
        def __init__(self, net_type: str = 'alex', version: str = '0.1'):
            super().__init__(net_type, version)
            self.load_state_dict(sd)
            self.to('cuda')

    mod = types.ModuleType(LPIPS_ALIAS)
    mod.LPIPS = LPIPS
    mod.__doc__ = 'HIP LPIPS mounted by stylegan_directions_face_reenactment_amd.compat.install_lpips'
    sys.modules[LPIPS_ALIAS] = mod
    setattr(sys.modules['.'.join(parts[:-1])], parts[-1], mod)
    return LPIPS_ALIAS
