"""The device weight pack of a network head, kept once: LPIPS, the id-loss Backbone, FLAME, DECA's ResnetEncoder, FAN, S3FD and
Encoder4Editing hold their weights as an nn.Module and run on one flat float32 pack that a `sgdfr_*_prepack_f32` launch builds
from the folded weights.  `PackedWeights` owns that pack's lifetime ("The pack cache"); a head declares what differs:

    class FAN(PackedWeights, nn.Module):                   # PackedWeights first: its hooks wrap nn.Module's
        PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_fan_prepack_f32', 'sgdfr_fan_pack_elems', N.FAN_PARAMS
        TRAIN_ERROR = '...'                                # check(): the words for train mode; None = train mode is not tested
        GRAD_ERROR = '...'                                 # check(): the words for a trainable parameter; None = not tested
        def folded(self): ...                              # the tensors the prepack takes, None where it takes NULL
"""
import ctypes
from collections import OrderedDict

import torch

from . import _native as N


class PackedWeights:
    PREPACK = PACK_ELEMS = PARAMS = None
    TRAIN_ERROR = GRAD_ERROR = None
    PACK_DTYPE = torch.float32      # what every folded tensor must be; None: any dtype, on the GPU
    WRAP_STATE_DICT = True          # load_state_dict() rewraps the dict, which drops `_metadata` (BatchNorm then loads as version None)
    _pack = None                    # (key, pack, folded tensors)

    def _key(self):
        return tuple((t.data_ptr(), t._version, t.device) for t in self.state_dict(keep_vars=True).values())

    def invalidate_packs(self):
        """Drop the weight pack (needed only after in-place writes through `.data`, which bump no version counter)."""
        self._pack = None

    def _prepack_plan(self, ps):
        """(pointers the prepack takes, arguments of the pack_elems query, integers between the pointer array and the pack)."""
        return self.PARAMS, (), ()

    def packed(self):
        """The device weight pack, rebuilt when any state-dict entry's storage, version or device changes."""
        key = self._key()
        if self._pack is None or self._pack[0] != key:
            ps = self.folded()
            for p in ps:
                if p is not None:
                    N.require_device(p, dtype=self.PACK_DTYPE or p.dtype)
            count, elems_args, extra = self._prepack_plan(ps)
            pack = torch.empty(getattr(N.load(), self.PACK_ELEMS)(*elems_args), dtype=torch.float32, device=ps[0].device)
            arr = (ctypes.c_void_p * count)(*[None if p is None else p.data_ptr() for p in ps])
            N.call(self.PREPACK, arr, *extra, N.ptr(pack), N.stream())
            self._pack = (key, pack, ps)          # the folded tensors stay alive until the stream has read them
        return self._pack[1]

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_packs()
        return out

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        res = super().load_state_dict(OrderedDict(state_dict) if self.WRAP_STATE_DICT else state_dict, strict=strict, **kwargs)
        self.invalidate_packs()
        return res

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_pack'] = None           # rebuilt on demand: never copied, never pickled
        return state

    def check(self):
        if self.TRAIN_ERROR is not None and self.training:
            raise RuntimeError(self.TRAIN_ERROR)
        if self.GRAD_ERROR is not None and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError(self.GRAD_ERROR)


class views:
    """Cuts a flat buffer into consecutive [rows, *shape] views: cut = views(buffer, rows, align=1); cut(shape) returns the next view
    and moves on, rounding the offset up to `align` elements; cut.done() asserts that the buffer is used up."""

    def __init__(self, buffer, rows, align=1):
        self.buffer, self.rows, self.align, self.o = buffer, rows, align, 0

    def __call__(self, shape):
        n = self.rows
        for d in shape:
            n *= d
        v = self.buffer[self.o:self.o + n].view(self.rows, *shape)
        self.o = (self.o + n + self.align - 1) // self.align * self.align
        return v

    def done(self):
        assert self.o == self.buffer.numel(), (self.o, self.buffer.numel())
