"""One base for the `nn.Module`s whose parameters are mirrored into a handle of libcwm_hip.so (include/cwm_hip.h): the plain VMAE predictor
(`cwm_model_*`), the conjoined predictors (`cwm_conj_*`) and RAFT (`cwm_raft_*`).  `LibraryModule` owns the handle's life, the weight
upload with its change detector and the per-handle options; a model class states its entry points (`_ABI`) and fills its config struct
(`_create`).  `_NoForward` is the parameter container their module trees are made of.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib


class _NoForward(nn.Module):
    """One node of a reference module tree: holds parameters (the state-dict layout of the published checkpoints), never computes."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("%s is a parameter container: the computation runs inside libcwm_hip.so via the forward of the model that owns it"
                           % type(self).__name__)


class LibraryModule(nn.Module):
    """A module that holds no compute: its parameters are uploaded into a library handle and its forward is one call into the C ABI.

    A subclass sets `_ABI` (role -> exported symbol: "destroy", "load_weight", "forward" and, where the model kind has them, "set_option",
    "set_lanes", "timing_enable", "timing_collect"; the functions are bound once, when the handle is created: `self._fn`) and overrides
    `_create(lib, handle_out)`.  A role that `_ABI` does not list raises a RuntimeError naming the model class.

    The change detector: a cheap "has any parameter changed since the last upload?" test.  Walking `state_dict()` costs ~0.3 ms per forward
    for ViT-B (218 tensors) -- GPU idle time whenever the caller synchronises between forwards -- so the tensors are listed once, each with
    the module dict that owns it, and a forward only checks (a) that every slot still holds the listed object (`setattr` /
    `register_parameter` replacing a Parameter, also through a SUBMODULE's `.to()` when torch swaps parameter objects) and (b) the (storage
    pointer, version counter) pairs (`p.data = ...`, `encoder.double()`, `copy_`, optimiser steps, `load_state_dict`): ~60 us.  Not visible
    to it: in-place edits through `.data` that keep the storage (`p.data.mul_(2)`): call `sync_weights(force=True)` after those."""

    _ABI: Dict[str, str] = {}
    _cwm = None  # the library chosen by `use_library` (None: the production one)

    def __init__(self):
        super().__init__()
        self._handle: Optional[int] = None
        self._handle_device: Optional[torch.device] = None
        self._loaded: Dict[str, Tuple[int, int]] = {}
        self._fn: Dict[str, object] = {}
        self._plist = None
        self._psig = None
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module._forget_params())

    # ---- change detector -------------------------------------------------------------------------
    def _forget_params(self):
        self._plist = None

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._plist = None
        return out

    def _param_device(self):
        return self._plist[0][2].device if self._plist else next(self.parameters()).device

    def _params_unchanged(self) -> bool:
        pl = self._plist
        if pl is None:
            return False
        for slots, key, p in pl:
            if slots.get(key) is not p:
                return False
        return tuple((p.data_ptr(), p._version) for _, _, p in pl) == self._psig

    def _remember_params(self):
        pl = []
        for mod in self.modules():
            pl += [(mod._parameters, k, p) for k, p in mod._parameters.items() if p is not None]
            pl += [(mod._buffers, k, b) for k, b in mod._buffers.items() if b is not None and k not in mod._non_persistent_buffers_set]
        self._plist = pl
        self._psig = tuple((p.data_ptr(), p._version) for _, _, p in pl)

    # ---- the handle ------------------------------------------------------------------------------
    def _library(self):
        """The shared object this module's handle lives in: libcwm_hip.so unless `use_library` chose the development one."""
        return self._cwm if self._cwm is not None else _lib.get_lib()

    def _check(self, rc):
        if rc:
            _lib.check(rc, self._library())

    def use_library(self, lib):
        """Create this model's handle in another build of the library (tools / tests: `_lib.get_dev_lib()`, whose per-shape tile overrides and
        thread-local switches a handle of the production library never sees).  Call before the first forward; an existing handle is released."""
        self._release()
        object.__setattr__(self, "_cwm", lib)

    def _create(self, lib, handle_out) -> int:
        """Fill the model kind's config struct and call its `cwm_*_create` with `C.byref(handle_out)`; returns the library's return code."""
        raise NotImplementedError

    def _ensure_handle(self, device: torch.device) -> int:
        if self._handle is not None and self._handle_device == device:
            return self._handle
        self._release()
        lib = self._library()
        h = C.c_void_p()
        with torch.cuda.device(device):
            self._check(self._create(lib, h))
        self._fn = {role: getattr(lib, name) for role, name in self._ABI.items()}
        self._handle, self._handle_device, self._loaded = h.value, device, {}
        for k, v in self.__dict__.get("_options", {}).items():
            self._check(self._fn["set_option"](self._handle, k.encode(), v))
        return self._handle

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            try:
                self._fn["destroy"](self._handle)
            except Exception:
                pass
            # plain attributes: nn.Module.__setattr__ can already be half torn down when __del__ runs at interpreter exit
            object.__setattr__(self, "_handle", None)
            object.__setattr__(self, "_loaded", {})

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ---- weights ---------------------------------------------------------------------------------
    def sync_weights(self, device: Optional[torch.device] = None, force: bool = False) -> int:
        """Push every state-dict tensor that changed since the last call into the library (which packs it for its kernels); returns how
        many were uploaded.  Counterpart of `load_state_dict` at the boundary.  A change is detected by object identity + (storage pointer,
        version counter) of every parameter: `load_state_dict`, `copy_`, optimiser steps, `p.data = t`, `.to()` / `.double()` on the model
        or a submodule, a replaced Parameter.  In-place edits through `.data` that keep the storage (`p.data.mul_(2)`) are NOT visible --
        call `sync_weights(force=True)` (or `invalidate_weights()`) after such an edit.  `device` defaults to the parameters' device; a
        CUDA tensor that lives on another device is moved to the handle's first."""
        if device is None:
            device = self._param_device()
        if not force and self._handle is not None and self._handle_device == device and self._params_unchanged():
            return 0
        h = self._ensure_handle(device)
        load = self._fn["load_weight"]
        if force:
            self._loaded = {}
        n = 0
        with torch.cuda.device(device):
            for name, p in self.state_dict(keep_vars=True).items():
                tag = (p.data_ptr(), p._version)
                if self._loaded.get(name) == tag:
                    continue
                t = p.detach()
                if t.dtype != torch.float32 or not t.is_contiguous():
                    t = t.float().contiguous()
                if t.is_cuda and t.device != device:
                    t = t.to(device)
                shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)  # (a 0-d tensor would give a zero-length array)
                self._check(load(h, name.encode(), t.data_ptr(), 1 if t.is_cuda else 0, shape, t.dim()))
                self._loaded[name] = tag
                n += 1
        self._remember_params()
        return n

    def invalidate_weights(self):
        """Forget what has been uploaded: the next forward re-packs every parameter (see `sync_weights`)."""
        self._loaded = {}
        self._plist = None

    # ---- per-handle options and kernel timing (bench.py roofline) ----------------------------------
    def _require_entry(self, role: str):
        if role not in self._ABI:
            raise RuntimeError("%s has no %s: the library has no such entry point for this model kind" % (type(self).__name__, role))

    def _call(self, role: str, doing: str, *args):
        self._require_entry(role)
        if self._handle is None:
            raise RuntimeError("run a forward pass (or sync_weights) before %s" % doing)
        self._check(self._fn[role](self._handle, *args))

    def set_option(self, key: str, value: int):
        """One execution option of THIS model (include/cwm_hip.h cwm_model_set_option / cwm_conj_set_option: "attn_kernel", "gemm_tile",
        "prune_last_block" ...): per handle, never process-wide.  Options set before the first forward are applied when the handle is
        created.  An unknown key / a refused value raises and leaves nothing behind."""
        self._require_entry("set_option")
        if getattr(self, "_handle", None) is not None:  # the library validates; remembered (for a re-created handle) only once it accepted
            self._check(self._fn["set_option"](self._handle, key.encode(), int(value)))
        else:
            _lib.validate_option(key, int(value))
        self.__dict__.setdefault("_options", {})[key] = int(value)

    def set_lanes(self, lanes: int):
        """1: every kernel on the current stream; 2 (library default): batches whose halves keep enough encoder rows (csrc/engine.h
        kMinLaneRows: ViT-B/8 from batch 8; kMinLaneRowsConj for the conjoined models) run as two half batches on two HIP streams,
        forked / joined inside the library, which fills the idle time between dependent kernels.  The plain predictor takes up to 4."""
        self._call("set_lanes", "set_lanes", int(lanes))

    def timing_enable(self, kclass: int, enable: bool = True):
        self._call("timing_enable", "enabling timing", kclass, int(enable))

    def timing_collect(self, kclass: int):
        st = _lib.CwmKernelStats()
        self._call("timing_collect", "collecting timing", kclass, C.byref(st))
        return {"launches": st.launches, "total_ms": st.total_ms, "total_flops": st.total_flops}
