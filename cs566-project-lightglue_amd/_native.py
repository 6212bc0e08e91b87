"""What the modules that own a native handle share (LightGlue, SuperGlue, SuperPoint,
SuperPointOpen, ALIKED): the handle's life cycle, the weight upload keyed by the parameters' version
counters, and the grow-only byte workspace.

A subclass gives

* ``_native_prefix``: the C-ABI family, one of ``"lg"``, ``"sg"``, ``"sp"``, ``"sp_aliked"``
  (selects ``<prefix>_destroy`` and ``<prefix>_load_weights``);
* ``_native_name``: how the fp32 / device error starts (``"<name> <key> is <dtype> on <device>"``);
* ``_create_handle(lib, device, h)``: ``<prefix>_create`` into ``h`` (a ``ctypes.c_void_p``);
* ``_native_state()``: the tensors ``<prefix>_load_weights`` takes, by schema name (default: the
  state dict);
* ``_weights_signature()``: a hashable that changes whenever one of those tensors does;

and calls ``_native_init()`` from its constructor.
"""
import ctypes

import torch
from torch import nn

from . import _lib


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class NativeModule(nn.Module):
    _native_prefix = None
    _native_name = None

    def _native_init(self):
        self._handle = None
        self._handle_device = None
        self._weights_key = None
        self._ws = None

    # ------------------------------------------------------------ what a subclass gives
    def _create_handle(self, lib, device, h):
        raise NotImplementedError

    def _native_state(self):
        return self.state_dict(keep_vars=True)

    def _weights_signature(self):
        raise NotImplementedError

    # ------------------------------------------------------------ optional hooks
    def _handle_stale(self, device):
        """True when the handle cannot serve ``device`` any more and must be rebuilt."""
        return self._handle_device != device

    def _on_handle_event(self):
        """Called after the handle was created and after weights were uploaded into it."""

    def _upload_stream(self, device):
        """The stream ``<prefix>_load_weights`` runs on."""
        return torch.cuda.current_stream(device)

    # ------------------------------------------------------------ handle and weights
    def _ensure_handle(self, device, upload=True):
        """The native handle on ``device``; with ``upload`` the tensors of ``_native_state()`` are
        (re)packed into it when ``_weights_signature()`` changed.  The training paths pass raw
        parameter pointers to every call and never need the packed copy (upload=False)."""
        lib = _lib.load()
        if self._handle is not None and self._handle_stale(device):
            getattr(lib, f"{self._native_prefix}_destroy")(self._handle)
            self._handle = None
        if self._handle is None:
            h = ctypes.c_void_p()
            self._create_handle(lib, device, h)
            self._handle, self._handle_device, self._weights_key = h, device, None
            self._on_handle_event()
        if not upload:
            return lib
        key = self._weights_signature()
        if key != self._weights_key:
            sd = self._native_state()
            names = list(sd)
            ts = []
            for n in names:
                t = sd[n].detach()
                if t.device != device or t.dtype != torch.float32:
                    raise RuntimeError(f"{self._native_name} {n} is {t.dtype} on {t.device}; "
                                       f"move the module to {device} in fp32")
                ts.append(t.contiguous())
            arr_n = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
            arr_p = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            arr_k = (ctypes.c_int64 * len(ts))(*[t.numel() for t in ts])
            what = f"{self._native_prefix}_load_weights"
            stream = self._upload_stream(device)
            _lib.check(getattr(lib, what)(self._handle, len(ts), arr_n, arr_p, arr_k, ctypes.c_void_p(stream.cuda_stream)),
                       what)
            stream.synchronize()  # the sources may be temporaries
            self._weights_key = key
            self._on_handle_event()
        return lib

    def reload_weights(self):
        """Force the next forward to re-upload every tensor.  Needed only after writes the
        signature cannot see: in-place writes through ``p.data`` (``p.data.copy_(...)``, EMA
        updates) bump the version counter of a temporary tensor, not of ``p``."""
        self._weights_key = None

    def _apply(self, fn, *args, **kwargs):  # .to() / .cuda() / .float(): parameters may be new tensors
        self._weights_key = None
        return super()._apply(fn, *args, **kwargs)

    def __del__(self):
        try:
            if self._handle is not None and _lib._lib is not None:
                getattr(_lib._lib, f"{self._native_prefix}_destroy")(self._handle)
        except Exception:
            pass

    def _workspace_bytes(self, nbytes, device):
        """A byte tensor of at least ``nbytes`` on ``device``, kept and only ever grown."""
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws
