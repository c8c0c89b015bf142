"""What the code objects (``LDPCCode``, ``ConvCode``, ``TurboCode``, ``RSCode``) share: the device handle with its one-device rule
and its teardown, the message check, the encoders of the codes that have a ``tx_var``, and the table that puncturing and the
transmit order make."""
from __future__ import annotations

import ctypes

import numpy as np


def transmit_table(sent: np.ndarray, tx_order=None) -> np.ndarray:
    """``tx_var`` from a boolean T x outputs matrix (variable order: True = sent) and ``tx_order``, a permutation of the
    surviving variables' ranks (None: increasing variable order)."""
    keep = np.flatnonzero(np.asarray(sent, dtype=bool).reshape(-1)).astype(np.int64)
    if keep.size == 0:
        raise ValueError("the puncture pattern sends nothing")
    if tx_order is not None:
        order = np.asarray(tx_order, dtype=np.int64).ravel()
        if order.size != keep.size or not np.array_equal(np.sort(order), np.arange(keep.size)):
            raise ValueError(f"tx_order must be a permutation of the {keep.size} surviving variables' ranks")
        keep = keep[order]
    return np.ascontiguousarray(keep, dtype=np.int64)


class DeviceCode:
    """A code whose tables live behind an opaque ``wf_*_code *`` on ONE device, made on first use and freed with the object.  A
    subclass names its ``wf_*_code_free`` (``_free``), makes the ``wf_*_code_create`` call (``_create``) and, where its device
    encoder takes messages of k bits, names the ``waveforms_amd.device`` function (``_encode``)."""

    _free: str
    _encode: str
    _handle = _handle_dev = _lib = None

    def _create(self, lib, ctx, out) -> int:
        """The ``wf_*_code_create`` call from ``c_tables()``: ``out`` receives the handle; returns the call's code."""
        raise NotImplementedError

    def handle(self) -> int:
        """The ``wf_*_code *`` of this code on the current device (made on first use)."""
        from .. import _hip

        dev = _hip.require_device()
        if self._handle is not None and self._handle_dev == dev:
            return self._handle
        if self._handle is not None:
            raise RuntimeError(f"this code's tables live on device {self._handle_dev}, not {dev}")
        out = ctypes.c_void_p()
        _hip.check(self._create(_hip.lib(), _hip.ctx(), ctypes.byref(out)))
        self._handle, self._handle_dev, self._lib = out.value, dev, _hip.lib()
        return self._handle

    def __del__(self):
        h, lib = self._handle, self._lib
        if h and lib is not None:
            try:
                getattr(lib, self._free)(h)
            except Exception:          # noqa: BLE001 - interpreter teardown
                pass
            self._handle = None

    def _messages(self, info) -> np.ndarray:
        """Messages as contiguous ncw x k uint8."""
        u = np.ascontiguousarray(np.atleast_2d(np.asarray(info, dtype=np.uint8)))
        if u.shape[1] != self.k:
            raise ValueError(f"messages must have k = {self.k} bits")
        return u

    def encode_host(self, info: np.ndarray) -> np.ndarray:
        """Host encoder: messages (ncw x k) -> transmitted bits (ncw x n_tx, uint8) in transmit order."""
        return np.ascontiguousarray(self.codeword_host(info)[:, self.tx_var])

    def encode(self, info: np.ndarray) -> np.ndarray:
        """Messages (ncw x k, 0/1) -> transmitted bits (ncw x n_tx, uint8), encoded on the GPU."""
        from .. import _hip
        from .. import device as dev

        return _hip.to_host(getattr(dev, self._encode)(self, _hip.to_device(self._messages(info))))
