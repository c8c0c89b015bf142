"""What the four code classes share (waveforms_amd/encoding/_code.py) and the one upload path behind their handles
(waveforms_amd/csrc/wf_code.h), on the smallest valid code of each family."""
import ctypes
import gc

import numpy as np
import pytest

from waveforms_amd.encoding import conv, ldpc, rs, turbo

CODES = {
    "conv": lambda: conv.nasa_k3(8),
    "turbo": lambda: turbo.TurboCode(8, np.arange(8), 0o7, (0o5,), 3),
    "rs": lambda: rs.RSCode.conventional(15, 11),
    "ldpc": lambda: ldpc.LDPCCode.from_parity_check(np.array([[1, 1, 0, 1], [0, 1, 1, 1]])),      # tests/test_ldpc.py: `ok`
}


def _no_device():
    import torch

    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_device(), reason="the upload's failure path needs a box without a HIP device")
@pytest.mark.parametrize("name", sorted(CODES))
def test_create_reports_a_failed_upload_and_leaves_no_handle(name):
    """A valid code on a fake context (device 0) where no device exists: the tables pass validation, the upload fails at its
    first step, and the caller gets WF_ERR_HIP, a NULL handle and the step's name."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    code = CODES[name]()
    fake = ctypes.create_string_buffer(1 << 16)
    out = ctypes.c_void_p(0xDEAD)
    assert code._create(lib, fake, ctypes.byref(out)) == _hip.WF_ERR_HIP
    assert out.value is None
    assert lib.wf_last_error_string().decode().startswith(f"wf_{name}_code_create: hipSetDevice failed: ")
    assert getattr(lib, code._free)(None) == 0


class _FreeRecorder:
    """Stands in for a code's ``_lib``: forwards every call and notes it."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            rc = fn(*args)
            self.calls.append((name, args, rc))
            return rc

        return call


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CODES))
def test_gpu_handle_encode_teardown_and_the_one_device_rule(name):
    rng = np.random.default_rng(5)
    code = CODES[name]()
    msgs = rng.integers(0, 256, size=(3, 11), dtype=np.uint8) if name == "rs" else rng.integers(0, 2, size=(3, code.k), dtype=np.uint8)
    h = code.handle()
    assert h and code.handle() == h
    want = code.encode_host(msgs)
    assert np.array_equal(code.encode(msgs), want) and code.handle() == h
    freed = code._lib = _FreeRecorder(code._lib)
    del code
    gc.collect()
    assert freed.calls == [(f"wf_{name}_code_free", (h,), 0)]
    fresh = CODES[name]()
    assert np.array_equal(fresh.encode(msgs), want)
    fresh._handle_dev += 1
    with pytest.raises(RuntimeError, match="tables live on device"):
        fresh.handle()
    fresh._handle_dev -= 1
    assert fresh.handle()
