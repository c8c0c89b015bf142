"""tests/golden/code_refusals.json: every call the C refusal tests of the four code families make that the library refuses, in
order: [function, return code, wf_last_error_string()].  The tests (TESTS below) need no GPU: they hand the library invalid codes
and calls on a fake context.  ``record()`` runs them with ``_hip.lib`` replaced by a proxy that forwards every call and notes each
negative return; tests/test_code_refusals.py does the same and compares the whole list, so a change of the host code that is meant
to move a check without rewording or reordering it can show that it did.  Names, integers and message texts only.

    python3 tests/golden/make_code_refusals.py        (writes the JSON)
"""
import importlib
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "code_refusals.json"
TESTS = [("test_conv", "test_c_create_refuses_invalid_codes_without_a_gpu"),
         ("test_turbo", "test_c_entry_points_refuse_invalid_arguments_without_a_gpu"),
         ("test_turbo", "test_c_decode_refuses_every_invalid_argument_without_a_gpu"),
         ("test_rs", "test_c_create_refuses_invalid_codes_without_a_gpu"),
         ("test_ldpc", "test_c_create_refuses_invalid_codes_without_a_gpu"),
         ("test_rs_erasures", "test_c_refusals_without_a_gpu"),
         ("test_idd", "test_idd_argument_validation_without_a_gpu")]


class _Recorder:
    """Stands in for the loaded library: every function is the library's own, with its refusals noted."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            rc = fn(*args)
            if isinstance(rc, int) and not isinstance(rc, bool) and rc < 0:
                self._log.append([name, rc, self._lib.wf_last_error_string().decode()])
            return rc

        return call


def record() -> list:
    from waveforms_amd import _hip

    real, log = _hip.lib, []
    proxy = _Recorder(real(), log)
    _hip.lib = lambda: proxy
    try:
        for module, test in TESTS:
            getattr(importlib.import_module(module), test)()
    finally:
        _hip.lib = real
    return log


if __name__ == "__main__":
    here = Path(__file__).resolve().parent
    sys.path[:0] = [str(here.parent.parent), str(here.parent)]
    refusals = record()
    OUT.write_text(json.dumps(refusals, indent=0) + "\n")
    print("wrote", OUT, len(refusals), "refusals,", len({tuple(r) for r in refusals}), "distinct")
