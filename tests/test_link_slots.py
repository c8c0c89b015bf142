"""The coded links' synchroniser slots where no other test reaches them (waveforms_amd/encoding/coded.py): the ``*_result()`` methods
on the links that have no synchroniser keywords at all - the clipped loops of sccc.py, pccc.py and rsconv.py, which keep a ``_last``
of their own -, and ``samples()``, the noisy samples ``front_end`` works from, against ``front_end``'s own rows."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import make_coded_links as M  # noqa: E402

SOQPSK_RESULTS = {"carrier_result": "a recovery", "timing_result": "a timing_recovery", "acquisition_result": "an acquisition",
                  "coarse_result": "a coarse acquisition"}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["conv_outer3", "turbo_outer2", "rsconv_outer1", "coded_soqpsk_pt"])
def test_gpu_results_without_a_synchroniser_are_runtime_errors(case):
    """Before and after a block, with the documented words; the block leaves the class's own counters as they were recorded."""
    _cls, db, make = M.CASES[case]
    link = make(M._names())
    for ran in (False, True):
        for method, a in SOQPSK_RESULTS.items():
            with pytest.raises(RuntimeError) as e:
                getattr(link, method)()
            assert str(e.value) == f"{method} needs {a} and a block that ran"
        if not ran:
            link.run_block(db, seed=M.SEED, stream_id=0)
    assert link.blocks == 1 and link.uncoded_result()[1] == link.nch


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["coded_cpm_pcmfm", "coded_soqpsk_coarse_recovery"])
def test_gpu_samples_are_what_the_front_end_works_from(case):
    """``samples()``, then the link's correcting slot and its plain bank by hand, are ``front_end``'s rows bit for bit: on a plain
    CPM link and on an SOQPSK-TG link with ``coarse`` beside ``recovery`` (a plain SOQPSK-TG link takes the fused bank, another
    kernel)."""
    from waveforms_amd import _hip

    _cls, db, make = M.CASES[case]
    link = make(M._names())
    tx = link.encode(link.info_bits(1))
    rows, syms = link.front_end(tx, db, M.SEED, 1)
    received, at, syms2 = link.samples(tx, db, M.SEED, 1)
    if getattr(link, "coarse", None) is not None:
        received, _found = link.coarse.correct(received, out=received)
    got, want = _hip.to_host(link._bank(received, *at)), _hip.to_host(rows)
    assert got.shape == want.shape and np.array_equal(_hip.to_host(syms), _hip.to_host(syms2))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
