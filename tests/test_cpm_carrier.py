"""Carrier phase and frequency recovery for the generic CPM detectors (waveforms_amd/sync/carrier_cpm.py; include/wfhip.h:
wf_cpm_soft_branch, wf_carrier_stat_terms, wf_carrier_track_mod, wf_rows_derotate_n).

The definition of wf_cpm_soft_branch is restated sequentially in C (tests/cpm_carrier_ref.c: the recursion of
tests/cpm_soft_ref.c with branch and term, explicit fma, compiled with -ffp-contract=off).  CPU: the restatement against
cpm_soft_ref.c and against brute force over all paths, the numpy statement against the restatement on the oracle's rows,
``recover_cpm_host`` at constant rotations and at the documented drift.  GPU: every device stage against its statement -
λ, bits, branch and term bitwise, the statistics bitwise, the trajectory and the rotations within the bounds of the SOQPSK
stages' tests (tests/test_carrier.py) - and the whole recovery on a burst.
"""
import ctypes
import itertools
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_cpm_soft as TC
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import carrier_cpm as CC

SPS = 8
EPS = 2.0 ** -52
HERE = Path(__file__).resolve().parent
NAMES = ("wf_cpm_soft_branch", "wf_carrier_stat_terms", "wf_carrier_track_mod", "wf_rows_derotate_n")
WAVEFORMS = ["multih", "pcmfm"]
NOISY_DB = {"multih": 8.0, "pcmfm": 6.0}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = tmp_path_factory.mktemp("cpm_carrier_ref") / "libcpmcarrierref.so"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", str(so), str(HERE / "cpm_carrier_ref.c"), "-lm"])
    lib = ctypes.CDLL(str(so))
    for name in ("cpm_soft_rec", "cpm_soft_rows", "cpm_soft_branch_rec", "cpm_soft_branch_rows"):
        getattr(lib, name).restype = ctypes.c_int
    return lib


_p, _K, _specs = TC._p, TC._K, TC._specs


def restate(ref, spec, rows, first_call=0, rot=None):
    """The header's definition over complex128 rows [n][M^Lp] -> (llr, bits, branch, term[n, 2])."""
    rows = np.ascontiguousarray(rows, dtype=np.complex128).reshape(-1, spec.nfilt)
    n, lg = rows.shape[0], spec.bits_per_symbol
    llr, bits = np.empty(n * lg), np.empty(n * lg, dtype=np.uint8)
    branch, term = np.empty(n, dtype=np.uint8), np.empty((n, 2))
    rot = np.ascontiguousarray(CC.hypothesis_table(spec) if rot is None else rot)
    assert ref.cpm_soft_branch_rows(spec.M, spec.p, len(spec.K), _K(spec), spec.Lp, _p(rot), _p(rows), ctypes.c_int64(n),
                                    ctypes.c_int64(first_call), _p(llr), _p(bits), _p(branch), _p(term)) == 0
    return llr, bits, branch, term


def _oracle_rows(oracle, waveform, nsym, ebn0=None, seed=5):
    """(full-phase spec, complex128 rows of the oracle's chain on random symbols)."""
    spec = _specs()[waveform]
    rng = np.random.default_rng(seed)
    if waveform == "multih":
        sym, pulse = oracle.multih_mapper(rng.integers(0, 2, 2 * nsym).astype(np.uint8))[0], oracle.freq_pulse_multih_irig(SPS)
        ospec = oracle.ARTM_64
    else:
        sym, pulse = oracle.pcmfm_mapper(rng.integers(0, 2, nsym).astype(np.uint8)), oracle.freq_pulse_pcmfm(SPS)
        ospec = oracle.CPMDetectorSpec(M=2, p=10, K=(7,), Lp=2, NC=10, D=32)
    noise = None
    if ebn0 is not None:
        noise = oracle.numpy_awgn(oracle.cpm_sigma_for_ebn0(ebn0, SPS, spec.bits_per_symbol), (np.asarray(sym).size + 1) * SPS,
                                  np.random.Generator(np.random.PCG64(seed)))
    return spec, np.ascontiguousarray(oracle.cpm_detection_run(sym, pulse, SPS, ospec, noise=noise)["rows"])


def _rot(rows, deg=0.0, turns_per_window=0.0, window=C.DEFAULT_WINDOW):
    k = np.arange(rows.shape[0], dtype=np.float64)
    return rows * np.exp(1j * (math.radians(deg) + 2.0 * math.pi * turns_per_window * k / window))[:, None]


def _drift(spec, fraction=CC.MAX_DRIFT_PERIODS):
    """``fraction`` of P per window, in turns per window."""
    return fraction / spec.p


def _symbol_errors(spec, bits, genie, guard=8):
    lg = spec.bits_per_symbol
    d = (bits != genie).reshape(-1, lg).any(axis=1)
    return int(np.count_nonzero(d[guard:d.size - guard]))


# ------------------------------------------------------------------------------------------------ CPU
def test_cpm_carrier_entry_points_exported_bound_and_declared():
    from waveforms_amd import _hip, device
    from waveforms_amd.encoding import coded
    from waveforms_amd.viterbi import cpm

    header = (HERE.parent / "include" / "wfhip.h").read_text()
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header, name
    for name in ("cpm_soft_branch", "carrier_stat_terms", "rows_derotate_n", "carrier_track"):
        assert callable(getattr(device, name))
    for name in ("period", "hypothesis_table", "cpm_map_branch_host", "carrier_stat_terms_host", "recover_cpm_host"):
        assert callable(getattr(CC, name))
    rec = CC.CPMCarrierRecovery(cpm.ARTM_64)
    assert (rec.window, rec.span, rec.hypotheses, rec.refine) == (256, 5, 2, 1)
    assert CC.period(cpm.ARTM_64) == 2.0 * math.pi / 16 and CC.period(cpm.PCMFM_20) == 2.0 * math.pi / 10
    for spec in (cpm.ARTM_64, cpm.PCMFM_20):
        assert np.array_equal(CC.hypothesis_table(spec), cpm.rotation_table(spec))
        np.testing.assert_allclose(CC.hypothesis_table(spec, 0.3), np.stack([np.cos(np.pi * np.arange(2 * spec.p) / spec.p + 0.3),
                                                                            np.sin(np.pi * np.arange(2 * spec.p) / spec.p + 0.3)], axis=1))
    assert 0.0 < CC.MAX_DRIFT_PERIODS <= 0.125
    import inspect

    for cls in (coded.CodedCPMLink, coded.IterativeCPMLink):
        assert list(inspect.signature(cls.__init__).parameters)[-2:] == ["carrier", "recovery"]


def test_cpm_carrier_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before the context is touched (a fake context: no device exists here)."""
    from waveforms_amd import _hip
    from waveforms_amd.viterbi import cpm

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 15)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    b, c, d, e, f = a + 4096, a + 8192, a + 12288, a + 16384, a + 20480
    V = _hip.WF_ERR_VALUE
    nan, inf = float("nan"), float("inf")
    good = cpm.ARTM_64.c_config()

    # wf_cpm_soft_branch(ctx, det, rot, rows, ncalls, first_call, warmup, llr, bits, branch, term, stream)
    def call(cfg=good, ctx=fake, r=a, z=b, n=10, first=0, warmup=0, out=c, bits=d, branch=e, term=f):
        return lib.wf_cpm_soft_branch(ctx, None if cfg is None else ctypes.byref(cfg), r, z, n, first, warmup, out, bits, branch, term, None)

    assert call(ctx=None) == V and call(cfg=None) == V and call(r=None) == V and call(z=None) == V
    assert call(out=None) == V and call(bits=None) == V and call(branch=None) == V
    assert call(term=f + 8) == V and call(z=b + 8) == V and call(r=a + 8) == V and call(out=c + 4) == V
    for n in (0, -1):
        assert call(n=n) == V
    assert call(first=-1) == V and call(warmup=-1) == V
    for spec in (cpm.ARTM_16, cpm.PCMFM_10, cpm.ARTM_256):       # NC != p; 256 states
        assert call(cfg=spec.c_config()) == V
    for field, value in (("M", 3), ("M", 8), ("nh", 3), ("nh", 0), ("Lp", 0), ("Lp", 4), ("NC", 8)):
        cfg = cpm.ARTM_64.c_config()
        setattr(cfg, field, value)
        assert call(cfg=cfg) == V, (field, value)
    # wf_carrier_stat_terms(ctx, term, ncalls, W, stat, stream)
    for args in ((None, a, 10, 64, c), (fake, None, 10, 64, c), (fake, a, 10, 64, None), (fake, a, 0, 64, c), (fake, a + 8, 10, 64, c),
                 (fake, a, 10, 64, c + 4)) + tuple((fake, a, 10, w, c) for w in (0, 32, 63, 65, 96, 8256, 16384, -64)):
        assert lib.wf_carrier_stat_terms(*args, None) == V, args
    # wf_carrier_track_mod(ctx, stat_h, H, nwin, span, period, phase, choice, stream)
    P = 2.0 * math.pi / 16
    for args in ((None, a, 1, 4, 1, P, b, c), (fake, None, 1, 4, 1, P, b, c), (fake, a, 1, 4, 1, P, None, c), (fake, a, 1, 4, 1, P, b, None),
                 (fake, a, 0, 4, 1, P, b, c), (fake, a, 257, 4, 1, P, b, c), (fake, a, 1, 0, 1, P, b, c), (fake, a, 1, 4, 0, P, b, c),
                 (fake, a, 1, 4, 2, P, b, c), (fake, a + 4, 1, 4, 1, P, b, c), (fake, a, 1, 4, 1, P, b + 4, c),
                 (fake, a, 1, 4, 1, nan, b, c), (fake, a, 1, 4, 1, inf, b, c), (fake, a, 1, 4, 1, 0.0, b, c), (fake, a, 1, 4, 1, -P, b, c),
                 (fake, a, 1, 4, 1, math.nextafter(2.0 * math.pi, 7.0), b, c)):
        assert lib.wf_carrier_track_mod(*args, None) == V, args
    # wf_rows_derotate_n(ctx, rows, ncalls, nvals, W, phase, nwin, phase0, out, stream)
    for args in ((None, a, 10, 4, 64, b, 1, 0.0, c), (fake, None, 10, 4, 64, b, 1, 0.0, c), (fake, a, 10, 4, 64, b, 1, 0.0, None),
                 (fake, a, 0, 4, 64, b, 1, 0.0, c), (fake, a, 10, 0, 64, b, 1, 0.0, c), (fake, a, 10, 65, 64, b, 1, 0.0, c),
                 (fake, a, 10, -1, 64, b, 1, 0.0, c), (fake, a, 10, 4, 64, b, 1, nan, c), (fake, a, 10, 4, 64, None, 0, inf, c),
                 (fake, a, 10, 4, 96, b, 1, 0.0, c), (fake, a, 10, 4, 64, b, 0, 0.0, c), (fake, a + 8, 10, 4, 64, b, 1, 0.0, c),
                 (fake, a, 10, 4, 64, b, 1, 0.0, c + 8), (fake, a, 10, 4, 64, b + 4, 1, 0.0, c)):
        assert lib.wf_rows_derotate_n(*args, None) == V, args
    # ... and the Python layer's own
    for kw in ({"window": 96}, {"window": 32}, {"window": 16384}, {"span": 4}, {"span": 0}, {"hypotheses": 0}, {"hypotheses": 257}, {"refine": -1}):
        with pytest.raises(ValueError):
            CC.CPMCarrierRecovery(cpm.ARTM_64, **kw)
    for spec in (cpm.ARTM_256, cpm.ARTM_16, cpm.PCMFM_10):       # more than 64 states; not full-phase
        with pytest.raises(ValueError):
            CC.CPMCarrierRecovery(spec)
    with pytest.raises(ValueError):
        CC.carrier_stat_terms_host(np.zeros(4), np.zeros(4), 100)
    for bad in (0.0, -1.0, nan, 7.0):
        with pytest.raises(ValueError):
            C.carrier_track_host(np.zeros((1, 4, 2)), 1, bad)


@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_restatement_llr_and_bits_are_the_soft_restatements(ref, waveform):
    spec = _specs()[waveform]
    rng = np.random.default_rng(11)
    for n, first_call in ((1, 0), (2, 1), (7, 0), (300, 5)):
        rows = 2.0 * (rng.standard_normal((n, spec.nfilt)) + 1j * rng.standard_normal((n, spec.nfilt)))
        want_llr, want_bits = TC.restate(ref, spec, rows, first_call)
        llr, bits, branch, term = restate(ref, spec, rows, first_call)
        assert np.array_equal(llr.view(np.uint64), want_llr.view(np.uint64)) and np.array_equal(bits, want_bits)
        assert int(branch.max()) < spec.nstates * spec.M
        # the input symbol of the decided branch is the decision of every bit's λ: T's minimum is one of each bit's two minima
        assert np.array_equal(_bits_of(branch % spec.M, spec), bits)


def _bits_of(u, spec):
    lg = spec.bits_per_symbol
    return np.stack([(u >> (lg - 1 - i)) & 1 for i in range(lg)], axis=-1).reshape(-1).astype(np.uint8)


def brute_force_branch(spec, inc, first_call):
    """b*_k = the smallest M s + u among the branches of section k that lie on a path of minimum total cost: every start
    state, every input sequence."""
    n, S, M = inc.shape
    ends = [TC._ends(spec, first_call + k) for k in range(n)]
    best = np.full((n, S * M), np.inf)
    for s0 in range(S):
        for us in itertools.product(range(M), repeat=n):
            s, cost, on = s0, 0.0, []
            for k in range(n):
                on.append(s * M + us[k])
                cost += inc[k, s, us[k]]
                s = ends[k][s][us[k]]
            for k in range(n):
                best[k, on[k]] = min(best[k, on[k]], cost)
    return np.argmin(best, axis=1).astype(np.uint8)          # the first of equal minima


@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_restatement_branch_equals_brute_force(ref, waveform):
    """Integer increments: every sum is exact, so T_k(s, u) is the cheapest path through branch (s, u) minus a constant of the
    section, ties and all.  All-zero increments tie everywhere: branch 0."""
    spec = _specs()[waveform]
    S, M, lg = spec.nstates, spec.M, spec.bits_per_symbol
    rng = np.random.default_rng(3 + M)
    for first_call in (0, 1, 2):
        for n in range(1, 5):
            for inc in (rng.integers(-8, 9, (n, S, M)).astype(np.float64), rng.integers(-1, 2, (n, S, M)).astype(np.float64),
                        np.zeros((n, S, M))):
                llr, bits, branch = np.empty(n * lg), np.empty(n * lg, dtype=np.uint8), np.empty(n, dtype=np.uint8)
                assert ref.cpm_soft_branch_rec(M, spec.p, len(spec.K), _K(spec), spec.Lp, _p(inc), ctypes.c_int64(n), ctypes.c_int64(first_call),
                                               _p(llr), _p(bits), _p(branch)) == 0
                want = brute_force_branch(spec, inc, first_call)
                assert np.array_equal(branch, want), (first_call, n, branch, want)
                assert inc.any() or not branch.any()


@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_numpy_statement_agrees_with_the_restatement_on_oracle_rows(oracle, ref, waveform):
    """2000 calls at 8 dB (ARTM) / 6 dB (PCM/FM).  The numpy statement rounds an increment twice where the definition has one
    fma, so a call whose two best T lie within 1e-9 may pick another branch and is left out; at most 0.1 % of the calls may be."""
    spec, rows = _oracle_rows(oracle, waveform, 2010, NOISY_DB[waveform])
    rows = rows[:2000]
    assert rows.shape[0] == 2000
    for rot in (None, CC.hypothesis_table(spec, CC.period(spec) / 2.0)):
        want_llr, want_bits, want_branch, want_term = restate(ref, spec, rows, 0, rot)
        llr, bits, branch, x, y, gap = CC.cpm_map_branch_host(spec, rows, 0, rot, margins=True)
        keep = gap >= 1e-9
        print(f"{waveform}: {np.count_nonzero(~keep)} calls left out, smallest margin {gap.min():.3g}")
        assert np.count_nonzero(~keep) <= 2
        assert np.array_equal(branch[keep], want_branch[keep])
        np.testing.assert_allclose(llr, want_llr, rtol=0, atol=1e-9)
        np.testing.assert_allclose(np.stack([x, y], axis=1)[keep], want_term[keep], rtol=0, atol=1e-12 * SPS)
        lg = spec.bits_per_symbol
        assert np.array_equal(bits.reshape(-1, lg)[keep], want_bits.reshape(-1, lg)[keep])


@pytest.fixture(scope="module")
def genie(oracle):
    """4096 noiseless oracle rows per waveform, with the decisions of the unrotated rows."""
    out = {}
    for waveform in WAVEFORMS:
        spec, rows = _oracle_rows(oracle, waveform, 4110)
        rows = rows[:4096]
        assert rows.shape[0] == 4096
        out[waveform] = (spec, rows, CC.cpm_map_branch_host(spec, rows)[1])
    return out


def _cases(spec):
    P = 360.0 / spec.p
    d = _drift(spec)
    return [(5.0, 0.0), (P / 2.0, 0.0), (40.0, 0.0), (100.0, 0.0), (40.0, d), (40.0, -d)]


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_recover_cpm_host_rotations_and_the_documented_drift(genie, waveform, case):
    """Constant rotations of 5 degrees, P / 2, 40 and 100 degrees, and 40 degrees with +-MAX_DRIFT_PERIODS of P per window:
    the decisions after the recovery are the genie's outside the first and last 8 calls.  (The trajectory is not compared
    with the injected phase: the two-symbol matched filters leave a constant offset of a few degrees, harmless to the detector.)"""
    spec, rows, want = genie[waveform]
    deg, drift = _cases(spec)[case]
    out, phase, choice = CC.recover_cpm_host(spec, _rot(rows, deg, drift))
    assert phase.shape == choice.shape == (16,) and int(choice.max()) < CC.DEFAULT_HYPOTHESES
    assert _symbol_errors(spec, CC.cpm_map_branch_host(spec, out)[1], want) == 0
    # the steps of the trajectory follow the drift to a tenth of the documented step (windows 5 .. 10: the first and last two
    # are smoothed over fewer windows, and the refinement's own smoothing carries that two windows further in)
    np.testing.assert_allclose(np.degrees(np.diff(phase[5:-5])), 360.0 * drift, rtol=0, atol=0.1 * 360.0 * _drift(spec))


@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_one_hypothesis_is_not_enough(oracle, genie, waveform):
    """At P / 2 one hypothesis sits between two symmetric images; where the decisions of a window mix the two, its estimate is
    off by up to P / 2, and under the documented drift that costs decisions, which is why the search exists.  The rows at
    P / 2 with +-MAX_DRIFT_PERIODS of drift, in the two conditions the limit is documented for (noiseless, and the same
    symbols at 8 dB for ARTM / 6 dB for PCM/FM): over the four bursts one hypothesis makes errors against the transmitted
    symbols that two do not.  Measured, (+, -) drift: PCM/FM noiseless 3, 3 against 0, 0 and at 6 dB 8, 7 against 8, 6; ARTM at
    8 dB 47, 11 against 14, 7 - and noiseless 0, 0 against 0, 0: ARTM's noiseless path slips too rarely (14 symbols of 4096
    without any recovery) for a window to mix."""
    spec, rows, want = genie[waveform]
    noisy = _oracle_rows(oracle, waveform, 4110, NOISY_DB[waveform])[1][:4096]
    errs = {1: [], 2: []}
    for z in (rows, noisy):
        for sign in (1.0, -1.0):
            bad = _rot(z, 180.0 / spec.p, sign * _drift(spec))
            for H in (1, 2):
                out, _ph, _ch = CC.recover_cpm_host(spec, bad, hypotheses=H)
                errs[H].append(_symbol_errors(spec, CC.cpm_map_branch_host(spec, out)[1], want))
    print(f"{waveform}: symbol errors (noiseless +, -, noisy +, -) with one hypothesis {errs[1]}, with two {errs[2]}")
    assert errs[2][:2] == [0, 0]
    assert sum(errs[1]) > sum(errs[2])


def test_host_statements_at_their_edges():
    from waveforms_amd.viterbi import cpm

    x, y = np.arange(100.0), -np.arange(100.0)
    st = CC.carrier_stat_terms_host(x, y, 64)
    assert st.shape == (2, 2) and st[0, 0] == x[:64].sum() and st[1, 1] == y[64:].sum()
    # carrier_track_host with its default period is what it was: π
    stat = np.random.default_rng(2).standard_normal((3, 9, 2))
    a, b = C.carrier_track_host(stat, 3), C.carrier_track_host(stat, 3, math.pi)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the unwrapping follows a ramp through many periods
    P = CC.period(cpm.ARTM_64)
    true = 0.3 * P * np.arange(40)
    ramp = np.stack([-np.cos(true), -np.sin(true)], axis=1)[None]
    phase, _c = C.carrier_track_host(ramp, 1, P)
    np.testing.assert_allclose(phase - phase[0], true, atol=1e-9)
    z = np.ones((5, 4), dtype=np.complex128)
    np.testing.assert_allclose(CC.derotate_n_host(cpm.PCMFM_20, z, phase0=0.5), np.exp(-0.5j) * z)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    _hip.set_option(handle, _hip.WF_OPT_DET_FINAL_VERIFY, 1)
    yield handle
    _hip.free_ctx(handle)


def _counters(dev, handle):
    return dev.viterbi_unmerged(reset=True, ctx=handle), dev.viterbi_repaired(reset=True, ctx=handle)


def _same(got, want, what):
    from waveforms_amd import _hip

    llr, bits, branch, term = (_hip.to_host(t) for t in got)
    assert np.array_equal(llr.view(np.uint64), want[0].view(np.uint64)), (what, "llr", int(np.count_nonzero(llr != want[0])))
    assert np.array_equal(bits, want[1]), (what, "bits")
    assert np.array_equal(branch, want[2]), (what, "branch", int(np.count_nonzero(branch != want[2])))
    assert np.array_equal(term.view(np.uint64), want[3].view(np.uint64)), (what, "term", int(np.count_nonzero(term != want[3])))


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_cpm_soft_branch_any_chunking_short_bursts_and_first_call(ref, ctx, waveform):
    """λ, bits, branch and term bitwise the restatement's whatever the chunking, the warm-up and the first call; λ and bits
    bitwise ``cpm_soft``'s; all-zero rows tie everywhere and give branch 0; a turned table gives the restatement's result
    with the same table; ``terms=False`` leaves the rest alone."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec = _specs()[waveform]
    rng = np.random.default_rng(7)
    turned = CC.hypothesis_table(spec, CC.period(spec) / 2.0)
    d_turned = _hip.to_device(turned)
    for n in (1, 2, 3, 5, 33, 1001):
        rows = 2.0 * (rng.standard_normal((n, spec.nfilt)) + 1j * rng.standard_normal((n, spec.nfilt)))
        d_rows = _hip.to_device(rows)
        for first_call in (0, 1, 5):
            want = restate(ref, spec, rows, first_call)
            want_turned = restate(ref, spec, rows, first_call, turned)
            for chunk in (0, 1, 7, 64):
                _hip.set_option(ctx, _hip.WF_OPT_CPM_SOFT_CHUNK_CALLS, chunk)
                for warmup in (0, 1, 3):
                    _same(dev.cpm_soft_branch(d_rows, spec, first_call, warmup, ctx=ctx), want, (n, first_call, chunk, warmup))
                    assert _counters(dev, ctx)[0] == 0
                _same(dev.cpm_soft_branch(d_rows, spec, first_call, 0, ctx=ctx, d_rot=d_turned), want_turned, (n, first_call, chunk, "turned"))
            plain_llr, plain_bits = dev.cpm_soft(d_rows, spec, first_call, 0, ctx=ctx)
            assert np.array_equal(_hip.to_host(plain_llr).view(np.uint64), want[0].view(np.uint64)) and np.array_equal(_hip.to_host(plain_bits), want[1])
            llr, bits, branch, term = dev.cpm_soft_branch(d_rows, spec, first_call, 0, ctx=ctx, terms=False)
            assert term is None and np.array_equal(_hip.to_host(branch), want[2]) and np.array_equal(_hip.to_host(llr).view(np.uint64), want[0].view(np.uint64))
        zeros = np.zeros((n, spec.nfilt), dtype=np.complex128)
        got = dev.cpm_soft_branch(_hip.to_device(zeros), spec, 0, 1, ctx=ctx)
        _same(got, restate(ref, spec, zeros), (n, "zeros"))
        assert not _hip.to_host(got[2]).any()
    assert _counters(dev, ctx)[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_cpm_soft_branch_through_the_repairs_on_link_rows(ref, ctx, waveform):
    """20 000 link rows at 6 dB: with a 2-call warm-up the result comes through the repairs and is still the restatement's."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi.cpm import full_phase

    rows, _syms, spec = TC._link_rows(waveform, 20_000, 6.0)
    fspec = full_phase(spec)
    want = restate(ref, fspec, _hip.to_host(rows, complex_pairs=True))
    _counters(dev, ctx)
    for warmup in (0, 2):
        _same(dev.cpm_soft_branch(rows, fspec, 0, warmup, ctx=ctx), want, warmup)
        unproven, repaired = _counters(dev, ctx)
        assert unproven == 0
        if warmup == 2:
            assert repaired > 0


@pytest.mark.gpu
@pytest.mark.parametrize("window", [64, 256])
def test_carrier_stat_terms_bitwise(ctx, window):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(window)
    for n in (1, window - 1, window, 5 * window + 77, 2000):
        term = rng.standard_normal((n, 2))
        term[0] = (0.0, -0.0)                             # signed zeros among the terms
        want = CC.carrier_stat_terms_host(term[:, 0], term[:, 1], window)
        got = _hip.to_host(dev.carrier_stat_terms(_hip.to_device(term), window, ctx=ctx))
        assert got.shape == want.shape == (-(-n // window), 2)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, np.abs(got - want).max())


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 2])
def test_carrier_track_mod_against_the_host_statement(ctx, H):
    """Statistics of a noisy ramp through many periods.  choice exact; phase within 8 * 2^-52 * max(1, |phase|) * nwin of the
    host statement (wf_carrier_track's stated bound) for the periods 2π/16 and 2π/10; with period π bitwise wf_carrier_track."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(21 + H)
    for nwin in (1, 16, 1500):
        for period in (2.0 * math.pi / 16, 2.0 * math.pi / 10):
            true = 0.21 * period * np.arange(nwin) + 0.4
            stat = np.empty((H, nwin, 2))
            for h in range(H):
                ang = true - h * period / H
                amp = 200.0 * (1.0 + 0.5 * np.cos(2.0 * math.pi * ang / period))      # the hypothesis nearest a symmetric image wins
                stat[h, :, 0], stat[h, :, 1] = -amp * np.cos(ang), -amp * np.sin(ang)
            stat += 0.5 * rng.standard_normal(stat.shape)
            for span in (1, 5):
                phase, choice = dev.carrier_track(_hip.to_device(stat), span, ctx=ctx, period=period)
                want_phase, want_choice = C.carrier_track_host(stat, span, period)
                phase = _hip.to_host(phase)
                assert np.array_equal(_hip.to_host(choice), want_choice)
                bound = 8.0 * EPS * np.maximum(1.0, np.abs(want_phase)) * nwin
                assert (np.abs(phase - want_phase) <= bound).all(), (nwin, period, span, np.abs(phase - want_phase).max(), bound.min())
        d_stat = _hip.to_device(stat)
        a_phase, a_choice = dev.carrier_track(d_stat, 5, ctx=ctx)
        b_phase, b_choice = dev.carrier_track(d_stat, 5, ctx=ctx, period=math.pi)
        assert np.array_equal(_hip.to_host(a_phase).view(np.uint64), _hip.to_host(b_phase).view(np.uint64))
        assert np.array_equal(_hip.to_host(a_choice), _hip.to_host(b_choice))


def _rot_bound(z, ang):
    """tests/test_carrier.py, _rot_bound: (4 * 2^-52 + 2^-52 |φ|) |z| per element."""
    return (4.0 * EPS + EPS * np.abs(ang)) * np.abs(z)


@pytest.mark.gpu
def test_rows_derotate_n_against_numpy(ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi import cpm

    rng = np.random.default_rng(9)
    n, window = 1000, 64
    nwin = -(-n // window)
    phase = np.cumsum(rng.uniform(-0.4, 0.4, nwin)) + 50.0
    for spec in (cpm.PCMFM_20, cpm.ARTM_64):
        nv = spec.nfilt
        assert nv in (4, 16)
        rows = 3.0 * (rng.standard_normal((n, nv)) + 1j * rng.standard_normal((n, nv)))
        d_rows = _hip.to_device(rows)
        for ph, phase0, w in ((phase, 0.0, window), (phase, -1.25, window), (None, 2.5, 64), (phase[:1], 0.3, 1024), (phase[:4], 0.0, 256)):
            want = CC.derotate_n_host(spec, rows, w, ph, phase0)
            ang = phase0 + (0.0 if ph is None else C.interpolate_phase_host(n, w, ph)) + np.zeros(n)
            got = _hip.to_host(dev.rows_derotate_n(d_rows, nv, w, None if ph is None else _hip.to_device(ph), phase0, ctx=ctx), True).reshape(n, nv)
            assert (np.abs(got - want) <= _rot_bound(rows, ang[:, None])).all(), (nv, np.abs(got - want).max())
        buf = d_rows.clone()
        out = dev.rows_derotate_n(buf, nv, window, _hip.to_device(phase), 0.0, out=buf, ctx=ctx)
        assert out.data_ptr() == buf.data_ptr()
        ang = C.interpolate_phase_host(n, window, phase)
        assert (np.abs(_hip.to_host(buf, True).reshape(n, nv) - CC.derotate_n_host(spec, rows, window, phase)) <= _rot_bound(rows, ang[:, None])).all()
    # nvals = 3 is wf_rows_derotate, bit for bit
    rows = 3.0 * (rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3)))
    d_rows, d_phase = _hip.to_device(rows), _hip.to_device(phase)
    for ph, phase0 in ((d_phase, 0.7), (None, -2.0)):
        a = _hip.to_host(dev.rows_derotate(d_rows, window, ph, phase0, ctx=ctx))
        b = _hip.to_host(dev.rows_derotate_n(d_rows, 3, window, ph, phase0, ctx=ctx))
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_recover_cpm_on_a_burst(oracle, ref, ctx, waveform):
    """4096 noiseless calls turned by 40 degrees plus half the documented drift: the choices are the host statement's, the
    trajectory is within the tracker's bound of it (8 * 2^-52 * max(1, |phase|) * nwin), and the decisions after the recovery
    are the genie's outside 8 calls at each end."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec, rows = _oracle_rows(oracle, waveform, 4110)
    rows = rows[:4096]
    want = restate(ref, spec, rows)[1]
    bad = _rot(rows, 40.0, 0.5 * _drift(spec))
    rec = CC.CPMCarrierRecovery(spec)
    out, phase, choice = rec.recover(_hip.to_device(bad), ctx=ctx)
    host_out, host_phase, host_choice = CC.recover_cpm_host(spec, bad)
    assert np.array_equal(_hip.to_host(choice), host_choice)
    nwin = host_phase.size
    bound = 8.0 * EPS * np.maximum(1.0, np.abs(host_phase)) * nwin
    err =np.abs(_hip.to_host(phase) - host_phase)
    print(f"{waveform}: max |device - host| / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all(), (err.max(), bound.min())
    _llr, bits, _branch, _term = dev.cpm_soft_branch(out, spec, ctx=ctx)
    out = _hip.to_host(out, True).reshape(-1, spec.nfilt)
    assert np.array_equal(_hip.to_host(bits), restate(ref, spec, out)[1])
    assert _counters(dev, ctx)[0] == 0
    assert _symbol_errors(spec, _hip.to_host(bits), want) == 0
