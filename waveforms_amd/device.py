"""Device-tensor level wrappers of the C ABI (one function per kernel entry point).

Inputs and outputs are torch tensors on the GPU (used purely as HBM buffers);
complex128 data is float64[..., 2].  Everything is asynchronous on the current torch
stream.  The reference-shaped host API (``waveforms_amd.cpm`` ...) is built on these.
"""
from __future__ import annotations

import contextlib
import ctypes
import math

import numpy as np

from . import _hip

_u64 = lambda v: ctypes.c_uint64(int(v) & 0xFFFFFFFFFFFFFFFF)  # noqa: E731


def _ctx(ctx):
    """The caller's private wf_ctx, or the device's shared one."""
    return ctx if ctx is not None else _hip.ctx()


def _geometry(c_fn: str, names, *args) -> dict:
    """The int64 words a ``wf_*_geometry`` entry point writes behind ``args``, by name."""
    g = (ctypes.c_int64 * len(names))()
    _hip.check(getattr(_hip.lib(), c_fn)(*args, g))
    return dict(zip(names, (int(v) for v in g)))


def lfsr_bits(degree: int, mask: int, state: int, n: int, skip: int = 0):
    """K1 -> (bits u8[n] on device, register state after skip+n steps)."""
    out = _hip.empty(max(n, 1) + 16, "uint8")
    st = ctypes.c_uint64(0)
    _hip.check(_hip.lib().wf_lfsr_generate(_hip.ctx(), degree, _u64(mask), _u64(state), _u64(skip),
                                           _hip.ptr(out), n, ctypes.byref(st), _hip.stream()))
    return out[:n], st.value


def fsm_encode(next_tab: np.ndarray, out_tab: np.ndarray, bits, i0: int = 0, state0: int = 0,
               want_state: bool = True):
    """K2 -> (symbols i8 on device, final state or None)."""
    columns, states, ninp = next_tab.shape
    card = ninp.bit_length() - 1
    nbits = int(bits.numel())
    nxt = np.ascontiguousarray(next_tab, dtype=np.uint8)
    out = np.ascontiguousarray(out_tab, dtype=np.int8)
    sym = _hip.empty(nbits // card + 16, "int8")
    st = ctypes.c_int(state0)
    _hip.check(_hip.lib().wf_fsm_encode(
        _hip.ctx(), nxt.ctypes.data, out.ctypes.data, columns, states, card, _hip.ptr(bits), nbits, i0,
        state0, _hip.ptr(sym), ctypes.byref(st) if want_state else None, _hip.stream()))
    return sym[:nbits // card], (st.value if want_state else None)


def symbol_map(kind: int, bits, parity: int = 0, mem=(0, 0)):
    n = int(bits.numel())
    if kind == 1 and n % 2:
        raise ValueError("Odd length bit array passed into quaternary mapper.")
    nout = n // 2 if kind == 1 else n
    out = _hip.empty(nout + 16, "int8")
    _hip.check(_hip.lib().wf_symbol_map(_hip.ctx(), kind, _hip.ptr(bits), n, parity, int(mem[0]), int(mem[1]),
                                        _hip.ptr(out), _hip.stream()))
    return out[:nout]


def upsample_fir(symbols, h, pulse, sps: int):
    """K3 -> freq pulses f64[max((N+1)*sps, M)] on device."""
    nsym, ntaps = int(symbols.numel()), int(pulse.numel())
    n = _hip.lib().wf_fir_out_len(nsym, sps, ntaps)
    out = _hip.empty(n, "float64")
    _hip.check(_hip.lib().wf_upsample_fir_f64(_hip.ctx(), _hip.ptr(symbols), nsym, _hip.ptr(h), int(h.numel()),
                                              _hip.ptr(pulse), ntaps, sps, _hip.ptr(out), _hip.stream()))
    return out


def phase_cexp(freq, sps: int, phi0: float, revs_in: float = 0.0, revs_out=None):
    """K4 -> complex signal f64[n, 2] on device."""
    n = int(freq.numel())
    out = _hip.empty((n, 2), "float64")
    _hip.check(_hip.lib().wf_phase_cexp_f64(_hip.ctx(), _hip.ptr(freq), n, sps, float(phi0), float(revs_in),
                                            _hip.ptr(out), _hip.ptr(revs_out), _hip.stream()))
    return out


def cpm_modulate(symbols, h, pulse, sps: int, phi0: float = math.pi / 4, fused: bool = True):
    """K3 + K4.  Fused single-pass kernel when the configuration allows it, otherwise (or
    with fused=False) the FIR stage followed by the phase-scan stage."""
    nsym, ntaps = int(symbols.numel()), int(pulse.numel())
    if fused:
        n = _hip.lib().wf_fir_out_len(nsym, sps, ntaps)
        out = _hip.empty((n, 2), "float64")
        rc = _hip.lib().wf_cpm_modulate_c128(_hip.ctx(), _hip.ptr(symbols), nsym, _hip.ptr(h), int(h.numel()),
                                            _hip.ptr(pulse), ntaps, sps, float(phi0), _hip.ptr(out), _hip.stream())
        if rc == 0:
            return out
        if rc < 0:
            _hip.check(rc)
    return phase_cexp(upsample_fir(symbols, h, pulse, sps), sps, phi0)


def phase_modulate(phase, sens: float):
    n = int(phase.numel())
    out = _hip.empty((n, 2), "float64")
    _hip.check(_hip.lib().wf_phase_modulate_f64(_hip.ctx(), _hip.ptr(phase), n, float(sens), _hip.ptr(out),
                                                _hip.stream()))
    return out


def time_axis(n: int, step: float):
    out = _hip.empty(n, "float64")
    _hip.check(_hip.lib().wf_time_axis_f64(_hip.ctx(), n, float(step), _hip.ptr(out), _hip.stream()))
    return out


def awgn(signal, n: int, sigma: float, seed: int, stream_id: int = 0, first_index: int = 0,
         rot: complex = 1.0, out=None):
    """K5: out = signal*rot + noise (signal may be None -> pure noise)."""
    if out is None:
        out = _hip.empty((n, 2), "float64")
    rot = complex(rot)
    _hip.check(_hip.lib().wf_awgn_c128(_hip.ctx(), _hip.ptr(signal), n, rot.real, rot.imag, float(sigma),
                                       _u64(seed), _u64(stream_id), _u64(first_index), _hip.ptr(out),
                                       _hip.stream()))
    return out


def box_muller32(words, sigma: float):
    """Box-Muller of caller-supplied word pairs: ``words`` int32[n, 2] (bit patterns of the
    uint32 radius / angle words) -> complex samples f64[n, 2]."""
    n = int(words.shape[0])
    out = _hip.empty((n, 2), "float64")
    _hip.check(_hip.lib().wf_box_muller32_c128(_hip.ctx(), _hip.ptr(words), n, float(sigma), _hip.ptr(out), _hip.stream()))
    return out


def mf_bank(received, taps, first: int, step: int, ncols: int):
    """K6/K7 -> rows f64[ncols, nfilt, 2] on device; taps f64[nfilt, ntaps, 2]."""
    nsamp = int(received.shape[0])
    nfilt, ntaps = int(taps.shape[0]), int(taps.shape[1])
    out = _hip.empty((max(ncols, 0), nfilt, 2), "float64")
    _hip.check(_hip.lib().wf_mf_bank_c128(_hip.ctx(), _hip.ptr(received), nsamp, _hip.ptr(taps), nfilt, ntaps,
                                          first, step, ncols, _hip.ptr(out), _hip.stream()))
    return out


def awgn_mf_bank(signal, taps, first: int, step: int, ncols: int, sigma: float, seed: int, stream_id: int = 0,
                 first_index: int = 0, rot: complex = 1.0):
    """K5 + K6 fused: rows of MF(signal*rot + noise) without materialising the noisy signal."""
    nsamp = int(signal.shape[0])
    nfilt, ntaps = int(taps.shape[0]), int(taps.shape[1])
    out = _hip.empty((max(ncols, 0), nfilt, 2), "float64")
    rot = complex(rot)
    _hip.check(_hip.lib().wf_awgn_mf_bank_c128(_hip.ctx(), _hip.ptr(signal), nsamp, rot.real, rot.imag, float(sigma),
                                               _u64(seed), _u64(stream_id), _u64(first_index), _hip.ptr(taps), nfilt,
                                               ntaps, first, step, ncols, _hip.ptr(out), _hip.stream()))
    return out


def viterbi_detect_count(mf_rows, ref_bits, ref_syms, skip: int, ncompare: int, counts, differential: bool = True,
                         warmup: int = 0):
    """K8-K11 fused: decisions + error counts (added to ``counts``) in one launch."""
    ncalls = int(mf_rows.shape[0])
    bits = _hip.empty(ncalls + 16, "uint8")
    syms = _hip.empty(ncalls + 16, "int8")
    _hip.check(_hip.lib().wf_viterbi4_detect_count(_hip.ctx(), _hip.ptr(mf_rows), ncalls, int(bool(differential)), warmup,
                                                   _hip.ptr(bits), _hip.ptr(syms), _hip.ptr(ref_bits), _hip.ptr(ref_syms),
                                                   skip, ncompare, _hip.ptr(counts), _hip.stream()))
    return bits[:ncalls], syms[:ncalls]


def viterbi_detect(mf_rows, differential: bool = True, warmup: int = 0, state=None, ctx=None):
    """K8-K10 (length 2) -> (bits u8[ncalls], symbols i8[ncalls]) on device.  ``ctx``: a private
    wf_ctx (own scratch and own unmerged-chunk counter) instead of the device's shared one."""
    ncalls = int(mf_rows.shape[0])
    bits = _hip.empty(ncalls + 16, "uint8")
    syms = _hip.empty(ncalls + 16, "int8")
    _hip.check(_hip.lib().wf_viterbi4_detect(_ctx(ctx), _hip.ptr(mf_rows), ncalls, int(bool(differential)),
                                             warmup, _hip.ptr(bits), _hip.ptr(syms), _hip.ptr(state),
                                             _hip.stream()))
    return bits[:ncalls], syms[:ncalls]


def viterbi_detect_window(mf_rows, length: int, differential: bool = True, warmup: int = 0, state=None, ctx=None):
    """K8-K10 for any window ``length`` (1 .. 64, odd ones as the reference pairs them) -> (bits u8[ncalls], symbols i8[ncalls]) on device;
    ``state``: float64[wf_viterbi4_window_state_bytes() / 8] carry (zeros = a fresh detector) or None."""
    ncalls = int(mf_rows.shape[0])
    bits = _hip.empty(ncalls + 16, "uint8")
    syms = _hip.empty(ncalls + 16, "int8")
    _hip.check(_hip.lib().wf_viterbi4_detect_window(_ctx(ctx), _hip.ptr(mf_rows), ncalls, int(length),
                                                    int(bool(differential)), warmup, _hip.ptr(bits), _hip.ptr(syms),
                                                    _hip.ptr(state), _hip.stream()))
    return bits[:ncalls], syms[:ncalls]


def viterbi_soft(rows, differential: bool = True, warmup: int = 0, row_bytes: int = 48, ctx=None):
    """Max-log-MAP soft output over the SOQPSK 4-state trellis (``wf_viterbi4_soft``; include/wfhip.h states the
    definition) -> (llr f64[ncalls], bits u8[ncalls]) on device, one fresh burst.  ``rows``: a contiguous device
    tensor of ncalls rows, 48 B each (float64[n, 3, 2]) or, ``row_bytes=32``, the links' detector-packed rows
    {Re z1, Im z1, a, b}.  λ_k > 0 favours bit 0, bits_k = λ_k < 0, and transmitted bit j pairs with λ_{j+1}.
    λ is in metric units: λ/σ² over-states the confidence of the PT and PAM metrics (see tools/soft_bench.py for the
    fitted scale).  The hard decisions are the ML sequence, not the length-2 detector's, and can have MORE bit errors
    than it.  Proof counters as for the hard detectors (viterbi_unmerged / viterbi_repaired)."""
    ncalls = _rows(rows, row_bytes, allow_empty=True)
    llr = _hip.empty(max(ncalls, 1), "float64")
    bits = _hip.empty(ncalls + 16, "uint8")
    _hip.check(_hip.lib().wf_viterbi4_soft(_ctx(ctx), _hip.ptr(rows), ncalls, int(row_bytes),
                                           int(bool(differential)), int(warmup), _hip.ptr(llr), _hip.ptr(bits), _hip.stream()))
    return llr[:ncalls], bits[:ncalls]


def viterbi_soft_geometry(ncalls: int, warmup: int = 0, ctx=None) -> dict:
    """What ``viterbi_soft`` launches for a burst of ``ncalls`` rows on this context (``wf_viterbi4_soft_geometry``)."""
    return _geometry("wf_viterbi4_soft_geometry", ("chunk_calls", "lanes", "warmup", "scratch_bytes"), _ctx(ctx), int(ncalls), int(warmup))


def viterbi_soft_apriori(rows, apriori=None, apriori_scale: float = 1.0, differential: bool = True, warmup: int = 0,
                         row_bytes: int = 48, ctx=None):
    """``viterbi_soft`` with a per-row prior and extrinsic output (``wf_viterbi4_soft_apriori``; include/wfhip.h states
    the definition) -> (ext f64[ncalls], bits u8[ncalls]) on device.  ``apriori``: a contiguous device float32 tensor of
    ncalls values (row k's prior at [k]: transmitted bit j's at [j + 1]) or None (= ``viterbi_soft``, bitwise);
    π = ``apriori_scale`` * apriori > 0 favours bit 0.  ``ext`` leaves the prior of its own bit out (it is what an outer
    decoder is fed); ``bits`` are the decisions of ext + π.  Geometry: ``viterbi_soft_geometry``."""
    ncalls = _rows(rows, row_bytes, allow_empty=True)
    if apriori is not None:
        if apriori.dtype != _hip.torch().float32 or not apriori.is_contiguous() or apriori.numel() != ncalls:
            raise ValueError(f"apriori must be {ncalls} contiguous float32 values (one per row)")
    ext = _hip.empty(max(ncalls, 1), "float64")
    bits = _hip.empty(ncalls + 16, "uint8")
    _hip.check(_hip.lib().wf_viterbi4_soft_apriori(_ctx(ctx), _hip.ptr(rows), ncalls, int(row_bytes),
                                                   int(bool(differential)), int(warmup), _hip.ptr(apriori), float(apriori_scale),
                                                   _hip.ptr(ext), _hip.ptr(bits), _hip.stream()))
    return ext[:ncalls], bits[:ncalls]


def _rows(rows, row_bytes: int, allow_empty: bool) -> int:
    """The number of rows in a contiguous tensor of 32- or 48-byte detector rows."""
    if row_bytes not in (32, 48):
        raise ValueError(f"row_bytes must be 32 or 48, not {row_bytes}")
    if not rows.is_contiguous():
        raise ValueError("rows must be contiguous")
    nbytes = rows.numel() * rows.element_size()
    if nbytes % row_bytes or (nbytes == 0 and not allow_empty):
        raise ValueError(f"{nbytes} bytes of rows are not a whole number of {row_bytes}-byte rows")
    return nbytes // row_bytes


def _rows48(rows) -> int:
    if not rows.is_contiguous():
        raise ValueError("rows must be contiguous")
    nbytes = rows.numel() * rows.element_size()
    if nbytes % 48 or nbytes == 0 or rows.dtype != _hip.torch().float64:
        raise ValueError(f"{nbytes} bytes of rows are not a whole number of 48-byte float64 rows")
    return nbytes // 48


def _trajectory(name: str, traj) -> int:
    """nwin of a per-window trajectory argument (``phase`` or ``tau``: contiguous device float64[nwin]); None: 0."""
    if traj is None:
        return 0
    if traj.dtype != _hip.torch().float64 or not traj.is_contiguous() or traj.numel() < 1:
        raise ValueError(f"{name} must be contiguous float64[nwin]")
    return int(traj.numel())


def _stat_out(out, nwin: int):
    """Where a statistic goes: ``out`` checked as contiguous float64[nwin, 2], or a new table."""
    if out is None:
        return _hip.empty((nwin, 2), "float64")
    if out.dtype != _hip.torch().float64 or not out.is_contiguous() or out.numel() != 2 * nwin:
        raise ValueError(f"out must be contiguous float64[{nwin}, 2]")
    return out


def carrier_offset(signal, theta0: float, nu: float, first_index: int = 0, out=None):
    """The carrier impairment at sample rate (``wf_carrier_offset_c128``; include/wfhip.h states the definition): out_k = in_k
    exp(j (theta0 + 2π frac(nu (first_index + k)))), ``nu`` in cycles per sample.  ``signal``: contiguous device float64[n, 2];
    ``out=signal`` works in place."""
    torch = _hip.torch()
    if signal.dtype != torch.float64 or not signal.is_contiguous() or signal.numel() % 2 or signal.numel() == 0:
        raise ValueError("signal must be contiguous float64[n, 2]")
    n = signal.numel() // 2
    if out is None:
        out = _hip.empty((n, 2), "float64")
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != signal.numel():
        raise ValueError("out must be contiguous float64[n, 2]")
    _hip.check(_hip.lib().wf_carrier_offset_c128(_hip.ctx(), _hip.ptr(signal), n, float(theta0), float(nu), int(first_index), _hip.ptr(out),
                                                 _hip.stream()))
    return out


def _samples(name: str, signal) -> int:
    """n of a sample argument: contiguous device float64[n, 2]."""
    if signal.dtype != _hip.torch().float64 or not signal.is_contiguous() or signal.numel() % 2 or signal.numel() == 0:
        raise ValueError(f"{name} must be contiguous float64[n, 2]")
    return signal.numel() // 2


def coarse_lines(received, sps: int, smooth: int, nfft: int, window, out=None, scratch=None, ctx=None):
    """The periodograms of the two spectral lines of the squared SOQPSK-TG signal (``wf_coarse_lines_c128``; include/wfhip.h states
    the definition) -> device float64[2, nfft] = (P₋, P₊) in fftshift order.  ``received``: contiguous device float64[n, 2];
    ``window``: contiguous device float64[nfft]; ``scratch``: a contiguous device float64 tensor of at least
    ``wf_coarse_scratch_doubles`` values to reuse (None: a new one per call).  A burst that does not fill one segment of ``nfft``
    bits is a ValueError."""
    torch = _hip.torch()
    n = _samples("received", received)
    if window.dtype != torch.float64 or not window.is_contiguous() or window.numel() != int(nfft):
        raise ValueError(f"window must be contiguous float64[{int(nfft)}]")
    words = _hip.lib().wf_coarse_scratch_doubles(n, int(sps), int(nfft), int(smooth))
    if words < 1:
        raise ValueError(f"coarse_lines: {n} samples at sps = {sps}, smooth = {smooth} do not fill one segment of nfft = {nfft} bits, or an "
                         "argument is out of range (sps 2 .. 64, smooth 1 .. 1024, nfft a power of two from 64 to 4096)")
    if out is None:
        out = _hip.empty((2, int(nfft)), "float64")
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 2 * int(nfft):
        raise ValueError(f"out must be contiguous float64[2, {int(nfft)}]")
    if scratch is None:
        scratch = _hip.empty(words, "float64")
    elif scratch.dtype != torch.float64 or not scratch.is_contiguous() or scratch.numel() < words:
        raise ValueError(f"scratch must be a contiguous float64 tensor of at least {words} values")
    _hip.check(_hip.lib().wf_coarse_lines_c128(_ctx(ctx), _hip.ptr(received), n, int(sps), int(smooth), int(nfft), _hip.ptr(window),
                                               _hip.ptr(scratch), _hip.ptr(out), _hip.stream()))
    return out


def coarse_estimate(spectra, sps: int, search: int, out=None, ctx=None):
    """The carrier frequency from the two line periodograms (``wf_coarse_estimate``; include/wfhip.h states the definition) ->
    device float64[4] = (nu in cycles per sample, eps, the peak of the summed periodogram, its mean).  ``spectra``: contiguous
    device float64[2, nfft]."""
    torch = _hip.torch()
    if spectra.dtype != torch.float64 or not spectra.is_contiguous() or spectra.dim() != 2 or spectra.shape[0] != 2:
        raise ValueError("spectra must be contiguous float64[2, nfft]")
    if out is None:
        out = _hip.empty(4, "float64")
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 4:
        raise ValueError("out must be contiguous float64[4]")
    _hip.check(_hip.lib().wf_coarse_estimate(_ctx(ctx), _hip.ptr(spectra), int(spectra.shape[1]), int(sps), int(search), _hip.ptr(out),
                                             _hip.stream()))
    return out


def carrier_offset_dev(signal, nu, gain: float = 1.0, first_index: int = 0, out=None, ctx=None):
    """``carrier_offset`` with theta0 = 0 and the frequency ``gain`` * nu[0] read from device memory (``wf_carrier_offset_dev_c128``):
    bitwise ``carrier_offset(signal, 0.0, gain * nu)`` for the same value, with nothing brought to the host.  ``nu``: a contiguous
    device float64 tensor (its first value is read: ``coarse_estimate``'s output as it is); ``out=signal`` works in place."""
    torch = _hip.torch()
    n = _samples("signal", signal)
    if nu.dtype != torch.float64 or not nu.is_contiguous() or nu.numel() < 1:
        raise ValueError("nu must be a contiguous float64 tensor of at least one value")
    if out is None:
        out = _hip.empty((n, 2), "float64")
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != signal.numel():
        raise ValueError("out must be contiguous float64[n, 2]")
    _hip.check(_hip.lib().wf_carrier_offset_dev_c128(_ctx(ctx), _hip.ptr(signal), n, _hip.ptr(nu), float(gain), int(first_index), _hip.ptr(out),
                                                     _hip.stream()))
    return out


def noncoherent_templates(pulse, h: float, sps: int, N: int, offset: int | None = None):
    """The multi-symbol noncoherent detector's hypothesis table on the device: float64[2^N, N sps, 2], a host build
    (``viterbi.noncoherent.noncoherent_templates_host``, which states the definition) and one upload.  ``offset=None``:
    ``DEFAULT_OFFSET``."""
    from .viterbi import noncoherent as nc

    return _hip.to_device(nc.noncoherent_templates_host(pulse, h, sps, N, nc.DEFAULT_OFFSET if offset is None else offset))


def noncoherent_geometry(N: int, sps: int, nbits: int, ctx=None) -> dict:
    """What ``noncoherent_soft`` launches (``wf_noncoherent_geometry``): bits per tile (one workgroup), workgroups, LDS bytes each."""
    return _geometry("wf_noncoherent_geometry", ("tile_bits", "workgroups", "lds_bytes"), _ctx(ctx), int(N), int(sps), int(nbits))


def noncoherent_soft(received, templates, sps: int, start: int, nbits: int, out=None, ctx=None):
    """The multi-symbol noncoherent soft detector (``wf_noncoherent_soft_c128``; include/wfhip.h states the definition) -> (λ
    float64[nbits], bits uint8[nbits]) on the device.  ``received``: contiguous device float64[n, 2]; ``templates``: contiguous
    device float64[2^N, N sps, 2] (``noncoherent_templates``); bit j's window begins at sample ``start`` + (j - (N - 1) / 2) sps and
    samples outside the burst read as zero.  λ > 0 favours bit 0, bits = λ < 0.  ``out``: a (λ, bits) pair of contiguous device
    tensors of ``nbits`` values to write into."""
    torch = _hip.torch()
    n, sps, nbits = _samples("received", received), int(sps), int(nbits)
    if templates.dtype != torch.float64 or not templates.is_contiguous() or templates.dim() != 3 or templates.shape[2] != 2:
        raise ValueError("templates must be contiguous float64[2^N, N sps, 2]")
    rows, K = int(templates.shape[0]), int(templates.shape[1])
    N = K // sps if sps > 0 else 0
    if N not in (3, 5, 7) or N * sps != K or rows != 1 << N:
        raise ValueError(f"templates float64[{rows}, {K}, 2] are not float64[2^N, N sps, 2] with N odd and 3 .. 7 at sps = {sps}")
    if nbits < 1:
        raise ValueError("nbits must be at least 1")
    if out is None:
        llr, bits = _hip.empty(nbits, "float64"), _hip.empty(nbits, "uint8")
    else:
        llr, bits = out
        if llr.dtype != torch.float64 or bits.dtype != torch.uint8 or not llr.is_contiguous() or not bits.is_contiguous() or \
                llr.numel() != nbits or bits.numel() != nbits:
            raise ValueError(f"out must be (contiguous float64[{nbits}], contiguous uint8[{nbits}])")
    _hip.check(_hip.lib().wf_noncoherent_soft_c128(_ctx(ctx), _hip.ptr(received), n, _hip.ptr(templates), N, sps, int(start), nbits, _hip.ptr(llr),
                                                   _hip.ptr(bits), _hip.stream()))
    return llr, bits


def viterbi_soft_branch(rows, differential: bool = True, warmup: int = 0, ctx=None):
    """``viterbi_soft`` on 48-byte rows with the decided branch of every row (``wf_viterbi4_soft_branch``; include/wfhip.h
    states the definition) -> (llr f64[ncalls], bits u8[ncalls], branch u8[ncalls]) on device.  llr and bits are bitwise
    ``viterbi_soft``'s; branch[k] = 2 start + lsb of the section-k branch of a maximum-likelihood path."""
    ncalls = _rows48(rows)
    llr = _hip.empty(ncalls, "float64")
    bits = _hip.empty(ncalls + 16, "uint8")
    branch = _hip.empty(ncalls + 16, "uint8")
    _hip.check(_hip.lib().wf_viterbi4_soft_branch(_ctx(ctx), _hip.ptr(rows), ncalls, int(bool(differential)), int(warmup),
                                                  _hip.ptr(llr), _hip.ptr(bits), _hip.ptr(branch), _hip.stream()))
    return llr, bits[:ncalls], branch[:ncalls]


def carrier_stat(rows, branch, window: int, out=None, ctx=None):
    """The decision-directed phase statistic per window of ``window`` rows (``wf_carrier_stat``; include/wfhip.h states the
    definition) -> device float64[nwin, 2] = (X_w, Y_w), nwin = ceil(ncalls / window).  ``out``: where to write (a row of the
    H x nwin x 2 table ``carrier_track`` reads)."""
    torch = _hip.torch()
    ncalls = _rows48(rows)
    if branch.dtype != torch.uint8 or not branch.is_contiguous() or branch.numel() != ncalls:
        raise ValueError(f"branch must be {ncalls} contiguous bytes (one per row)")
    nwin = -(-ncalls // int(window))
    out = _stat_out(out, nwin)
    _hip.check(_hip.lib().wf_carrier_stat(_ctx(ctx), _hip.ptr(rows), _hip.ptr(branch), ncalls, int(window), _hip.ptr(out),
                                          _hip.stream()))
    return out


def _track_anchored(c_fn: str, stat, H: int, nwin: int, span: int, period: float, K: int, D: float, rho: float, ctx):
    """``wf_timing_track_anchored`` / ``wf_carrier_track_anchored`` -> (trajectory f64[nwin], choice u8[nwin], drift f64[1],
    marks u8[nwin]), all on the device."""
    traj = _hip.empty(max(nwin, 1), "float64")
    choice = _hip.empty(max(nwin, 1) + 16, "uint8")
    drift = _hip.empty(1, "float64")
    marks = _hip.empty(max(nwin, 1) + 16, "uint8")
    _hip.check(getattr(_hip.lib(), c_fn)(_ctx(ctx), _hip.ptr(stat), H, nwin, int(span), float(period), K, D, rho, _hip.ptr(traj), _hip.ptr(choice),
                                         _hip.ptr(drift), _hip.ptr(marks), _hip.stream()))
    return traj[:nwin], choice[:nwin], drift, marks[:nwin]


def carrier_track(stat, span: int = 1, ctx=None, period=None, anchor: int = 0, max_drift=None, reject=None):
    """Statistics of H hypothesis passes -> (phase f64[nwin], choice u8[nwin]) on device (``wf_carrier_track``; include/wfhip.h
    states the definition).  ``stat``: contiguous device float64[H, nwin, 2], pass h over rows derotated by h π / H.
    ``period``: the symmetry of the trellis in radians in place of π (``wf_carrier_track_mod``: 2π/p for the CPM detectors).
    ``anchor`` = K > 0 (odd, 3 .. 1023): the anchored unwrapping (``wf_carrier_track_anchored``) -> (phase, choice, the drift
    found in radians per window: device f64[1], the rejected windows: device u8[nwin]); ``max_drift`` in radians per window
    (None: 1.25 * 2π ``sync.carrier.MAX_DRIFT_TURNS``), ``reject`` in radians (None: period / 4)."""
    if stat.dtype != _hip.torch().float64 or not stat.is_contiguous() or stat.dim() != 3 or stat.shape[2] != 2:
        raise ValueError("stat must be contiguous float64[H, nwin, 2]")
    H, nwin = int(stat.shape[0]), int(stat.shape[1])
    if int(anchor):
        from .sync import _stages
        from .sync.carrier import MAX_DRIFT_TURNS

        P = math.pi if period is None else float(period)
        K, D, rho = _stages.anchor_args(anchor, max_drift, reject, P, 2.0 * math.pi * MAX_DRIFT_TURNS)
        return _track_anchored("wf_carrier_track_anchored", stat, H, nwin, span, P, K, D, rho, ctx)
    phase = _hip.empty(max(nwin, 1), "float64")
    choice = _hip.empty(max(nwin, 1) + 16, "uint8")
    if period is None:
        _hip.check(_hip.lib().wf_carrier_track(_ctx(ctx), _hip.ptr(stat), H, nwin, int(span), _hip.ptr(phase), _hip.ptr(choice),
                                               _hip.stream()))
    else:
        _hip.check(_hip.lib().wf_carrier_track_mod(_ctx(ctx), _hip.ptr(stat), H, nwin, int(span), float(period), _hip.ptr(phase),
                                                   _hip.ptr(choice), _hip.stream()))
    return phase[:nwin], choice[:nwin]


def carrier_stat_terms(term, window: int, out=None, ctx=None):
    """``carrier_stat`` from the terms ``cpm_soft_branch`` wrote (``wf_carrier_stat_terms``; include/wfhip.h states the
    definition) -> device float64[nwin, 2] = (X_w, Y_w).  ``term``: contiguous device float64[ncalls, 2]."""
    torch = _hip.torch()
    if term.dtype != torch.float64 or not term.is_contiguous() or term.numel() % 2 or term.numel() == 0:
        raise ValueError("term must be contiguous float64[ncalls, 2]")
    ncalls = term.numel() // 2
    nwin = -(-ncalls // int(window))
    out = _stat_out(out, nwin)
    _hip.check(_hip.lib().wf_carrier_stat_terms(_ctx(ctx), _hip.ptr(term), ncalls, int(window), _hip.ptr(out), _hip.stream()))
    return out


def _derotate(c_fn: str, nvals, rows, ncalls: int, window: int, phase, phase0: float, out, ctx):
    """``wf_rows_derotate`` (``nvals`` = (): its rows hold 3 values) or ``wf_rows_derotate_n`` (``nvals`` = (n,)) on checked rows."""
    nwin = _trajectory("phase", phase)
    if out is None:
        out = _hip.empty(tuple(rows.shape), "float64")
    elif out.dtype != _hip.torch().float64 or not out.is_contiguous() or out.numel() != rows.numel():
        raise ValueError("out must be contiguous float64 of the rows' size")
    _hip.check(getattr(_hip.lib(), c_fn)(_ctx(ctx), _hip.ptr(rows), ncalls, *nvals, int(window), _hip.ptr(phase), nwin, float(phase0), _hip.ptr(out),
                                         _hip.stream()))
    return out


def rows_derotate_n(rows, nvals: int, window: int = 64, phase=None, phase0: float = 0.0, out=None, ctx=None):
    """``rows_derotate`` for rows of ``nvals`` complex128 (``wf_rows_derotate_n``; include/wfhip.h states the definition): the
    rows ``cpm_mf_rows`` writes, float64[ncalls, nvals, 2] (ARTM 16, PCM/FM 4).  ``out=rows`` works in place."""
    nvals = int(nvals)
    if not 1 <= nvals <= 64:
        raise ValueError(f"nvals = {nvals} outside 1 .. 64")
    if rows.dtype != _hip.torch().float64 or not rows.is_contiguous() or rows.numel() == 0 or rows.numel() % (2 * nvals):
        raise ValueError(f"rows must be contiguous float64, a whole number of rows of {nvals} complex values")
    return _derotate("wf_rows_derotate_n", (nvals,), rows, rows.numel() // (2 * nvals), window, phase, phase0, out, ctx)


def rows_derotate(rows, window: int = 64, phase=None, phase0: float = 0.0, out=None, ctx=None):
    """48-byte rows times exp(-j (phase0 + φ_k)) (``wf_rows_derotate``; include/wfhip.h states the definition), φ interpolated
    between the centres of the windows of ``window`` rows from ``phase`` (device float64[nwin]; None: φ = 0).  ``out=rows``
    works in place."""
    return _derotate("wf_rows_derotate", (), rows, _rows48(rows), window, phase, phase0, out, ctx)


def rows_derotate_hyp(rows, hypotheses: int, stride: int | None = None, out=None, ctx=None):
    """The ``hypotheses`` rotated copies of 48-byte rows a coarse carrier search detects, in one pass over the rows
    (``wf_rows_derotate_hyp``; include/wfhip.h states the definition) -> device float64[H stride, 3, 2]: copy h at rows h stride ..,
    bitwise ``rows_derotate(rows, phase0=(h * pi) / H)``, then zero rows up to ``stride`` (a multiple of 64, at least the number
    of rows; None: that number rounded up to 64).  Out of place only."""
    torch = _hip.torch()
    ncalls, H = _rows48(rows), int(hypotheses)
    stride = -(-ncalls // 64) * 64 if stride is None else int(stride)
    if not 1 <= H <= 256:
        raise ValueError(f"hypotheses = {hypotheses} outside 1 .. 256")
    if stride < ncalls or stride % 64:
        raise ValueError(f"stride = {stride} must be a multiple of 64 and at least {ncalls}")
    if out is None:
        out = _hip.empty((H * stride, 3, 2), "float64")
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 6 * H * stride:
        raise ValueError(f"out must be contiguous float64[{H * stride}, 3, 2]")
    _hip.check(_hip.lib().wf_rows_derotate_hyp(_ctx(ctx), _hip.ptr(rows), ncalls, H, stride, _hip.ptr(out), _hip.stream()))
    return out


def viterbi_soft_branch_segments(rows, nseg: int, seglen: int, stride: int, differential: bool = True, warmup: int = 0, row_bytes: int = 48,
                                 branch: bool = True, ctx=None):
    """``viterbi_soft_branch`` over ``nseg`` independent trellis segments of one buffer in one set of launches
    (``wf_viterbi4_soft_branch_segments``; include/wfhip.h states the definition) -> (llr f64, bits u8, branch u8), each of
    nseg stride values addressed as the rows are.  Segment s is rows s stride .. s stride + seglen - 1 (``stride`` even, at least
    ``seglen``) and comes out bitwise as ``viterbi_soft_branch`` of those rows alone; the outputs of the pad rows are 0.  ``rows``
    holds (nseg - 1) stride + seglen rows at least.  ``row_bytes=32`` (packed rows) or ``branch=False``: ``viterbi_soft`` per
    segment, and None in place of the branches."""
    nseg, seglen, stride, row_bytes = int(nseg), int(seglen), int(stride), int(row_bytes)
    have = _rows(rows, row_bytes, allow_empty=False)
    if nseg < 1 or seglen < 1 or stride < seglen or stride % 2:
        raise ValueError("nseg and seglen must be at least 1, stride even and at least seglen")
    if have < (nseg - 1) * stride + seglen:
        raise ValueError(f"{have} rows are fewer than the {(nseg - 1) * stride + seglen} that {nseg} segments at stride {stride} take")
    if branch and row_bytes != 48:
        raise ValueError("the branches need 48-byte rows")
    n = nseg * stride
    llr = _hip.empty(n, "float64")
    bits = _hip.empty(n + 16, "uint8")
    br = _hip.empty(n + 16, "uint8") if branch else None
    _hip.check(_hip.lib().wf_viterbi4_soft_branch_segments(_ctx(ctx), _hip.ptr(rows), nseg, seglen, stride, row_bytes, int(bool(differential)),
                                                           int(warmup), _hip.ptr(llr), _hip.ptr(bits), _hip.ptr(br), _hip.stream()))
    return llr, bits[:n], (br[:n] if branch else None)


def timing_offset(signal, tau0: float, eps: float, first_index: int = 0, out=None):
    """The timing impairment at sample rate (``wf_timing_offset_c128``; include/wfhip.h states the definition): the signal read
    at n + tau0 + eps (first_index + n) by cubic Lagrange interpolation, samples outside the burst counting as zero.
    ``signal``: contiguous device float64[n, 2].  Out of place only: ``out`` must not overlap ``signal``."""
    torch = _hip.torch()
    if signal.dtype != torch.float64 or not signal.is_contiguous() or signal.numel() % 2 or signal.numel() == 0:
        raise ValueError("signal must be contiguous float64[n, 2]")
    n = signal.numel() // 2
    if out is None:
        out = _hip.empty((n, 2), "float64")
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != signal.numel():
        raise ValueError("out must be contiguous float64[n, 2]")
    _hip.check(_hip.lib().wf_timing_offset_c128(_hip.ctx(), _hip.ptr(signal), n, float(tau0), float(eps), int(first_index), _hip.ptr(out),
                                                _hip.stream()))
    return out


def mf_bank_resample(received, taps, first: int, step: int, ncols: int, window: int = 64, tau=None, tau0: float = 0.0, out=None, ctx=None):
    """Matched-filter rows at the instants first + k step + tau0 + τ_k (``wf_mf_bank_resample_c128``; include/wfhip.h states the
    definition) -> device float64[ncols, 3, 2].  ``received``: contiguous device float64[nsamp, 2]; ``taps``: float64[3, ntaps, 2],
    ntaps odd; ``tau``: device float64[nwin] in samples, interpolated between the centres of the windows of ``window`` rows as
    ``rows_derotate`` interpolates its phase (None: τ = 0).  ``first`` may be negative and rows may run past the end."""
    torch = _hip.torch()
    if received.dtype != torch.float64 or not received.is_contiguous() or received.numel() % 2 or received.numel() == 0:
        raise ValueError("received must be contiguous float64[nsamp, 2]")
    if taps.dtype != torch.float64 or not taps.is_contiguous() or taps.dim() != 3 or taps.shape[2] != 2:
        raise ValueError("taps must be contiguous float64[3, ntaps, 2]")
    nsamp, ncols = received.numel() // 2, int(ncols)
    nfilt, ntaps = int(taps.shape[0]), int(taps.shape[1])
    nwin = _trajectory("tau", tau)
    if out is None:
        out = _hip.empty((max(ncols, 1), 3, 2), "float64")[:max(ncols, 0)]
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 6 * ncols:
        raise ValueError(f"out must be contiguous float64[{ncols}, 3, 2]")
    _hip.check(_hip.lib().wf_mf_bank_resample_c128(_ctx(ctx), _hip.ptr(received), nsamp, _hip.ptr(taps), nfilt, ntaps, int(first), int(step), ncols,
                                                   int(window), _hip.ptr(tau), nwin, float(tau0), _hip.ptr(out), _hip.stream()))
    return out


def timing_track(stat, period: float, span: int = 1, ctx=None, anchor: int = 0, max_drift=None, reject=None):
    """Statistics of H timing hypotheses -> (tau f64[nwin] in samples, choice u8[nwin]) on device (``wf_timing_track``;
    include/wfhip.h states the definition).  ``stat``: contiguous device float64[H, nwin, 2] as ``carrier_stat`` writes it, pass
    h taken at the instant -period/2 + h period/H; only X is read.  ``anchor`` = K > 0 (odd, 3 .. 1023): the anchored unwrapping
    (``wf_timing_track_anchored``) -> (tau, choice, the drift found in samples per window: device f64[1], the rejected windows:
    device u8[nwin]); ``max_drift`` in samples per window (None: 1.25 ``sync.timing.MAX_DRIFT_SAMPLES``), ``reject`` in samples
    (None: period / 4)."""
    if stat.dtype != _hip.torch().float64 or not stat.is_contiguous() or stat.dim() != 3 or stat.shape[2] != 2:
        raise ValueError("stat must be contiguous float64[H, nwin, 2]")
    H, nwin = int(stat.shape[0]), int(stat.shape[1])
    if int(anchor):
        from .sync import _stages
        from .sync.timing import MAX_DRIFT_SAMPLES

        K, D, rho = _stages.anchor_args(anchor, max_drift, reject, float(period), MAX_DRIFT_SAMPLES)
        return _track_anchored("wf_timing_track_anchored", stat, H, nwin, span, float(period), K, D, rho, ctx)
    tau = _hip.empty(max(nwin, 1), "float64")
    choice = _hip.empty(max(nwin, 1) + 16, "uint8")
    _hip.check(_hip.lib().wf_timing_track(_ctx(ctx), _hip.ptr(stat), H, nwin, int(span), float(period), _hip.ptr(tau), _hip.ptr(choice),
                                          _hip.stream()))
    return tau[:nwin], choice[:nwin]


def timing_refine(stat3, delta: float, span: int = 1, ctx=None):
    """Statistics at τ - δ, τ, τ + δ -> the correction to τ, f64[nwin] in samples, on device (``wf_timing_refine``; include/wfhip.h
    states the definition).  ``stat3``: contiguous device float64[3, nwin, 2]."""
    if stat3.dtype != _hip.torch().float64 or not stat3.is_contiguous() or stat3.dim() != 3 or stat3.shape[0] != 3 or stat3.shape[2] != 2:
        raise ValueError("stat3 must be contiguous float64[3, nwin, 2]")
    nwin = int(stat3.shape[1])
    more = _hip.empty(max(nwin, 1), "float64")
    _hip.check(_hip.lib().wf_timing_refine(_ctx(ctx), _hip.ptr(stat3), nwin, int(span), float(delta), _hip.ptr(more), _hip.stream()))
    return more[:nwin]


def cpm_mf_rows_resample(received, templates, start0: int, sps: int, ncalls: int, window: int = 64, tau=None, tau0: float = 0.0, out=None,
                         ctx=None):
    """``cpm_mf_rows`` at the instants start0 + n sps + tau0 + τ_n (``wf_cpm_mf_rows_resample_c128``; include/wfhip.h states the
    definition) -> device float64[ncalls, nfilt, 2].  ``received``: contiguous device float64[nsamp, 2]; ``templates``:
    float64[nh, nfilt, ntm, 2]; ``tau``: device float64[nwin] in samples, interpolated between the centres of the windows of
    ``window`` rows as ``mf_bank_resample`` interpolates it (None: τ = 0).  Rows may fall before sample 0 or behind the end."""
    torch = _hip.torch()
    if received.dtype != torch.float64 or not received.is_contiguous() or received.numel() % 2 or received.numel() == 0:
        raise ValueError("received must be contiguous float64[nsamp, 2]")
    if templates.dtype != torch.float64 or not templates.is_contiguous() or templates.dim() != 4 or templates.shape[3] != 2:
        raise ValueError("templates must be contiguous float64[nh, nfilt, ntm, 2]")
    nsamp, ncalls = received.numel() // 2, int(ncalls)
    nh, nfilt, ntm = (int(v) for v in templates.shape[:3])
    nwin = _trajectory("tau", tau)
    if out is None:
        out = _hip.empty((max(ncalls, 1), nfilt, 2), "float64")[:max(ncalls, 0)]
    elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 2 * nfilt * ncalls:
        raise ValueError(f"out must be contiguous float64[{ncalls}, {nfilt}, 2]")
    _hip.check(_hip.lib().wf_cpm_mf_rows_resample_c128(_ctx(ctx), _hip.ptr(received), nsamp, _hip.ptr(templates), nh, nfilt, ntm, int(start0),
                                                       int(sps), ncalls, int(window), _hip.ptr(tau), nwin, float(tau0), _hip.ptr(out),
                                                       _hip.stream()))
    return out


def cpm_mf_rows_resample_geometry(nh: int, nfilt: int, ntm: int, sps: int) -> tuple[int, int, int]:
    """(rows per tile, the most workgroups of a launch, bytes of LDS per workgroup) of ``cpm_mf_rows_resample`` for these
    shapes (``wf_cpm_mf_rows_resample_geometry``) - host only."""
    geom = (ctypes.c_int64 * 3)()
    _hip.check(_hip.lib().wf_cpm_mf_rows_resample_geometry(int(nh), int(nfilt), int(ntm), int(sps), geom))
    return int(geom[0]), int(geom[1]), int(geom[2])


def llr_stat(llr, bits_per_call: int, window: int, out=None, ctx=None):
    """The timing statistic of the CPM chains per window of ``window`` calls (``wf_llr_stat``; include/wfhip.h states the
    definition) -> device float64[nwin, 2] = (-Σ |λ|, +0).  ``llr``: contiguous device float64[ncalls bits_per_call] as
    ``cpm_soft`` writes it.  ``out``: where to write (a row of the H x nwin x 2 table ``timing_track`` reads)."""
    torch = _hip.torch()
    bits_per_call = int(bits_per_call)
    if bits_per_call < 1 or llr.dtype != torch.float64 or not llr.is_contiguous() or llr.numel() == 0 or llr.numel() % bits_per_call:
        raise ValueError("llr must be contiguous float64, bits_per_call values for each of at least one call")
    ncalls = llr.numel() // bits_per_call
    nwin = -(-ncalls // int(window))
    out = _stat_out(out, nwin)
    _hip.check(_hip.lib().wf_llr_stat(_ctx(ctx), _hip.ptr(llr), ncalls, bits_per_call, int(window), _hip.ptr(out), _hip.stream()))
    return out


def idd_windows(state, nrows: int, n_tx: int, period: int | None = None, row_offset: int = 1, lock=None, marker_bits: int = 0,
                guard: int = 128, out=None, ctx=None):
    """The live windows of a burst from the decoder's freeze states (``wf_idd_windows``; include/wfhip.h states the definition,
    ``waveforms_amd.encoding.live.windows_host`` restates it) -> device int64[4 + 2 ncw]: W, live rows, open codewords, 0, then
    W pairs (s, e).  ``state``: device u8[ncw], 0 = open.  Codeword b starts at row ``row_offset`` + p̂ + ``marker_bits`` +
    b ``period`` (``period`` default ``n_tx``), p̂ read on the device from ``lock`` (the record of ``frame_search``; None: 0).
    Nothing comes back to the host."""
    torch = _hip.torch()
    period = int(n_tx) if period is None else int(period)
    if int(guard) < 0:
        raise ValueError(f"guard = {guard} must not be negative")
    if int(nrows) < 1 or int(n_tx) < 1 or period < int(n_tx) or int(row_offset) < 0 or int(marker_bits) < 0:
        raise ValueError("nrows and n_tx must be at least 1, period at least n_tx, row_offset and marker_bits not negative")
    if state.dtype != torch.uint8 or state.numel() < 1 or not state.is_contiguous():
        raise ValueError("state must hold ncw contiguous bytes")
    ncw = int(state.numel())
    if out is None:
        out = _hip.empty(4 + 2 * ncw, "int64")
    elif out.dtype != torch.int64 or out.numel() < 4 + 2 * ncw or not out.is_contiguous():
        raise ValueError("out must hold 4 + 2 ncw contiguous int64")
    _hip.check(_hip.lib().wf_idd_windows(_ctx(ctx), _hip.ptr(state), ncw, int(nrows), int(n_tx), period,
                                         int(row_offset), None if lock is None else _hip.ptr(_frame_lock(lock)), int(marker_bits), int(guard),
                                         _hip.ptr(out), _hip.stream()))
    return out


def viterbi_soft_apriori_windows(rows, apriori, windows, apriori_scale: float = 1.0, differential: bool = True, warmup: int = 0,
                                 row_bytes: int = 48, ctx=None, out=None, max_windows: int | None = None):
    """``viterbi_soft_apriori`` on the live windows of a burst only (``wf_viterbi4_soft_apriori_windows``; include/wfhip.h
    states the definition) -> (ext f64[ncalls], bits u8[ncalls]) on device.  ``windows``: the device int64 table of
    ``idd_windows`` (read on the device; ``max_windows`` default: what the table has room for).  Inside a window the result
    is bitwise ``viterbi_soft_apriori`` of the slice; rows outside every window are NOT written: pass ``out`` = (ext, bits) of
    an earlier pass to keep their values (fresh, uninitialised buffers otherwise)."""
    torch = _hip.torch()
    ncalls = _rows(rows, row_bytes, allow_empty=False)
    if apriori is None or apriori.dtype != torch.float32 or not apriori.is_contiguous() or apriori.numel() != ncalls:
        raise ValueError(f"apriori must be {ncalls} contiguous float32 values (one per row)")
    if windows.dtype != torch.int64 or not windows.is_contiguous() or windows.numel() < 6:
        raise ValueError("windows must be the contiguous int64 table idd_windows writes (at least 6 words)")
    room = (windows.numel() - 4) // 2
    max_windows = room if max_windows is None else int(max_windows)
    if not 1 <= max_windows <= room:
        raise ValueError(f"max_windows = {max_windows} outside 1 .. {room} (the table's room)")
    if out is None:
        ext, bits = _hip.empty(ncalls, "float64"), _hip.empty(ncalls + 16, "uint8")
    else:
        ext, bits = out
        if ext.dtype != torch.float64 or not ext.is_contiguous() or ext.numel() < ncalls:
            raise ValueError("out[0] must hold ncalls contiguous float64")
        if bits.dtype != torch.uint8 or not bits.is_contiguous() or bits.numel() < ncalls:
            raise ValueError("out[1] must hold ncalls contiguous bytes")
    _hip.check(_hip.lib().wf_viterbi4_soft_apriori_windows(_ctx(ctx), _hip.ptr(rows), ncalls, int(row_bytes),
                                                           int(bool(differential)), int(warmup), _hip.ptr(apriori), float(apriori_scale),
                                                           _hip.ptr(windows), max_windows, _hip.ptr(ext), _hip.ptr(bits), _hip.stream()))
    return ext[:ncalls], bits[:ncalls]


def cpm_soft(rows, spec, first_call: int = 0, warmup: int = 0, ctx=None, d_rot=None):
    """Max-log-MAP soft output of the generic CPM trellis (``wf_cpm_soft``; include/wfhip.h states the definition) -> (llr
    f64[n lgM], bits u8[n lgM]) on device, one fresh burst.  ``spec``: a full-phase design (NC = p, at most 64 states:
    ``viterbi.cpm.full_phase``, e.g. ARTM_64, PCMFM_20); ``rows``: contiguous device float64[n, M^Lp, 2], the rows
    ``wf_cpm_viterbi_detect`` reads; ``first_call``: the global index of the burst's first call.  λ > 0 favours bit 0, bits
    = λ < 0, bit i (MSB first) of symbol j pairs with λ[lgM j + i].  ``d_rot``: the device rotation table
    (``rotation_table(spec)``) if the caller holds one.  Proof counters as for the hard detectors (viterbi_unmerged /
    viterbi_repaired)."""
    from .viterbi.cpm import rotation_table

    if not rows.is_contiguous():
        raise ValueError("rows must be contiguous")
    per = 2 * spec.nfilt
    if rows.numel() % per:
        raise ValueError(f"{rows.numel()} doubles of rows are not a whole number of {spec.nfilt}-filter rows")
    n, lg = rows.numel() // per, spec.bits_per_symbol
    if d_rot is None:
        d_rot = _hip.to_device(rotation_table(spec))
    llr = _hip.empty(max(n * lg, 1), "float64")
    bits = _hip.empty(n * lg + 16, "uint8")
    cfg = spec.c_config()
    _hip.check(_hip.lib().wf_cpm_soft(_ctx(ctx), ctypes.byref(cfg), _hip.ptr(d_rot), _hip.ptr(rows), n,
                                      int(first_call), int(warmup), _hip.ptr(llr), _hip.ptr(bits), _hip.stream()))
    return llr[:n * lg], bits[:n * lg]


def cpm_soft_branch(rows, spec, first_call: int = 0, warmup: int = 0, ctx=None, d_rot=None, terms: bool = True):
    """``cpm_soft`` with the decided branch of every call and its phase term (``wf_cpm_soft_branch``; include/wfhip.h states
    the definition) -> (llr f64[n lgM], bits u8[n lgM], branch u8[n], term f64[n, 2] or None) on device.  llr and bits are
    bitwise ``cpm_soft``'s; branch[k] = M s* + u* of the section-k branch of a maximum-likelihood path, term[k] = (x, y) of
    q_k on it.  ``d_rot``: the device rotation table; a rotated one (``sync.carrier_cpm.hypothesis_table``) detects the rows
    derotated by its angle.  ``terms=False``: no term is written."""
    from .viterbi.cpm import rotation_table

    if not rows.is_contiguous():
        raise ValueError("rows must be contiguous")
    per = 2 * spec.nfilt
    if rows.numel() % per:
        raise ValueError(f"{rows.numel()} doubles of rows are not a whole number of {spec.nfilt}-filter rows")
    n, lg = rows.numel() // per, spec.bits_per_symbol
    if d_rot is None:
        d_rot = _hip.to_device(rotation_table(spec))
    llr = _hip.empty(max(n * lg, 1), "float64")
    bits = _hip.empty(n * lg + 16, "uint8")
    branch = _hip.empty(n + 16, "uint8")
    term = _hip.empty((max(n, 1), 2), "float64") if terms else None
    cfg = spec.c_config()
    _hip.check(_hip.lib().wf_cpm_soft_branch(_ctx(ctx), ctypes.byref(cfg), _hip.ptr(d_rot), _hip.ptr(rows), n, int(first_call),
                                             int(warmup), _hip.ptr(llr), _hip.ptr(bits), _hip.ptr(branch), _hip.ptr(term),
                                             _hip.stream()))
    return llr[:n * lg], bits[:n * lg], branch[:n], (term[:n] if terms else None)


def cpm_soft_branch_segments(rows, spec, nseg: int, seglen: int, row_stride: int, out_stride: int, d_rot, rot_stride: int = 0,
                             first_call: int = 0, warmup: int = 0, ctx=None, terms: bool = True):
    """``cpm_soft_branch`` over ``nseg`` independent segments in one set of launches (``wf_cpm_soft_branch_segments``;
    include/wfhip.h states the definition) -> (llr f64[nseg out_stride lgM], bits u8[...], branch u8[nseg out_stride], term
    f64[nseg out_stride, 2] or None).  Segment s reads rows s row_stride .. + seglen - 1 of ``rows`` (``row_stride`` 0: every
    segment the same rows) under table s rot_stride of ``d_rot`` (device float64[ntab, 2p, 2]; ``rot_stride`` 0 or 1) and comes
    out at call offset s out_stride bitwise as ``cpm_soft_branch`` of those rows and that table alone; the outputs of the
    calls behind ``seglen`` in each stride are 0.  ``out_stride``: a multiple of 64, at least ``seglen``."""
    nseg, seglen, row_stride, out_stride, rot_stride = int(nseg), int(seglen), int(row_stride), int(out_stride), int(rot_stride)
    if not rows.is_contiguous() or not d_rot.is_contiguous():
        raise ValueError("rows and tables must be contiguous")
    per = 2 * spec.nfilt
    if rows.numel() % per:
        raise ValueError(f"{rows.numel()} doubles of rows are not a whole number of {spec.nfilt}-filter rows")
    if nseg < 1 or seglen < 1 or (row_stride != 0 and row_stride < seglen) or rot_stride not in (0, 1) or out_stride < seglen or out_stride % 64:
        raise ValueError("nseg and seglen must be at least 1, row_stride 0 or at least seglen, rot_stride 0 or 1, out_stride a multiple of 64 and at least seglen")
    need = (nseg - 1) * row_stride + seglen
    if rows.numel() // per < need:
        raise ValueError(f"{rows.numel() // per} rows are fewer than the {need} that {nseg} segments at stride {row_stride} take")
    ntab = (nseg - 1) * rot_stride + 1
    if d_rot.numel() < ntab * 4 * spec.p:
        raise ValueError(f"d_rot holds fewer than {ntab} tables of {2 * spec.p} (cos, sin) pairs")
    n, lg = nseg * out_stride, spec.bits_per_symbol
    llr = _hip.empty(n * lg, "float64")
    bits = _hip.empty(n * lg + 16, "uint8")
    branch = _hip.empty(n + 16, "uint8")
    term = _hip.empty((n, 2), "float64") if terms else None
    cfg = spec.c_config()
    _hip.check(_hip.lib().wf_cpm_soft_branch_segments(_ctx(ctx), ctypes.byref(cfg), _hip.ptr(d_rot), rot_stride, _hip.ptr(rows), nseg, seglen,
                                                      row_stride, out_stride, int(first_call), int(warmup), _hip.ptr(llr), _hip.ptr(bits),
                                                      _hip.ptr(branch), _hip.ptr(term), _hip.stream()))
    return llr, bits[:n * lg], branch[:n], term


def cpm_soft_segments_geometry(spec, nseg: int, seglen: int, warmup: int = 0, ctx=None) -> dict:
    """What ``cpm_soft_branch_segments`` launches for ``nseg`` segments of ``seglen`` calls on this context
    (``wf_cpm_soft_segments_geometry``)."""
    return _geometry("wf_cpm_soft_segments_geometry", ("chunk_calls", "chunks", "warmup", "scratch_bytes", "chunks_per_segment"), _ctx(ctx),
                     ctypes.byref(spec.c_config()), int(nseg), int(seglen), int(warmup))


def cpm_soft_apriori(rows, spec, apriori=None, apriori_scale: float = 1.0, first_call: int = 0, warmup: int = 0, ctx=None, d_rot=None):
    """``cpm_soft`` with a per-bit prior and extrinsic per-bit output (``wf_cpm_soft_apriori``; include/wfhip.h states the
    definition) -> (ext f64[n lgM], bits u8[n lgM]) on device.  ``apriori``: a contiguous device float32 tensor of n lgM
    values indexed as the output is (bit i, MSB first, of call k at [lgM k + i]) or None (= ``cpm_soft``, bitwise);
    π = ``apriori_scale`` * apriori > 0 favours bit 0.  ``ext`` leaves the prior of its own bit out and keeps the one of the
    other bit of the same quaternary symbol (it is what a binary outer decoder is fed); ``bits`` are the decisions of
    ext + π.  Geometry: ``cpm_soft_geometry``."""
    from .viterbi.cpm import rotation_table

    if not rows.is_contiguous():
        raise ValueError("rows must be contiguous")
    per = 2 * spec.nfilt
    if rows.numel() % per:
        raise ValueError(f"{rows.numel()} doubles of rows are not a whole number of {spec.nfilt}-filter rows")
    n, lg = rows.numel() // per, spec.bits_per_symbol
    if not math.isfinite(float(apriori_scale)):
        raise ValueError("apriori_scale must be finite")
    if apriori is not None:
        if apriori.dtype != _hip.torch().float32 or not apriori.is_contiguous() or apriori.numel() != n * lg:
            raise ValueError(f"apriori must be {n * lg} contiguous float32 values ({lg} per call)")
    if d_rot is None:
        d_rot = _hip.to_device(rotation_table(spec))
    ext = _hip.empty(max(n * lg, 1), "float64")
    bits = _hip.empty(n * lg + 16, "uint8")
    cfg = spec.c_config()
    _hip.check(_hip.lib().wf_cpm_soft_apriori(_ctx(ctx), ctypes.byref(cfg), _hip.ptr(d_rot), _hip.ptr(rows), n,
                                              int(first_call), int(warmup), _hip.ptr(apriori), float(apriori_scale), _hip.ptr(ext),
                                              _hip.ptr(bits), _hip.stream()))
    return ext[:n * lg], bits[:n * lg]


def cpm_soft_geometry(spec, ncalls: int, warmup: int = 0, ctx=None) -> dict:
    """What ``cpm_soft`` launches for a burst of ``ncalls`` calls on this context (``wf_cpm_soft_geometry``)."""
    return _geometry("wf_cpm_soft_geometry", ("chunk_calls", "chunks", "warmup", "scratch_bytes"), _ctx(ctx), ctypes.byref(spec.c_config()), int(ncalls), int(warmup))


def viterbi_unmerged(reset: bool = True, ctx=None) -> int:
    """Chunks of the chunk-parallel detectors left UNPROVEN since the last reset (``wf_viterbi4_unmerged``;
    synchronises).  0 = every batch call reproduced the sequential detector bit for bit — which, since chunks
    that miss their warm-up are repaired on the device (cascading into the following chunks where needed), is
    always the case unless the context's WF_OPT_DET_REPAIR option turned the repairs off."""
    n = ctypes.c_int64(0)
    _hip.check(_hip.lib().wf_viterbi4_unmerged(_ctx(ctx), ctypes.byref(n), int(reset), _hip.stream()))
    return int(n.value)


def require_proven(ctx=None, check: bool = False, also=None) -> None:
    """Raise RuntimeError if the chunk-parallel detectors left a chunk unproven on ``ctx`` since the last reset — which only
    a context with the repairs switched off (WF_OPT_DET_REPAIR, tests of the proof itself) can do.  Reads with reset
    (``viterbi_unmerged``; synchronises); ``check``: ``wf_ctx_check`` first (joins a pipelined link's side streams and reads
    the fault word); ``also``: a second context whose count is reset too before raising (the other lane of a stream)."""
    if check:
        _hip.check(_hip.lib().wf_ctx_check(_ctx(ctx), _hip.stream()))
    unproven = viterbi_unmerged(reset=True, ctx=ctx)
    if unproven:
        if also is not None:
            viterbi_unmerged(reset=True, ctx=also)
        raise RuntimeError(f"{unproven} detector chunk(s) were left unproven (the repairs are switched off on this context)")


@contextlib.contextmanager
def proven_carry(carry, ctx):
    """Around a detector launch that advances the device-resident ``carry``: ``require_proven`` behind it, and where that
    raises the carry is what it was before the launch (cloned only on a context that has the repairs switched off: nothing
    else can raise behind a launch), so the caller can run the same rows again."""
    keep = carry.clone() if _hip.get_option(ctx, _hip.WF_OPT_DET_REPAIR) else None
    yield
    try:
        require_proven(ctx)
    except RuntimeError:
        if keep is not None:
            carry.copy_(keep)
        raise


def viterbi_repaired(reset: bool = True, ctx=None) -> int:
    """Chunk repairs the detectors ran on the device since the last reset, every round counted
    (``wf_viterbi_repaired``; synchronises): chunks that missed their warm-up, run again from the true state."""
    n = ctypes.c_int64(0)
    _hip.check(_hip.lib().wf_viterbi_repaired(_ctx(ctx), ctypes.byref(n), int(reset), _hip.stream()))
    return int(n.value)


def viterbi_cascaded(reset: bool = True, ctx=None) -> int:
    """Of those repairs, the ones whose chunk ENDED in a different state than before and therefore handed on to
    the next chunk (``wf_viterbi_cascaded``; synchronises)."""
    n = ctypes.c_int64(0)
    _hip.check(_hip.lib().wf_viterbi_cascaded(_ctx(ctx), ctypes.byref(n), int(reset), _hip.stream()))
    return int(n.value)


def count_errors(det_syms, ref_syms, det_bits, ref_bits, m: int, counts=None):
    """K11: counts[0] += symbol errors, counts[1] += bit errors over the first m elements."""
    if counts is None:
        counts = _hip.zeros(2, "int64")
    _hip.check(_hip.lib().wf_count_errors(_hip.ctx(), _hip.ptr(det_syms), _hip.ptr(ref_syms), _hip.ptr(det_bits),
                                          _hip.ptr(ref_bits), m, _hip.ptr(counts), _hip.stream()))
    return counts


def decimation(size: int, sps: int, length: int, timing_offset: int):
    """(first, ncols) of the samples n in range(size - length*sps) with
    (n + timing_offset) % sps == 0 (reference examples/soqpsk_detection.py:189-192)."""
    limit = size - length * sps
    first = (-timing_offset) % sps
    ncols = (limit - first + sps - 1) // sps if limit > first else 0
    return first, ncols



def cpm_mf_rows(received, templates, start0: int, sps: int, ncalls: int):
    """Generic CPM detector front end -> rows f64[ncalls, nfilt, 2]; templates f64[nh, nfilt, ntm, 2]."""
    nsamp = int(received.shape[0])
    nh, nfilt, ntm = (int(v) for v in templates.shape[:3])
    out = _hip.empty((max(ncalls, 0), nfilt, 2), "float64")
    _hip.check(_hip.lib().wf_cpm_mf_rows_c128(_hip.ctx(), _hip.ptr(received), nsamp, _hip.ptr(templates), nh, nfilt, ntm,
                                              start0, sps, ncalls, _hip.ptr(out), _hip.stream()))
    return out


def cpm_count_errors(decided_u, ref_alpha, M: int, m: int, counts=None):
    """counts[0] += symbol errors, counts[1] += bit errors of decided U against transmitted alpha."""
    if counts is None:
        counts = _hip.zeros(2, "int64")
    _hip.check(_hip.lib().wf_cpm_count_errors(_hip.ctx(), _hip.ptr(decided_u), _hip.ptr(ref_alpha), M, m, _hip.ptr(counts),
                                              _hip.stream()))
    return counts


_WAVE_GEOMETRY = ("codewords_per_wave", "waves", "checkpoint_steps", "lds_bytes", "scratch_bytes")


def _encode(c_fn: str, code, d_info):
    """ncw x k message bits through a ``wf_*_encode`` entry point -> ncw x n_tx transmitted bits."""
    if not d_info.is_contiguous() or d_info.numel() % code.k or d_info.numel() == 0:
        raise ValueError(f"messages must be a contiguous whole number of k = {code.k} bits")
    ncw = d_info.numel() // code.k
    out = _hip.empty((ncw, code.n_tx), "uint8")
    _hip.check(getattr(_hip.lib(), c_fn)(_hip.ctx(), code.handle(), _hip.ptr(d_info), ncw, _hip.ptr(out), _hip.stream()))
    return out


def _codewords(code, d_llr) -> int:
    """ncw of a decoder's input."""
    if not d_llr.is_contiguous() or d_llr.numel() % code.n_tx or d_llr.numel() == 0:
        raise ValueError(f"LLRs must be a contiguous whole number of n_tx = {code.n_tx} values")
    return d_llr.numel() // code.n_tx


def _ext_stride(code, ext_stride) -> int:
    stride = code.n_tx if ext_stride is None else int(ext_stride)
    if stride < code.n_tx:
        raise ValueError(f"ext_stride {stride} is below n_tx = {code.n_tx}")
    return stride


def _ext_room(code, ext, stride: int, ncw: int) -> None:
    if ext.dtype != _hip.torch().float32 or not ext.is_contiguous() or ext.numel() < (ncw - 1) * stride + code.n_tx:
        raise ValueError("ext must be contiguous float32 with room for (ncw - 1) ext_stride + n_tx values")


def _ref_counts(code, ref_info, counts, n: int, ncw: int):
    """The counts a decoder adds to when it has a reference (``counts``, or fresh zeros int64[n]); None without one."""
    if ref_info is None:
        return None
    if ref_info.numel() != ncw * code.k or not ref_info.is_contiguous():
        raise ValueError("ref_info must hold ncw x k contiguous bits")
    return _hip.zeros(n, "int64") if counts is None else counts


def ldpc_encode(code, d_info):
    """LDPC encoder (``wf_ldpc_encode``): device messages (ncw x k bits, u8) -> transmitted bits (ncw x n_tx, u8) in
    transmit order.  ``code``: a :class:`waveforms_amd.encoding.ldpc.LDPCCode`."""
    return _encode("wf_ldpc_encode", code, d_info)


def ldpc_decode(code, d_llr, scale: float = 1.0, alpha: float = 0.75, max_iter: int = 50, ref_info=None, counts=None,
                want_post: bool = False) -> dict:
    """Layered normalized min-sum decoding (``wf_ldpc_decode``; include/wfhip.h states the definition) of ncw codewords:
    ``d_llr`` contiguous float64, codeword b's λ for transmitted position t at [b n_tx + t], λ > 0 favouring bit 0.  Returns
    {"info_bits": u8 ncw x k, "iters": int32 ncw, "post": float32 ncw x n or None, "counts": the int64[4] counts or None}.
    With ``ref_info`` (device ncw x k bits) the decoder ADDS to ``counts`` (fresh zeros if None): information bit errors,
    codewords with an information bit error, codewords not converged, iterations summed."""
    ncw = _codewords(code, d_llr)
    info = _hip.empty((ncw, code.k), "uint8")
    iters = _hip.empty(ncw, "int32")
    post = _hip.torch().empty((ncw, code.n), dtype=_hip.torch().float32, device="cuda") if want_post else None
    counts = _ref_counts(code, ref_info, counts, 4, ncw)
    _hip.check(_hip.lib().wf_ldpc_decode(_hip.ctx(), code.handle(), _hip.ptr(d_llr), ncw, float(scale), float(alpha), int(max_iter),
                                         _hip.ptr(info), _hip.ptr(post), _hip.ptr(iters), _hip.ptr(ref_info), _hip.ptr(counts), _hip.stream()))
    return {"info_bits": info, "iters": iters, "post": post, "counts": counts}


def ldpc_decode_ext(code, d_llr, state, ext, ext_stride: int | None = None, scale: float = 1.0, alpha: float = 0.75, max_iter: int = 5,
                    ext_clip: float = float("inf"), ext_sat: float = 50.0, info_bits=None, iters=None, want_post: bool = False,
                    post=None) -> dict:
    """One outer pass of the decoder in iterative detection and decoding (``wf_ldpc_decode_ext``; include/wfhip.h states the
    definition).  ``d_llr``: contiguous float64, ncw x n_tx, as for ``ldpc_decode``.  ``state``: device u8[ncw], in / out
    (0 open, 1 frozen: such a codeword is not touched).  ``ext``: a device float32 tensor (or a view into a prior buffer)
    that receives codeword b's extrinsic values at [b ext_stride + t] (``ext_stride`` default n_tx).  ``info_bits``
    (u8 ncw x k) and ``iters`` (int32 ncw, INCREASED) are updated in place for the open codewords; fresh zeros when None.
    Returns {"info_bits", "iters", "post" (float32 ncw x n, only open codewords written, or None), "state", "ext"}."""
    torch = _hip.torch()
    ncw = _codewords(code, d_llr)
    stride = _ext_stride(code, ext_stride)
    if state.dtype != torch.uint8 or state.numel() != ncw or not state.is_contiguous():
        raise ValueError("state must hold ncw contiguous bytes")
    _ext_room(code, ext, stride, ncw)
    if info_bits is None:
        info_bits = _hip.zeros((ncw, code.k), "uint8")
    elif info_bits.dtype != torch.uint8 or info_bits.numel() != ncw * code.k or not info_bits.is_contiguous():
        raise ValueError("info_bits must hold ncw x k contiguous bytes")
    if iters is None:
        iters = _hip.zeros(ncw, "int32")
    elif iters.dtype != torch.int32 or iters.numel() != ncw or not iters.is_contiguous():
        raise ValueError("iters must hold ncw contiguous int32")
    if post is None and want_post:
        post = torch.zeros((ncw, code.n), dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().wf_ldpc_decode_ext(_hip.ctx(), code.handle(), _hip.ptr(d_llr), ncw, float(scale), float(alpha), int(max_iter),
                                             _hip.ptr(state), _hip.ptr(info_bits), _hip.ptr(post), _hip.ptr(iters), _hip.ptr(ext), stride,
                                             float(ext_clip), float(ext_sat), _hip.stream()))
    return {"info_bits": info_bits, "iters": iters, "post": post, "state": state, "ext": ext}


def ldpc_count(code, info_bits, ref_info, state, iters, counts=None):
    """``counts`` (device int64[4], fresh zeros if None) += information bit errors, codewords with one, codewords still
    open, iterations summed (``wf_ldpc_count``): the counts of ``ldpc_decode`` after the last ``ldpc_decode_ext`` pass."""
    ncw = int(state.numel())
    if info_bits.numel() != ncw * code.k or ref_info.numel() != ncw * code.k or iters.numel() != ncw:
        raise ValueError("info_bits and ref_info must hold ncw x k bits, iters ncw values")
    if not (info_bits.is_contiguous() and ref_info.is_contiguous() and state.is_contiguous() and iters.is_contiguous()):
        raise ValueError("arguments must be contiguous")
    if counts is None:
        counts = _hip.zeros(4, "int64")
    _hip.check(_hip.lib().wf_ldpc_count(_hip.ctx(), code.handle(), _hip.ptr(info_bits), _hip.ptr(ref_info), _hip.ptr(state), _hip.ptr(iters),
                                        ncw, _hip.ptr(counts), _hip.stream()))
    return counts


def ldpc_decode_geometry(code, ncw: int) -> dict:
    """What ``ldpc_decode`` launches for ``ncw`` codewords (``wf_ldpc_decode_geometry``)."""
    return _geometry("wf_ldpc_decode_geometry", ("state_in_scratch", "codewords_per_workgroup", "workgroups", "lds_bytes", "scratch_bytes"),
                     _hip.ctx(), code.handle(), int(ncw))


def conv_encode(code, d_info):
    """Convolutional encoder (``wf_conv_encode``): device messages (ncw x k bits, u8) -> transmitted bits (ncw x n_tx, u8) in
    transmit order.  ``code``: a :class:`waveforms_amd.encoding.conv.ConvCode`."""
    return _encode("wf_conv_encode", code, d_info)


def conv_siso(code, d_llr, scale: float = 1.0, prior=None, ext=None, ext_stride: int | None = None, ext_clip: float = float("inf"),
              ref_info=None, counts=None, want_bits: bool = True, want_post: bool = True, want_ext: bool = True) -> dict:
    """Exact max-log-MAP decoding (``wf_conv_siso``; include/wfhip.h states the definition) of ncw codewords: ``d_llr``
    contiguous float64, codeword b's λ for transmitted position t at [b n_tx + t], λ > 0 favouring bit 0.  ``prior``: device
    float32 ncw x k (the information bits' prior) or None.  ``ext``: a device float32 tensor (or a view into a prior buffer)
    that receives codeword b's extrinsic values at [b ext_stride + t] (``ext_stride`` default n_tx); None: a fresh ncw x n_tx
    one when ``want_ext``.  Returns {"info_bits": u8 ncw x k, "info_post": float32 ncw x k (Λ), "ext", "counts"}, None for
    what was not asked for.  With ``ref_info`` (device ncw x k bits) the decoder ADDS to ``counts`` (int64[2], fresh zeros if
    None): information bit errors, codewords with any."""
    torch = _hip.torch()
    ncw = _codewords(code, d_llr)
    stride = _ext_stride(code, ext_stride)
    if not float(ext_clip) > 0.0:
        raise ValueError("ext_clip must be positive")
    if prior is not None and (prior.dtype != torch.float32 or not prior.is_contiguous() or prior.numel() != ncw * code.k):
        raise ValueError("prior must hold ncw x k contiguous float32 values")
    if ext is None:
        if want_ext:
            ext = torch.zeros((ncw, stride), dtype=torch.float32, device="cuda")
    else:
        _ext_room(code, ext, stride, ncw)
    counts = _ref_counts(code, ref_info, counts, 2, ncw)
    bits = _hip.empty((ncw, code.k), "uint8") if want_bits else None
    post = torch.empty((ncw, code.k), dtype=torch.float32, device="cuda") if want_post else None
    _hip.check(_hip.lib().wf_conv_siso(_hip.ctx(), code.handle(), _hip.ptr(d_llr), ncw, float(scale), _hip.ptr(prior), _hip.ptr(bits),
                                       _hip.ptr(post), _hip.ptr(ext), stride, float(ext_clip), _hip.ptr(ref_info), _hip.ptr(counts), _hip.stream()))
    return {"info_bits": bits, "info_post": post, "ext": ext, "counts": counts}


def conv_siso_geometry(code, ncw: int) -> dict:
    """What ``conv_siso`` launches for ``ncw`` codewords (``wf_conv_siso_geometry``)."""
    return _geometry("wf_conv_siso_geometry", _WAVE_GEOMETRY, _hip.ctx(), code.handle(), int(ncw))


def turbo_encode(code, d_info):
    """Turbo encoder (``wf_turbo_encode``): device messages (ncw x k bits, u8) -> transmitted bits (ncw x n_tx, u8) in transmit
    order.  ``code``: a :class:`waveforms_amd.encoding.turbo.TurboCode`."""
    return _encode("wf_turbo_encode", code, d_info)


def turbo_decode(code, d_llr, half_iters: int = 12, scale: float = 1.0, ext_scale: float = 0.75, early_stop: bool = True, a1=None,
                 want_a1: bool = False, ext=None, ext_stride: int | None = None, ext_clip: float = float("inf"), ref_info=None, counts=None,
                 want_bits: bool = True, want_post: bool = True, want_iters: bool = True, want_ext: bool = False) -> dict:
    """Max-log-MAP turbo decoding (``wf_turbo_decode``; include/wfhip.h states the definition): ``half_iters`` half-iterations
    of ncw codewords in ONE launch.  ``d_llr`` contiguous float64, codeword b's λ for transmitted position t at [b n_tx + t],
    λ > 0 favouring bit 0.  ``a1``: device float32 ncw x k, constituent 1's prior, read AND left as the last half-iteration
    made it (None: the prior starts as 0; ``want_a1`` then hands a fresh one back).  ``ext``: a device float32 tensor (or a
    view into a prior buffer) that receives codeword b's extrinsic values at [b ext_stride + t] (``half_iters`` even only);
    None: a fresh ncw x n_tx one when ``want_ext``.  Returns {"info_bits": u8 ncw x k, "info_post": float32 ncw x k, "iters":
    int32 ncw, "a1", "ext", "counts"}, None for what was not asked for.  With ``ref_info`` (device ncw x k bits) the decoder
    ADDS to ``counts`` (int64[3], fresh zeros if None): information bit errors, codewords with any, half-iterations run."""
    torch = _hip.torch()
    ncw = _codewords(code, d_llr)
    half_iters = int(half_iters)
    if not 1 <= half_iters <= 64:
        raise ValueError("half_iters must be 1 .. 64")
    stride = _ext_stride(code, ext_stride)
    if not float(ext_clip) > 0.0:
        raise ValueError("ext_clip must be positive")
    if (ext is not None or want_ext) and half_iters % 2:
        raise ValueError("the extrinsic output needs an even half_iters")
    if a1 is not None and (a1.dtype != torch.float32 or not a1.is_contiguous() or a1.numel() != ncw * code.k):
        raise ValueError("a1 must hold ncw x k contiguous float32 values")
    if a1 is None and want_a1:
        a1 = torch.zeros((ncw, code.k), dtype=torch.float32, device="cuda")
    if ext is None:
        if want_ext:
            ext = torch.zeros((ncw, stride), dtype=torch.float32, device="cuda")
    else:
        _ext_room(code, ext, stride, ncw)
    counts = _ref_counts(code, ref_info, counts, 3, ncw)
    bits = _hip.empty((ncw, code.k), "uint8") if want_bits else None
    post = torch.empty((ncw, code.k), dtype=torch.float32, device="cuda") if want_post else None
    iters = torch.empty(ncw, dtype=torch.int32, device="cuda") if want_iters else None
    _hip.check(_hip.lib().wf_turbo_decode(_hip.ctx(), code.handle(), _hip.ptr(d_llr), ncw, float(scale), float(ext_scale), half_iters,
                                          1 if early_stop else 0, _hip.ptr(a1), _hip.ptr(bits), _hip.ptr(post), _hip.ptr(iters), _hip.ptr(ext),
                                          stride, float(ext_clip), _hip.ptr(ref_info), _hip.ptr(counts), _hip.stream()))
    return {"info_bits": bits, "info_post": post, "iters": iters, "a1": a1, "ext": ext, "counts": counts}


def turbo_decode_geometry(code, ncw: int) -> dict:
    """What ``turbo_decode`` launches for ``ncw`` codewords (``wf_turbo_decode_geometry``)."""
    return _geometry("wf_turbo_decode_geometry", _WAVE_GEOMETRY, _hip.ctx(), code.handle(), int(ncw))


def _rs_frames(code, x, per: int, bits: bool, what: str) -> int:
    unit = (8 if bits else 1) * per * code.depth
    if x.dtype != _hip.torch().uint8 or not x.is_contiguous() or x.numel() % unit or x.numel() == 0:
        raise ValueError(f"{what} must be contiguous uint8, a whole number of frames of {unit} bytes")
    return x.numel() // unit


def rs_encode(code, d_msg, bits: bool = False):
    """Reed-Solomon encoder (``wf_rs_encode``): device message frames (F x k I symbols; with ``bits`` one bit per byte, MSB
    first) -> frames (F x n I) in the same form.  ``code``: a :class:`waveforms_amd.encoding.rs.RSCode`."""
    nf = _rs_frames(code, d_msg, code.k, bits, "messages")
    out = _hip.empty((nf, (8 if bits else 1) * code.n * code.depth), "uint8")
    _hip.check(_hip.lib().wf_rs_encode(_hip.ctx(), code.handle(), _hip.ptr(d_msg), nf, int(bool(bits)), _hip.ptr(out), _hip.stream()))
    return out


def rs_decode(code, d_rx, bits: bool = False, ref_msg=None, counts=None, want_status: bool = True, erasures=None) -> dict:
    """Bounded-distance Reed-Solomon decoding (``wf_rs_decode``; include/wfhip.h states the result) of F frames (F x n I
    symbols, or bits) -> {"msg": F x k I in the same form, "status": int32 F I (symbols corrected, -1 = failure), "counts"}.
    With ``ref_msg`` (device message frames) the decoder ADDS to ``counts`` (int64[5], fresh zeros if None): message bit errors,
    codewords wrong, codewords flagged, symbols corrected, frames with a wrong codeword.
    ``erasures``: device uint8 F x n I in SYMBOL form whatever ``bits`` is, nonzero = erased: errors-and-erasures decoding
    (``wf_rs_decode_erasures``); ``counts`` is then int64[6], [5] = erasures filled over the successful codewords."""
    nf = _rs_frames(code, d_rx, code.n, bits, "frames")
    ncount = 5 if erasures is None else 6
    if erasures is not None and _rs_frames(code, erasures, code.n, False, "erasures") != nf:
        raise ValueError("erasures must hold n x depth bytes for every frame")
    if ref_msg is not None:
        if _rs_frames(code, ref_msg, code.k, bits, "ref_msg") != nf:
            raise ValueError("ref_msg must hold as many message frames as there are frames")
        if counts is None:
            counts = _hip.zeros(ncount, "int64")
        elif counts.numel() < ncount:
            raise ValueError(f"counts must hold {ncount} int64 values")
    out = _hip.empty((nf, (8 if bits else 1) * code.k * code.depth), "uint8")
    status = _hip.empty(nf * code.depth, "int32") if want_status else None
    tail = (_hip.ptr(out), _hip.ptr(status), _hip.ptr(ref_msg), _hip.ptr(counts) if ref_msg is not None else None, _hip.stream())
    if erasures is None:
        _hip.check(_hip.lib().wf_rs_decode(_hip.ctx(), code.handle(), _hip.ptr(d_rx), nf, int(bool(bits)), *tail))
    else:
        _hip.check(_hip.lib().wf_rs_decode_erasures(_hip.ctx(), code.handle(), _hip.ptr(d_rx), _hip.ptr(erasures), nf, int(bool(bits)), *tail))
    return {"msg": out, "status": status, "counts": counts if ref_msg is not None else None}


def rs_mark_erasures(code, post, f_max: int, below: float = float("inf")):
    """Erasures from the inner decoder's soft output (``wf_rs_mark_erasures``): ``post`` device float32, F x 8 n I (the Λ of
    ``conv_siso`` for frames in bit form) -> uint8 F x n I, 1 = erased: per codeword the at most ``f_max`` symbols of smallest
    ρ = min |Λ| over the symbol's bits among those with ρ < ``below``, ties to the smaller index.  ``below`` is rounded to float32
    and an infinite one becomes the largest finite float32 (``RSCode.mark_erasures_host`` does the same)."""
    from .encoding.rs import below_f32

    torch = _hip.torch()
    unit = 8 * code.n * code.depth
    if post.dtype != torch.float32 or not post.is_contiguous() or post.numel() % unit or post.numel() == 0:
        raise ValueError(f"post must be contiguous float32, a whole number of frames of {unit} values")
    nf = post.numel() // unit
    out = _hip.empty((nf, code.n * code.depth), "uint8")
    _hip.check(_hip.lib().wf_rs_mark_erasures(_hip.ctx(), code.handle(), _hip.ptr(post), nf, int(f_max), below_f32(below), _hip.ptr(out),
                                              _hip.stream()))
    return out


def rs_decode_geometry(code, nframes: int) -> dict:
    """What ``rs_decode`` launches for ``nframes`` frames (``wf_rs_decode_geometry``)."""
    return _geometry("wf_rs_decode_geometry", ("waves_per_workgroup", "workgroups", "launches", "lds_bytes", "threads_per_workgroup"),
                     _hip.ctx(), code.handle(), int(nframes))


def _frame_pn(pn, n_tx: int):
    torch = _hip.torch()
    if pn is not None and (pn.dtype != torch.uint8 or pn.numel() != n_tx or not pn.is_contiguous()):
        raise ValueError(f"pn must hold n_tx = {n_tx} contiguous bytes")
    return pn


def _frame_lock(lock):
    torch = _hip.torch()
    if lock.dtype != torch.int64 or lock.numel() != 4 or not lock.is_contiguous():
        raise ValueError("lock must be the contiguous int64[4] record frame_search writes")
    return lock


def frame_build(tx, n_tx: int, marker: int, marker_bits: int = 64, pn=None):
    """Transmit side of a framed link (``wf_frame_build``): device coded bits (ncw x n_tx, u8) -> ncw frames of
    ``marker_bits`` marker bits (MSB first) + the codeword exclusive-ored with ``pn`` (device u8[n_tx] or None), u8
    [ncw, marker_bits + n_tx]."""
    if not tx.is_contiguous() or tx.numel() % n_tx or tx.numel() == 0:
        raise ValueError(f"coded bits must be a contiguous whole number of n_tx = {n_tx} bits")
    ncw = tx.numel() // n_tx
    out = _hip.empty((ncw, int(marker_bits) + n_tx), "uint8")
    _hip.check(_hip.lib().wf_frame_build(_hip.ctx(), _hip.ptr(tx), ncw, int(n_tx), int(marker) & (2 ** 64 - 1), int(marker_bits),
                                         _hip.ptr(_frame_pn(pn, n_tx)), _hip.ptr(out), _hip.stream()))
    return out


def frame_search(llr, marker: int, marker_bits: int, period: int, lock=None, want_folded: bool = False):
    """Soft frame search (``wf_frame_search``; include/wfhip.h states the definition) over a burst's λ (contiguous device
    float64; offset the view to align with the detector).  Returns (lock, folded): ``lock`` the device int64[4] record
    { p̂, σ = ±1, best value and best of the others as float64 bit patterns: ``lock[2:].view(torch.float64)`` }, ``folded``
    float64[2, period] (G+ then G-) or None.  Nothing comes back to the host."""
    torch = _hip.torch()
    if llr.dtype != torch.float64 or not llr.is_contiguous():
        raise ValueError("λ must be contiguous float64")
    lock = _hip.empty(4, "int64") if lock is None else _frame_lock(lock)
    folded = _hip.empty((2, int(period)), "float64") if want_folded and period > 0 else None
    _hip.check(_hip.lib().wf_frame_search(_hip.ctx(), _hip.ptr(llr), int(llr.numel()), int(marker) & (2 ** 64 - 1), int(marker_bits), int(period),
                                          _hip.ptr(lock), _hip.ptr(folded), _hip.stream()))
    return lock, folded


def frame_gather(llr, lock, marker_bits: int, n_tx: int, ncw: int, pn=None, out=None):
    """Deframe (``wf_frame_gather``): the ncw x n_tx float64 decoder input of the burst ``llr`` located by ``lock`` (read on
    the device), derandomised by ``pn`` and with the lock's polarity; positions beyond the burst give +0."""
    torch = _hip.torch()
    if llr.dtype != torch.float64 or not llr.is_contiguous() or llr.numel() == 0:
        raise ValueError("λ must be contiguous float64")
    if out is None:
        out = _hip.empty((int(ncw), int(n_tx)), "float64")
    elif out.dtype != torch.float64 or out.numel() != int(ncw) * int(n_tx) or not out.is_contiguous():
        raise ValueError("out must hold ncw x n_tx contiguous float64")
    _hip.check(_hip.lib().wf_frame_gather(_hip.ctx(), _hip.ptr(llr), int(llr.numel()), _hip.ptr(_frame_lock(lock)), int(marker_bits), int(n_tx),
                                          _hip.ptr(_frame_pn(pn, n_tx)), int(ncw), _hip.ptr(out), _hip.stream()))
    return out


def frame_scatter(ext, lock, marker: int, marker_bits: int, n_tx: int, prior, pn=None, marker_prior: float = 0.0,
                  ext_stride: int | None = None):
    """Reframe (``wf_frame_scatter``): the decoder's extrinsic values ``ext`` (device float32, codeword b at [b ext_stride + t],
    ``ext_stride`` default n_tx) into the burst's prior buffer ``prior`` (device float32 view, offset as the search's λ was)
    at the lock's position, randomised by ``pn`` and with the lock's polarity; the marker positions get ±``marker_prior``
    (0: left alone).  In place; returns ``prior``."""
    torch = _hip.torch()
    stride = int(n_tx) if ext_stride is None else int(ext_stride)
    if ext.dtype != torch.float32 or not ext.is_contiguous() or ext.numel() == 0 or stride < n_tx:
        raise ValueError("ext must be contiguous float32 and ext_stride at least n_tx")
    ncw = (ext.numel() - int(n_tx)) // stride + 1
    if prior.dtype != torch.float32 or not prior.is_contiguous() or prior.numel() == 0:
        raise ValueError("prior must be contiguous float32")
    _hip.check(_hip.lib().wf_frame_scatter(_hip.ctx(), _hip.ptr(ext), stride, _hip.ptr(_frame_lock(lock)), int(marker) & (2 ** 64 - 1),
                                           int(marker_bits), int(n_tx), _hip.ptr(_frame_pn(pn, n_tx)), ncw, float(marker_prior), _hip.ptr(prior),
                                           int(prior.numel()), _hip.stream()))
    return prior
