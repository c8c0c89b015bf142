"""tests/golden/link_geometry.json: what the host halves of the uncoded links answer, recorded once.  "geometry": the geometry
entry points of the SOQPSK and CPM links and their streams over a sweep of configurations, as [configuration, the answers of
the calls made with it].  "refusals": every refusal the run and stream-chunk entry points give before they touch a device,
on a zeroed fake context, as [function, case, return code, wf_last_error_string()].  None of it needs a GPU.
tests/test_link_geometry.py replays ``geometry()`` and ``refusals()`` and compares every entry, so a change of the host code
that is meant to move a computation or a check without changing it can show that it did.  Names, integers and message texts only.

    python3 tests/golden/make_link_geometry.py        (writes the JSON)
"""
import ctypes
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "link_geometry.json"
P = ctypes.c_void_p


def _chunk_indices(calls: int, B: int) -> list:
    """0, 1, a middle one, the last, one past the last."""
    n = max(-(-calls // B), 1)
    return sorted({0, 1, n // 2, n - 1, n})


def _soqpsk_cfg(_hip, nsym, sps, mf_ntaps, fuse, timing_offset, table=0x10000):
    cfg = _hip.LinkConfig()
    cfg.nsym, cfg.sps, cfg.degree, cfg.mask, cfg.state = nsym, sps, 23, 0x420000, 0x7FFFFF
    cfg.differential, cfg.ntaps, cfg.mf_ntaps, cfg.mf_nfilt = 1, 8 * sps + 1, mf_ntaps, 3        # (the SOQPSK-TG pulse: 8 symbols)
    cfg.d_h = cfg.d_pulse = cfg.d_mf_taps = table
    cfg.timing_offset, cfg.fuse, cfg.event_slot, cfg.seed = timing_offset, fuse, -1, 1
    return cfg


def _cpm_cfg(_hip, spec, nsym, fuse, sps=8, table=0x10000):
    cfg = _hip.CPMLinkConfig()
    cfg.nsym, cfg.sps, cfg.degree, cfg.mask, cfg.state = nsym, sps, 23, 0x420000, 0x7FFFFF
    cfg.mapper_kind, cfg.det = (1 if spec.M == 4 else 2), spec.c_config()
    if spec.M == 4:
        from waveforms_amd.cpm.multih import freq_pulse_multih_irig as pulse
    else:
        from waveforms_amd.cpm.pcmfm import freq_pulse_pcmfm as pulse
    cfg.ntaps = int(pulse(sps).size)
    cfg.d_h = cfg.d_pulse = cfg.d_templates = cfg.d_rot_cs = table
    cfg.skip_head, cfg.event_slot, cfg.fuse, cfg.seed = 64, -1, fuse, 1
    return cfg


def geometry() -> list:
    """[configuration, the answers of every geometry call made with it, in the order of the calls]: a byte count, an
    interior flag, or the eight layout words (a refused layout: its return code alone)."""
    from waveforms_amd import _hip
    from waveforms_amd.viterbi import cpm

    lib, out = _hip.lib(), []

    def words(got, fn, *args):
        info = (ctypes.c_int64 * 8)(*([-7] * 8))          # (a word the call leaves alone stays -7)
        rc = fn(*args, info)
        got.append(list(info) if rc == 0 else rc)
        return info

    for sps in (4, 8, 10, 20):
        for mf_ntaps in (sps + 1, 73):
            for fuse in (0, 7, 15, 31, 47):
                for off in (-1, 0, -5):
                    for nsym in (1, 100, 4096, 300_001, 9 * 65536 + 777):
                        cfg = _soqpsk_cfg(_hip, nsym, sps, mf_ntaps, fuse, off)
                        r, got = ctypes.byref(cfg), [lib.wf_link_workspace_bytes(ctypes.byref(cfg))]
                        calls = words(got, lib.wf_link_layout, r)[0]
                        for B in (1000, 5120, 65536):
                            got.append(lib.wf_link_stream_workspace_bytes(r, B))
                            for c in _chunk_indices(calls, B):
                                words(got, lib.wf_link_stream_layout, r, B, c)
                                got.append(lib.wf_link_stream_interior(r, B, c))
                        out.append([f"soqpsk sps{sps} taps{mf_ntaps} fuse{fuse} off{off} n{nsym}", got])
    for name in ("ARTM_16", "ARTM_64", "ARTM_256", "PCMFM_10"):
        for base in (10, 42, 10 | 128, 42 | 128):
            for fuse in (base, base | 64):
                for nsym in (100, 40_961, 2 * (3 << 20) + 1_200_000):
                    cfg = _cpm_cfg(_hip, getattr(cpm, name), nsym, fuse)
                    r, got = ctypes.byref(cfg), [lib.wf_cpm_link_workspace_bytes(ctypes.byref(cfg))]
                    calls = words(got, lib.wf_cpm_link_layout, r)[0]
                    for B in (1000, 5120, 3 << 20):
                        got.append(lib.wf_cpm_link_stream_workspace_bytes(r, B))
                        for c in _chunk_indices(calls, B):
                            words(got, lib.wf_cpm_link_stream_layout, r, B, c)
                    out.append([f"{name} fuse{fuse} n{nsym}", got])
    return out


def refusals() -> list:
    """Every call here must be refused by an argument check: one that passed them all would go on to the device."""
    from waveforms_amd import _hip
    from waveforms_amd.viterbi import cpm

    lib, out = _hip.lib(), []
    fake = ctypes.create_string_buffer(1 << 16)           # a zeroed wf_ctx: no device exists here
    ctx = ctypes.cast(fake, P)
    ws, st, cnt = P(0x7F0000001000), P(0x7F0000000100), P(0x7F0000000200)     # never dereferenced on the host
    m = ctypes.c_int64(0)

    def refused(fn, case, *args):
        rc = getattr(lib, fn)(*args)
        assert rc < 0, (fn, case, rc)
        out.append([fn, case, rc, lib.wf_last_error_string().decode()])

    # ---- one-shot links: (ctx, cfg, workspace, workspace_bytes, counts, compared, stream)
    links = (("wf_link_run", lambda **k: _soqpsk_cfg(_hip, 40_000, 8, 9, k.get("fuse", 15), -1, table=k.get("table", 0x10000)),
              lib.wf_link_workspace_bytes, 47),
             ("wf_cpm_link_run", lambda **k: _cpm_cfg(_hip, cpm.ARTM_16, 40_000, k.get("fuse", 10), table=k.get("table", 0x10000)),
              lib.wf_cpm_link_workspace_bytes, 42))
    for fn, make, nbytes, piped_fuse in links:
        cfg = make()
        r, n = ctypes.byref(cfg), nbytes(ctypes.byref(cfg))
        refused(fn, "NULL ctx", None, r, ws, n, cnt, ctypes.byref(m), None)
        refused(fn, "NULL cfg", ctx, None, ws, n, cnt, ctypes.byref(m), None)
        refused(fn, "NULL workspace", ctx, r, None, n, cnt, ctypes.byref(m), None)
        refused(fn, "NULL counts", ctx, r, ws, n, None, ctypes.byref(m), None)
        bad = make()
        bad.nsym = 0
        refused(fn, "nsym 0", ctx, ctypes.byref(bad), ws, n, cnt, ctypes.byref(m), None)
        refused(fn, "workspace off alignment", ctx, r, P(ws.value + 128), n, cnt, ctypes.byref(m), None)
        refused(fn, "workspace too small", ctx, r, ws, n - 1, cnt, ctypes.byref(m), None)
        refused(fn, "workspace of 0 bytes", ctx, r, ws, 0, cnt, ctypes.byref(m), None)
        piped = make(fuse=piped_fuse)
        two = nbytes(ctypes.byref(piped))
        assert two >= 2 * n
        refused(fn, "fuse bit 5, one set", ctx, ctypes.byref(piped), ws, n, cnt, ctypes.byref(m), None)
        refused(fn, "fuse bit 5, between one and two sets", ctx, ctypes.byref(piped), ws, two - 1, cnt, ctypes.byref(m), None)
        for slot in (64, 1 << 20):
            cfg.event_slot = slot
            refused(fn, f"event_slot {slot}", ctx, r, ws, n, cnt, ctypes.byref(m), None)
        cfg.event_slot = -1
    refused("wf_cpm_link_run", "NULL tables", ctx, ctypes.byref(links[1][1](table=None)), ws, 1 << 30, cnt, ctypes.byref(m), None)
    short = _soqpsk_cfg(_hip, 1, 8, 73, 15, -1)
    short.ntaps = 1
    refused("wf_link_run", "burst shorter than the bank", ctx, ctypes.byref(short), ws, 1 << 30, cnt, ctypes.byref(m), None)

    # ---- stream chunks: (ctx, cfg, chunk, index, state, workspace, workspace_bytes, counts, compared, [phases,] stream)
    B = 5120
    scfg, ccfg = _soqpsk_cfg(_hip, 300_001, 8, 9, 15, -1), _cpm_cfg(_hip, cpm.ARTM_16, 300_001, 10 | 64)
    streams = (("wf_link_stream_chunk", scfg, lib.wf_link_stream_workspace_bytes, (), True),
               ("wf_link_stream_chunk_phase", scfg, lib.wf_link_stream_workspace_bytes, (7,), True),
               ("wf_link_stream_steady", scfg, lib.wf_link_stream_workspace_bytes, (), False),
               ("wf_cpm_link_stream_chunk", ccfg, lib.wf_cpm_link_stream_workspace_bytes, (), True),
               ("wf_cpm_link_stream_chunk_phase", ccfg, lib.wf_cpm_link_stream_workspace_bytes, (7,), True))
    for fn, cfg, nbytes, ph, indexed in streams:
        r, n = ctypes.byref(cfg), nbytes(ctypes.byref(cfg), B)
        assert n > 0

        def call(case, cx=ctx, rr=r, chunk=B, c=1, state=st, w=ws, nb=n, counts=cnt, phases=ph):
            refused(fn, case, cx, rr, chunk, *((c,) if indexed else ()), state, w, nb, counts, ctypes.byref(m), *phases, None)

        call("NULL ctx", cx=None)
        call("NULL cfg", rr=None)
        call("NULL state", state=None)
        call("NULL workspace", w=None)
        call("NULL counts", counts=None)
        call("workspace off alignment", w=P(ws.value + 128))
        call("state off alignment", state=P(st.value + 8))
        call("workspace too small", nb=n - 1)
        for chunk in (0, -5120, 1000, 5000, 128, 5120 + 64):
            assert nbytes(r, chunk) < 0                  # (the geometry refuses the size: the call cannot get past its checks)
            call(f"chunk size {chunk}", chunk=chunk)
        if indexed:
            call("chunk index -1", c=-1)
        if ph:
            for phases in (0, 8, -1):
                call(f"phases {phases}", phases=(phases,))
    short = _soqpsk_cfg(_hip, 5120 + 600, 8, 9, 15, -1)                # (a stream of two chunks: no interior one)
    refused("wf_link_stream_steady", "no interior chunk", ctx, ctypes.byref(short), B, st, ws, 1 << 30, cnt, ctypes.byref(m), None)
    unfused = _soqpsk_cfg(_hip, 300_001, 8, 9, 0, -1)
    refused("wf_link_stream_steady", "no fused channel", ctx, ctypes.byref(unfused), B, st, ws, 1 << 30, cnt, ctypes.byref(m), None)
    nul = _cpm_cfg(_hip, cpm.ARTM_16, 300_001, 10 | 64, table=None)
    refused("wf_cpm_link_stream_chunk", "NULL tables", ctx, ctypes.byref(nul), B, 1, st, ws, 1 << 30, cnt, ctypes.byref(m), None)

    # ---- stage times: (ctx, event_slot, ms)
    ms = (ctypes.c_float * 8)()
    refused("wf_link_stage_ms", "NULL ctx", None, 0, ms)
    refused("wf_link_stage_ms", "NULL output", ctx, 0, None)
    for slot in (-1, 64, 0):
        refused("wf_link_stage_ms", f"event_slot {slot}, nothing recorded", ctx, slot, ms)
    return out


def record() -> dict:
    return {"geometry": geometry(), "refusals": refusals()}


if __name__ == "__main__":
    here = Path(__file__).resolve().parent
    sys.path[:0] = [str(here.parent.parent)]
    got = record()
    OUT.write_text(json.dumps(got, separators=(",", ":")).replace("],[\"", "],\n[\"") + "\n")
    print("wrote", OUT, len(got["geometry"]), "configurations,", sum(len(g[1]) for g in got["geometry"]), "geometry answers,", len(got["refusals"]), "refusals,", OUT.stat().st_size, "bytes")
