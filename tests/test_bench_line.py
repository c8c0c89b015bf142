"""bench.py's plain line and --dump-outputs: a plain run carries the headline figure alone (everything else is --full),
and the dumped arrays are the last timed block's decisions and the counts of the timed steps."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FULL_ONLY = ("roofline", "stages", "steady_state", "clock_ramp", "overlapped", "ber_curve", "cpu_baseline", "collective",
             "per_rank_ms_per_step", "scaling_figure")


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def _dumped(d: Path) -> dict:
    out = {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


def test_bench_options_listed():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_line_and_dumped_soqpsk_decisions(tmp_path, oracle):
    """The same timed block (block 0: PRBS from the start, Philox stream 0) after no warm-up and after one: the pipelined link
    holds it in the other set of intermediates then, and both dumps are its decisions — whose errors against the transmitted
    bits and symbols are the counts of the line."""
    nsym = 262144
    lines, dumps = [], []
    for warmup in (0, 1):
        d = tmp_path / f"w{warmup}"
        line = _bench("--steps", "1", "--warmup", str(warmup), "--nsym", str(nsym), "--ebn0", "4", "--dump-outputs", str(d))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line
        assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
        assert not [k for k in FULL_ONLY if k in line]
        lines.append(line)
        dumps.append(_dumped(d))
    assert lines[0]["ber"] == lines[1]["ber"]
    for name in ("error_counts", "decided_bits", "decided_symbols"):
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
    ber, got = lines[0]["ber"], dumps[0]
    m = ber["symbols"]
    assert m == nsym - 3 and got["decided_bits"].shape == got["decided_symbols"].shape == (m,)
    assert got["error_counts"].tolist() == [ber["symbol_errors"], ber["bit_errors"], m]
    bits, _ = oracle.glfsr_bits(0x420000, 0x7FFFFF, nsym)
    sym = oracle.fsm_encode("SOQPSKTrellis4x2DiffEncoded", bits)[0]
    assert int((got["decided_bits"] != bits[:m]).sum()) == ber["bit_errors"] > 0
    assert int((got["decided_symbols"] != sym[:m]).sum()) == ber["symbol_errors"]


@pytest.mark.gpu
def test_dumped_cpm_decisions_are_the_timed_block(tmp_path):
    """The pipelined ARTM link: the timed block's decisions do not depend on how many blocks ran before it."""
    dumps = []
    for warmup in (0, 1):
        d = tmp_path / f"w{warmup}"
        line = _bench("--waveform", "multih", "--steps", "1", "--warmup", str(warmup), "--nsym", "262144", "--ebn0", "4",
                      "--dump-outputs", str(d))
        got = _dumped(d)
        assert got["error_counts"].tolist() == [line["ber"]["symbol_errors"], line["ber"]["bit_errors"], line["ber"]["symbols"]]
        assert got["decided_symbols"].shape == (line["ber"]["symbols"],)
        assert got["decided_symbols"].min() >= 0 and got["decided_symbols"].max() <= 3
        dumps.append(got)
    assert np.array_equal(dumps[0]["decided_symbols"], dumps[1]["decided_symbols"])
    assert dumps[0]["error_counts"].tolist() == dumps[1]["error_counts"].tolist()
