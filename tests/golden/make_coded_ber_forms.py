"""tests/golden/coded_ber_forms.json: what the synchroniser forms of tools/coded_ber.py (``--recover``, ``--recover-timing``,
``--acquire``, each for SOQPSK-TG and for a CPM waveform) print and which ``waveforms_amd.device`` calls they make, recorded at one
commit on two small bursts per point, so that a change of the tool that is meant to change nothing can show that it did.
tests/test_coded_ber_forms.py runs the same command lines with the same runner and asserts equality.

Per case, ``run_case`` loads the tool as a module, sets ``sys.argv``, captures stdout and records

    ``json``     the printed line with every time-valued entry replaced by null (``project``), key order kept
    ``calls``    the names of the ``waveforms_amd.device`` calls of the whole run, in order, as [name, count] runs, repeated
                 blocks of runs folded (``fold``)

The fixture is recorded twice, in two processes.  A float that differs between the two is null in the fixture and its path is
listed under ``"unstable"``; an integer, a string or a call name that differs is refused: that is a finding, not noise.

It also holds what needs no GPU: the exit code and the last stderr line of every ``ap.error`` path of the tool's ``main()``
(``ERRORS``: one command line per path) and the parser's options (option strings, default, nargs, choices, type).

    python3 tests/golden/make_coded_ber_forms.py --commit $(git rev-parse HEAD)    (on an MI355X; records twice, writes the JSON)
    python3 tests/golden/make_coded_ber_forms.py --scan [case ...]                 (prints the lower Eb/N0 each case can use)

Eb/N0 per case are conditions, not measurements: the lower point is the waveform's FER 1e-2 figure of HISTORY.md lowered in
0.5 dB steps until eight codewords leave a codeword error in ``genie`` and in every synchronised curve (``--scan`` does the
lowering; the table holds the value used), the upper point sits 1.5 dB above it.
"""
import argparse
import contextlib
import functools
import importlib.util
import io
import json
import math
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
OUT = HERE / "coded_ber_forms.json"
TOOL = ROOT / "tools" / "coded_ber.py"
SIZES = ["--codewords", "8", "--block-codewords", "4", "--lead-bits", "37", "--steps", "1", "--acq-time-rows", "4000", "--acq-out", ""]
START_DB = {"soqpsk": 5.5, "pcmfm": 3.5, "multih": 8.5}      # where --scan starts: about FER 1e-2 of the forms (HISTORY.md)
UPPER_DB = 1.5
# case -> the lower Eb/N0 in dB (--scan)
LOWER_DB = {
    "carrier_soqpsk": 5.5, "carrier_pcmfm": 3.0, "carrier_coarse_soqpsk": 5.0, "timing_anchor_soqpsk": 5.0, "timing_anchor_pcmfm": 3.0,
    "timing_multih": 7.5, "acquire_anchor_coarse_soqpsk": 5.0, "acquire_anchor_pcmfm": 3.0,
}
TIME_KEYS = ("ms", "ms_per_block", "recovery_ms_per_block", "coarse_ms_per_block", "stages_ms", "in_soft_detections")
# the only floats two recordings of one commit may disagree in (sums taken in another order)
MAY_BE_UNSTABLE = ("coarse_estimates", "nu_error")
# one command line per ap.error path of main(), in the order of the dispatch
ERRORS = {
    "coarse_alone": ["--coarse"],
    "acquire_beside_recover": ["--acquire", "--recover"],
    "timing_offset_alone": ["--timing-offset", "1"],
    "recover_timing_beside_recover": ["--recover-timing", "--recover"],
    "carrier_phase_alone": ["--carrier-phase", "1"],
    "recover_beside_outer": ["--recover", "--outer", "1"],
    "live_only_alone": ["--live-only"],
    "conv_framed": ["--code", "conv-k3", "--framed"],
    "rs_erasures_without_rs": ["--code", "conv-k3", "--rs-erasures", "1"],
    "interleave_without_conv": ["--interleave"],
}


def _impaired(flags: dict) -> list[str]:
    return [v for flag, value in flags.items() for v in (f"--{flag}", repr(float(value)))]


@functools.cache
def cases() -> dict:
    """name -> the case's command line without ``--ebn0``: the form's flags, the impairments of ``make_coded_links._names()`` (the
    synchroniser link tests' values) and ``SIZES``."""
    sys.path.insert(0, str(HERE))
    import make_coded_links

    n = make_coded_links._names()

    def carrier(c):
        return _impaired({"carrier-phase": math.degrees(c[0]), "carrier-freq": c[1]})

    def timing(t):
        return _impaired({"timing-offset": t[0], "timing-drift": t[1]})

    pcmfm, multih = ["--waveform", "pcmfm"], ["--waveform", "multih"]
    coarse = ["--coarse", "--coarse-nfft", "1024"]
    table = {
        "carrier_soqpsk": ["--recover"] + carrier(n.carrier),
        "carrier_pcmfm": pcmfm + ["--recover"] + carrier(n.cpm_carrier("pcmfm")),
        "carrier_coarse_soqpsk": ["--recover"] + coarse + carrier(n.coarse_carrier),
        "timing_anchor_soqpsk": ["--recover-timing", "--anchor", "3"] + timing(n.timing),
        "timing_anchor_pcmfm": pcmfm + ["--recover-timing", "--anchor", "3"] + timing(n.cpm_clock("pcmfm")),
        "timing_multih": multih + ["--recover-timing"] + timing(n.cpm_clock("multih")),
        "acquire_anchor_coarse_soqpsk": ["--acquire", "--anchor", "3"] + coarse + ["--acq-carrier-hyp", "8", "4"] + carrier(n.coarse_joint_carrier)
        + timing(n.joint_timing),
        "acquire_anchor_pcmfm": pcmfm + ["--acquire", "--anchor", "3"] + carrier(n.cpm_joint_carrier("pcmfm")) + timing(n.cpm_joint_clock("pcmfm")),
    }
    assert sorted(table) == sorted(LOWER_DB)
    return {name: argv + SIZES for name, argv in table.items()}


def waveform(argv: list[str]) -> str:
    return argv[argv.index("--waveform") + 1] if "--waveform" in argv else "soqpsk"


def ebn0(name: str, lower: float | None = None) -> list[str]:
    lower = LOWER_DB[name] if lower is None else lower
    return ["--ebn0", repr(lower), repr(lower + UPPER_DB)]


def load_tool():
    spec = importlib.util.spec_from_file_location("coded_ber_tool", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def run_tool(argv: list[str], tool=None):
    """The tool's ``main()`` under ``argv``, in this process -> (stdout, stderr, the SystemExit code or None, the parser)."""
    tool = tool or load_tool()
    seen = []
    parse = argparse.ArgumentParser.parse_args

    def parse_args(self, *a, **kw):
        seen.append(self)
        return parse(self, *a, **kw)

    out, err, code, old = io.StringIO(), io.StringIO(), None, sys.argv
    argparse.ArgumentParser.parse_args, sys.argv = parse_args, ["coded_ber.py"] + list(argv)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            tool.main()
    except SystemExit as e:
        code = e.code
    finally:
        argparse.ArgumentParser.parse_args, sys.argv = parse, old
    return out.getvalue(), err.getvalue(), code, seen[0]


def is_time(key: str) -> bool:
    return key.endswith("_ms") or key in TIME_KEYS


def project(value, timed: bool = False, times: list | None = None):
    """The printed JSON with every value at or under a time-valued key replaced by None, the key order kept; the values taken out
    are appended to ``times``."""
    if isinstance(value, dict):
        return {k: project(v, timed or is_time(k), times) for k, v in value.items()}
    if isinstance(value, list):
        return [project(v, timed, times) for v in value]
    if timed and times is not None:
        times.append(value)
    return None if timed else value


def run_case(name: str, lower: float | None = None) -> dict:
    """One case's command line with every public function of ``waveforms_amd.device`` recorded by name -> {"argv", "json", "calls",
    "times"}; ``times`` are the live values of the entries ``json`` has as null, and are not part of the fixture."""
    from waveforms_amd import device as dev

    argv = cases()[name] + ebn0(name, lower)
    calls = []

    def recorded(fname, fn):
        def call(*args, **kwargs):
            if calls and calls[-1][0] == fname:
                calls[-1][1] += 1
            else:
                calls.append([fname, 1])
            return fn(*args, **kwargs)
        return call

    real = {k: v for k, v in vars(dev).items() if not k.startswith("_") and callable(v) and not isinstance(v, type)}
    try:
        for k, fn in real.items():
            setattr(dev, k, recorded(k, fn))
        out, err, code, _parser = run_tool(argv)
    finally:
        for k, fn in real.items():
            setattr(dev, k, fn)
    assert code is None, (code, err[-2000:])
    (line,) = [ln for ln in out.splitlines() if ln.startswith("{")]
    times = []
    return {"argv": argv, "json": project(json.loads(line), times=times), "calls": calls, "times": times}


def run_error(argv: list[str]) -> dict:
    _out, err, code, _parser = run_tool(argv)
    return {"argv": argv, "exit": code, "stderr": err.strip().splitlines()[-1]}


def options() -> list[dict]:
    """The tool's options as its parser holds them (an ``ap.error`` path: nothing is run)."""
    parser = run_tool(ERRORS["coarse_alone"])[3]
    return [{"flags": a.option_strings, "default": repr(a.default).replace(str(ROOT), "<root>"), "nargs": a.nargs,
             "choices": None if a.choices is None else list(a.choices), "type": None if a.type is None else a.type.__name__, "help": a.help}
            for a in parser._actions if a.option_strings != ["-h", "--help"]]


def curves(point: dict) -> dict:
    return {k: v for k, v in point.items() if isinstance(v, dict) and "codeword_errors" in v}


def errors_show(point: dict) -> bool:
    """A codeword error in ``genie`` and in every synchronised curve of the point."""
    return all(c["codeword_errors"] > 0 for name, c in curves(point).items() if name != "impaired")


def check(records: dict) -> None:
    """The fixture must not pass vacuously: at its lower point every case loses codewords in ``genie`` and in each synchronised
    curve, and ``impaired`` loses at least as many as ``genie`` at both points."""
    for name, rec in records.items():
        lower, upper = rec["json"]["points"]
        assert len(curves(lower)) > 2 and errors_show(lower), f"{name}: a curve without a codeword error at the lower point"
        for p in (lower, upper):
            assert p["impaired"]["codeword_errors"] >= p["genie"]["codeword_errors"], f"{name}: impaired loses less than genie"


def merge(a, b, path: str, unstable: list):
    """Two recordings of one commit -> one: a float that differs becomes None and its path goes to ``unstable``; anything else
    that differs is refused."""
    if isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b):
        return {k: merge(a[k], b[k], f"{path}/{k}", unstable) for k in a}
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [merge(x, y, f"{path}/{i}", unstable) for i, (x, y) in enumerate(zip(a, b))]
    if a == b and type(a) is type(b):
        return a
    if isinstance(a, float) and isinstance(b, float) and any(f"/{k}" in path for k in MAY_BE_UNSTABLE):
        unstable.append(path)
        return None
    raise SystemExit(f"two recordings of one commit differ at {path}: {a!r} against {b!r} - a finding about the commit, not noise")


def drop(value, path: list[str]):
    """``value`` with the entry at ``path`` set to None (what ``merge`` did to an unstable float)."""
    for key in path[:-1]:
        value = value[int(key) if isinstance(value, list) else key]
    value[int(path[-1]) if isinstance(value, list) else path[-1]] = None


def fold(pairs: list) -> list:
    """[name, count] pairs -> the same with every run of equal consecutive blocks as one [[items of the block], repeats]: a form
    makes the same calls burst after burst, and the fixture stays small.  At each position the block (400 pairs at the most) whose
    repeats cover the most pairs is taken; ``unfold`` gives the pairs back."""
    out, i = [], 0
    while i < len(pairs):
        covered, length, repeats = 0, 1, 1
        for n in range(1, min(400, (len(pairs) - i) // 2) + 1):
            r = 1
            while pairs[i + r * n:i + (r + 1) * n] == pairs[i:i + n]:
                r += 1
            if (r - 1) * n > covered:
                covered, length, repeats = (r - 1) * n, n, r
        out.append([fold(pairs[i:i + length]), repeats] if repeats > 1 else pairs[i])
        i += length * repeats
    return out


def unfold(items: list) -> list:
    return [pair for head, count in items for pair in ([[head, count]] if isinstance(head, str) else unfold(head) * count)]


def dumps(fixture: dict) -> str:
    """The fixture as text: one line per entry of a case, per refusal and per option - it is a record, not a text to read."""
    blobs = []

    def line(value) -> str:
        blobs.append(json.dumps(value))
        return f"@{len(blobs) - 1}@"

    text = json.dumps({**fixture, "cases": {name: {k: line(v) for k, v in rec.items()} for name, rec in fixture["cases"].items()},
                       "errors": {name: line(rec) for name, rec in fixture["errors"].items()},
                       "options": [line(option) for option in fixture["options"]]}, indent=1)
    for i, blob in enumerate(blobs):
        text = text.replace(f'"@{i}@"', blob)
    return text + "\n"


def record() -> dict:
    records = {}
    for name in cases():
        rec = run_case(name)
        del rec["times"]
        rec["calls"] = fold(rec["calls"])
        records[name] = rec
        print(name, "recorded", flush=True)
    return {"cases": records, "errors": {name: run_error(argv) for name, argv in ERRORS.items()}, "options": options()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", help="hash of the commit the fixture is recorded at")
    ap.add_argument("--out", type=Path, default=OUT)
    ap.add_argument("--record-to", type=Path, help="record once, in this process, and write the recording there (what --commit starts twice)")
    ap.add_argument("--scan", action="store_true", help="per case: lower the lower Eb/N0 from the waveform's figure in 0.5 dB steps until "
                    "genie and every synchronised curve lose a codeword")
    ap.add_argument("cases", nargs="*", help="with --scan: these cases only")
    args = ap.parse_args()
    if args.scan:
        for name, argv in cases().items():
            if args.cases and name not in args.cases:
                continue
            db = START_DB[waveform(argv)]
            point = run_case(name, db)["json"]["points"][0]
            while not errors_show(point) and db > -5.0:
                db -= 0.5
                point = run_case(name, db)["json"]["points"][0]
            lost = {k: c["codeword_errors"] for k, c in curves(point).items()}
            print(f"{name}: table {LOWER_DB[name]} dB, usable {db} dB, codeword errors {lost}", flush=True)
        return
    if args.record_to:
        args.record_to.write_text(json.dumps(record()))
        return
    if not args.commit:
        ap.error("--commit is needed to write the fixture")
    with tempfile.TemporaryDirectory() as tmp:
        two = []
        for i in range(2):                                       # (one process each: a fresh runtime, a fresh allocator)
            path = Path(tmp) / f"recording{i}.json"
            subprocess.run([sys.executable, str(Path(__file__).resolve()), "--record-to", str(path)], check=True)
            two.append(json.loads(path.read_text()))
    unstable = []
    merged = merge(two[0], two[1], "", unstable)
    check(merged["cases"])
    args.out.write_text(dumps({"commit": args.commit, "unstable": unstable, **merged}))
    print("wrote", args.out, len(merged["cases"]), "cases,", len(unstable), "unstable floats")


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()
