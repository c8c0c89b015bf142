"""tests/golden/link_refusals.json: what the constructors of the four coded link classes (waveforms_amd/encoding/coded.py) answer
to keyword arguments they refuse, recorded at one commit: per case the exception's type and its full message.  No case reaches a
device: every refusal recorded here comes before the link touches one (a case that is not refused fails the recording).
tests/test_link_refusals.py builds the same cases and compares the whole table, so a change of the classes that is meant to move
a check without rewording or reordering it can show that it did.  Names and message texts only.

    python3 tests/golden/make_link_refusals.py        (writes the JSON)

The cases, each for the Coded and the Iterative class, the CPM ones for both waveforms:
  * every refusal the synchroniser link tests (tests/test_{carrier,cpm_carrier,timing,cpm_timing,joint,joint_cpm,coarse}_link.py)
    provoke on a constructor (TESTED);
  * per synchroniser keyword, each of its checks violated alone and every pair of them violated at once, which pins their order
    (SLOTS: the checks in the order the link makes them; a case's name ends in the violated checks);
  * NaN and infinity in each position of ``carrier``, ``timing`` and ``clock``.
"""
import itertools
import json
import math
import sys
from pathlib import Path
from types import SimpleNamespace

OUT = Path(__file__).resolve().parent / "link_refusals.json"
SPS = 8
NOT_REACHED = object()                       # a framing no refusal looks into (the link tests' own stand-in)


def _names():
    from waveforms_amd.encoding import coded, ldpc
    from waveforms_amd.sync import carrier, carrier_cpm, coarse, joint, joint_cpm, timing, timing_cpm
    from waveforms_amd.viterbi import cpm

    return SimpleNamespace(soqpsk=(coded.CodedSOQPSKLink, coded.IterativeSOQPSKLink), cpm=(coded.CodedCPMLink, coded.IterativeCPMLink),
                           code=ldpc.demo_code(), spec={"multih": cpm.ARTM_64, "pcmfm": cpm.PCMFM_20},
                           C=carrier.CarrierRecovery, CC=carrier_cpm.CPMCarrierRecovery, K=coarse.CoarseFrequency, J=joint.JointAcquisition,
                           JC=joint_cpm.CPMJointAcquisition, T=timing.TimingRecovery, TC=timing_cpm.CPMTimingRecovery)


def _other(w: str) -> str:
    return "pcmfm" if w == "multih" else "multih"


# What the link tests provoke: name -> keyword arguments from the names (and, for the CPM classes, the waveform w).
TESTED_SOQPSK = {
    "timing_recovery no framing": lambda n: dict(timing_recovery=n.T(SPS)),
    "timing_recovery beside recovery": lambda n: dict(framing=NOT_REACHED, timing_recovery=n.T(SPS), recovery=n.C()),
    "timing_recovery beside carrier": lambda n: dict(framing=NOT_REACHED, timing_recovery=n.T(SPS), carrier=(0.1, 0.0)),
    "timing_recovery other sps": lambda n: dict(framing=NOT_REACHED, timing_recovery=n.T(10)),
    "timing_recovery a CarrierRecovery": lambda n: dict(framing=NOT_REACHED, timing_recovery=n.C()),
    "acquisition no framing": lambda n: dict(acquisition=n.J(SPS)),
    "acquisition beside recovery": lambda n: dict(framing=NOT_REACHED, acquisition=n.J(SPS), recovery=n.C()),
    "acquisition beside timing_recovery": lambda n: dict(framing=NOT_REACHED, acquisition=n.J(SPS), timing_recovery=n.T(SPS)),
    "acquisition other sps": lambda n: dict(framing=NOT_REACHED, acquisition=n.J(10)),
    "acquisition a TimingRecovery": lambda n: dict(framing=NOT_REACHED, acquisition=n.T(SPS)),
    "coarse alone": lambda n: dict(framing=NOT_REACHED, coarse=n.K(SPS)),
    "coarse beside timing_recovery": lambda n: dict(framing=NOT_REACHED, coarse=n.K(SPS), timing_recovery=n.T(SPS)),
    "coarse other sps": lambda n: dict(framing=NOT_REACHED, coarse=n.K(10), acquisition=n.J(SPS)),
    "coarse a CarrierRecovery": lambda n: dict(framing=NOT_REACHED, coarse=n.C(), acquisition=n.J(SPS)),
    "recovery a CPMCarrierRecovery": lambda n: dict(recovery=n.CC(n.spec["multih"])),
    "recovery no framing": lambda n: dict(recovery=n.C()),
    "keyword clock": lambda n: dict(clock=(0.0, 0.0)),
    "keyword clock_recovery": lambda n: dict(clock_recovery=n.TC(n.spec["pcmfm"], SPS)),
    "keyword joint": lambda n: dict(joint=n.JC(n.spec["pcmfm"], SPS)),
}
TESTED_CPM = {
    "clock_recovery no framing": lambda n, w: dict(clock_recovery=n.TC(n.spec[w], SPS)),
    "clock_recovery beside recovery": lambda n, w: dict(framing=NOT_REACHED, clock_recovery=n.TC(n.spec[w], SPS), recovery=n.CC(n.spec[w])),
    "clock_recovery beside carrier": lambda n, w: dict(framing=NOT_REACHED, clock_recovery=n.TC(n.spec[w], SPS), carrier=(0.1, 0.0)),
    "clock_recovery other sps": lambda n, w: dict(framing=NOT_REACHED, clock_recovery=n.TC(n.spec[w], 10)),
    "clock_recovery a TimingRecovery": lambda n, w: dict(framing=NOT_REACHED, clock_recovery=n.T(SPS)),
    "clock_recovery other design": lambda n, w: dict(framing=NOT_REACHED, clock_recovery=n.TC(n.spec[_other(w)], SPS)),
    "joint no framing": lambda n, w: dict(joint=n.JC(n.spec[w], SPS)),
    "joint beside recovery": lambda n, w: dict(framing=NOT_REACHED, joint=n.JC(n.spec[w], SPS), recovery=n.CC(n.spec[w])),
    "joint beside clock_recovery": lambda n, w: dict(framing=NOT_REACHED, joint=n.JC(n.spec[w], SPS), clock_recovery=n.TC(n.spec[w], SPS)),
    "joint other sps": lambda n, w: dict(framing=NOT_REACHED, joint=n.JC(n.spec[w], 10)),
    "joint a JointAcquisition": lambda n, w: dict(framing=NOT_REACHED, joint=n.J(SPS)),
    "joint a CPMTimingRecovery": lambda n, w: dict(framing=NOT_REACHED, joint=n.TC(n.spec[w], SPS)),
    "joint other design": lambda n, w: dict(framing=NOT_REACHED, joint=n.JC(n.spec[_other(w)], SPS)),
    "recovery a CarrierRecovery": lambda n, w: dict(recovery=n.C()),
    "recovery other design": lambda n, w: dict(recovery=n.CC(n.spec[_other(w)])),
    "keyword timing": lambda n, w: dict(timing=(0.0, 0.0)),
    "keyword timing_recovery": lambda n, w: dict(timing_recovery=n.T(SPS)),
    "keyword acquisition": lambda n, w: dict(acquisition=n.J(SPS)),
    "keyword coarse": lambda n, w: dict(coarse=n.K(SPS)),
}

# Per synchroniser keyword: its checks in the link's order, and the keyword arguments in which the checks in ``bad`` are violated
# and no other.  A wrong class is one that has the attributes the later checks read, so every pair is two real violations.
SLOTS_SOQPSK = {
    "timing_recovery": (("class", "excludes", "sps", "framing"), lambda n, bad: dict(
        timing_recovery=(n.J if "class" in bad else n.T)(10 if "sps" in bad else SPS), framing=None if "framing" in bad else NOT_REACHED,
        **({"carrier": (0.1, 0.0)} if "excludes" in bad else {}))),
    "acquisition": (("class", "excludes", "sps", "framing"), lambda n, bad: dict(
        acquisition=(n.T if "class" in bad else n.J)(10 if "sps" in bad else SPS), framing=None if "framing" in bad else NOT_REACHED,
        **({"timing_recovery": n.T(SPS)} if "excludes" in bad else {}))),
    "coarse": (("class", "excludes", "needs", "sps"), lambda n, bad: dict(
        coarse=(n.T if "class" in bad else n.K)(10 if "sps" in bad else SPS), framing=NOT_REACHED,
        **({"timing_recovery": n.T(SPS)} if "excludes" in bad else {}),
        **({} if "needs" in bad or "excludes" in bad else {"acquisition": n.J(SPS)}))),      # (acquisition excludes timing_recovery itself)
}
SLOTS_CPM = {
    "clock_recovery": (("class", "excludes", "design", "sps", "framing"), lambda n, w, bad: dict(
        clock_recovery=(n.JC if "class" in bad else n.TC)(n.spec[_other(w) if "design" in bad else w], 10 if "sps" in bad else SPS),
        framing=None if "framing" in bad else NOT_REACHED, **({"recovery": n.CC(n.spec[w])} if "excludes" in bad else {}))),
    "joint": (("class", "excludes", "design", "sps", "framing"), lambda n, w, bad: dict(
        joint=(n.TC if "class" in bad else n.JC)(n.spec[_other(w) if "design" in bad else w], 10 if "sps" in bad else SPS),
        framing=None if "framing" in bad else NOT_REACHED, **({"clock_recovery": n.TC(n.spec[w], SPS)} if "excludes" in bad else {}))),
}
NOT_FINITE = {"nan first": (math.nan, 0.0), "nan second": (0.0, math.nan), "inf first": (math.inf, 0.0), "inf second": (0.0, -math.inf)}


def cases(n) -> dict:
    """name -> (class, its positional arguments behind (code, 2), a call that makes its keyword arguments)."""
    out = {}

    def add(name, cls, args, kw):
        name = " ".join((cls.__name__,) + args) + ": " + name
        assert name not in out, name
        out[name] = (cls, args, kw)

    def violated(checks):
        return [bad for r in (1, 2) for bad in itertools.combinations(checks, r)]

    for cls in n.soqpsk:
        for name, kw in TESTED_SOQPSK.items():
            add(name, cls, (), lambda kw=kw: kw(n))
        for slot, (checks, kw) in SLOTS_SOQPSK.items():
            for bad in violated(checks):
                add(f"{slot} violates {' and '.join(bad)}", cls, (), lambda kw=kw, bad=bad: kw(n, bad))
        for pair in ("carrier", "timing"):
            for name, value in NOT_FINITE.items():
                add(f"{pair} {name}", cls, (), lambda pair=pair, value=value: {pair: value})
    for cls, w in itertools.product(n.cpm, n.spec):
        for name, kw in TESTED_CPM.items():
            add(name, cls, (w,), lambda kw=kw, w=w: kw(n, w))
        for slot, (checks, kw) in SLOTS_CPM.items():
            for bad in violated(checks):
                add(f"{slot} violates {' and '.join(bad)}", cls, (w,), lambda kw=kw, w=w, bad=bad: kw(n, w, bad))
        for pair in ("carrier", "clock"):
            for name, value in NOT_FINITE.items():
                add(f"{pair} {name}", cls, (w,), lambda pair=pair, value=value: {pair: value})
    return out


def record() -> dict:
    """name -> [the exception's type, its message] of every case."""
    n, out = _names(), {}
    for name, (cls, args, kw) in cases(n).items():
        try:
            cls(n.code, 2, *args, **kw())
        except (ValueError, TypeError) as e:
            out[name] = [type(e).__name__, str(e)]
        else:
            raise AssertionError(f"{name}: not refused")
    return out


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
    refusals = record()
    OUT.write_text(json.dumps(refusals, indent=0) + "\n")
    print("wrote", OUT, len(refusals), "refusals,", len({tuple(r) for r in refusals.values()}), "distinct")
