"""What the four band-plan creators refuse and what they make, field by field against a recorded table.

sxfir_create_channelizer, sxfir_create_channelizer_os, sxfir_create_synthesizer and sxfir_create_synthesizer_os share one
creation path (create_band_plan, sxfir_plan.hip.h).  tests/golden/band_create.json holds, from the library BEFORE they were
folded into it, the return code and the exact sxfir_last_error() text of every refusal -- with two arguments bad at once too,
which fixes the order of the checks -- and for every accepted creation what the plan then answers.  No stream is processed.

    python tests/test_gpu_band_create.py --record [path]     # writes the table from the library that is importable
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "band_create.json")
CREATORS = ["channelizer", "channelizer_os", "synthesizer", "synthesizer_os"]
FMTS = ["CF32", "CF16", "S32"]

pytestmark = pytest.mark.gpu

# every refusal: name -> the arguments that differ from an accepted call (128 taps, 4 bands, oversample 2, one channel, CF32)
REFUSALS = {
    "null_out": {"out": False},
    "null_taps": {"taps": False},
    "ntaps_0": {"ntaps": 0},
    "nbands_0": {"nbands": 0},
    "nbands_3": {"nbands": 3},
    "nbands_8": {"nbands": 8},
    "ntaps_126": {"ntaps": 126},
    "nchan_0": {"nchan": 0},
    "bad_fmt": {"fmt": 7},
    "nbands_8_ntaps_126": {"nbands": 8, "ntaps": 126},
}
# the two _os creators alone (oversample 2 is the accepted call: code 0, no text)
REFUSALS_OS = {
    "oversample_0": {"oversample": 0},
    "oversample_1": {"oversample": 1},
    "oversample_2": {"oversample": 2},
    "oversample_3": {"oversample": 3},
    "oversample_4097": {"oversample": 4097},
    "oversample_3_nbands_8": {"oversample": 3, "nbands": 8},
}


def refusal_cases(creator):
    return dict(REFUSALS, **REFUSALS_OS) if creator.endswith("_os") else dict(REFUSALS)


def create_raw(creator, out=True, taps=True, ntaps=128, nbands=4, oversample=2, nchan=1, fmt=0):
    """[return code, sxfir_last_error() or None for code 0] of one call of sxfir_create_<creator>; a plan that was made is destroyed."""
    import sxxcvr_amd
    lib = sxxcvr_amd.load_sxfir()
    h = np.zeros(max(ntaps, 1), dtype=np.float32)
    plan = C.c_void_p()
    args = [C.byref(plan) if out else None, h.ctypes.data_as(C.c_void_p) if taps else C.c_void_p(), ntaps, nbands]
    if creator.endswith("_os"):
        args.append(oversample)
    rc = getattr(lib, "sxfir_create_" + creator)(*(args + [nchan, fmt, -1]))
    text = lib.sxfir_last_error().decode() if rc else None
    if plan:
        lib.sxfir_destroy(plan)
    return [rc, text]


def accepted_keys(creator):
    return ["%s/%d/%s/%d" % (creator, ntaps, fmt, nchan) for ntaps in (128, 64) for fmt in FMTS for nchan in (1, 2)]


def accepted(key):
    """What the plan of one accepted creation answers."""
    import sxxcvr_amd
    from sxxcvr_amd.resampler import KERNEL_TILED
    creator, ntaps, fmt, nchan = key.split("/")
    oversample = 2 if creator.endswith("_os") else 1
    if creator.startswith("chan"):
        plan = sxxcvr_amd.Channelizer(sxxcvr_amd.design_lowpass(int(ntaps), 4), 4, nchan=int(nchan), fmt=fmt, oversample=oversample)
    else:
        plan = sxxcvr_amd.Synthesizer(sxxcvr_amd.design_lowpass(int(ntaps), 4, 8.0, 4.0 / oversample), 4, nchan=int(nchan), fmt=fmt,
                                      oversample=oversample)
    try:
        contract = plan.contract
        rot = contract.rot
        return {"bands": plan.bands, "oversampling": plan.oversampling, "ratio": plan.ratio, "contract": list(contract), "rot": rot,
                "outputs_for_1000": plan.outputs_for(1000), "kernel_4096": plan.geometry(4096)["kernel"],
                "set_kernel_tiled": plan._lib.sxfir_set_kernel(plan._plan, KERNEL_TILED)}
    finally:
        plan.close()


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("creator", CREATORS)
def test_refusals_match_recorded(table, creator):
    want = table["refusals"][creator]
    cases = refusal_cases(creator)
    assert sorted(want) == sorted(cases)
    for name, args in cases.items():
        got = create_raw(creator, **args)
        assert got == want[name], "sxfir_create_%s, %s: %r, recorded %r" % (creator, name, got, want[name])


@pytest.mark.parametrize("creator", CREATORS)
def test_accepted_plans_match_recorded(table, creator):
    for key in accepted_keys(creator):
        want, got = table["accepted"][key], accepted(key)
        assert sorted(got) == sorted(want), key
        for field in want:
            assert got[field] == want[field], "%s, %s: %r, recorded %r" % (key, field, got[field], want[field])


def record(path):
    t = {"refusals": {c: {name: create_raw(c, **args) for name, args in refusal_cases(c).items()} for c in CREATORS},
         "accepted": {key: accepted(key) for c in CREATORS for key in accepted_keys(c)}}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n \"refusals\": {\n")
        f.write(",\n".join("  %s: {\n%s\n  }" % (json.dumps(c), ",\n".join("   %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in r.items()))
                           for c, r in t["refusals"].items()))
        f.write("\n },\n \"accepted\": {\n")
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in t["accepted"].items()))
        f.write("\n }\n}\n")
    print("recorded %d refusals, %d accepted creations -> %s" % (sum(len(r) for r in t["refusals"].values()), len(t["accepted"]), path))


if __name__ == "__main__":
    sys.path.append(ROOT)           # (behind PYTHONPATH: the table is recorded from whichever tree is put in front)
    record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
