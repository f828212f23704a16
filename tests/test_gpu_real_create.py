"""What sxfir_create and sxfir_create_complex refuse, what an accepted plan answers, and what the profiling build decides
under its knobs, field by field against a recorded table.

tests/golden/real_create.json holds, from the library BEFORE the real-tap and complex-tap creators were rewritten around one
form row per plan: (1) the return code and the exact sxfir_last_error() text of every refusal -- with two arguments bad at once
too, which fixes the order of the checks; (2) for every real-tap and complex-tap shape of tests/test_gpu_launch_table.py, in
every format and with one and two channels, what the plan answers and the text with which a forced tiled kernel refuses a
misaligned output; (3) for the profiling library, under every knob environment the variant and join tests create a plan with
and under the knobs no test sets, the creation's result, the contract and the launch geometry at three call sizes.  No stream
is processed: the only launches are one tiny call per accepted plan.  The geometry depends on the chip's compute-unit count,
which the table stores.

    python tests/test_gpu_real_create.py --record [path]     # writes the table from the library that is importable
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "real_create.json")
FIELDS = ["kernel", "tiled", "split", "tile_samples", "n_tiles", "workgroups", "resident"]
FMTS = ["CF32", "CF16", "S32"]
CREATORS = ["create", "create_complex"]
D, I = 0, 1         # SXFIR_DECIMATE, SXFIR_INTERPOLATE

pytestmark = pytest.mark.gpu

# ---- 1. refusals: name -> the arguments that differ from an accepted call (decimator, 128 taps, ratio 4, one channel, CF32)
REFUSALS = {
    "null_out": {"out": False},
    "null_taps": {"taps": False},
    "mode_2": {"mode": 2},
    "ntaps_0": {"ntaps": 0},
    "ntaps_65537": {"ntaps": 65537},
    "ratio_0": {"ratio": 0},
    "ratio_4097": {"ratio": 4097},
    "nchan_0": {"nchan": 0},
    "nchan_65536": {"nchan": 65536},
    "bad_fmt": {"fmt": 7},
    "interp_remainder": {"mode": I, "ntaps": 130},
    "interpolate": {"mode": I},
    "ntaps_0_ratio_0": {"ntaps": 0, "ratio": 0},
    "bad_fmt_interp_remainder": {"fmt": 7, "mode": I, "ntaps": 130},
    "mode_2_null_taps": {"mode": 2, "taps": False},
}


def create_raw(creator, out=True, taps=True, mode=D, ntaps=128, ratio=4, nchan=1, fmt=0):
    """[return code, sxfir_last_error() or None for code 0] of one call of sxfir_<creator>; a plan that was made is destroyed."""
    import sxxcvr_amd
    lib = sxxcvr_amd.load_sxfir()
    h = np.zeros(2 * max(ntaps, 1), dtype=np.float32)
    plan = C.c_void_p()
    rc = getattr(lib, "sxfir_" + creator)(C.byref(plan) if out else None, mode, h.ctypes.data_as(C.c_void_p) if taps else C.c_void_p(),
                                          ntaps, ratio, nchan, fmt, -1)
    text = lib.sxfir_last_error().decode() if rc else None
    if plan:
        lib.sxfir_destroy(plan)
    return [rc, text]


# ---- 2. accepted product plans
def product_names():
    from test_gpu_launch_table import SHAPE_NAMES
    return [n for n in SHAPE_NAMES if not n.startswith(("chan", "syn"))]


def product_keys(name):
    return ["%s/%s/%d" % (name, fmt, nchan) for fmt in FMTS for nchan in (1, 2)]


def _try_create(*args, **kw):
    """(plan, [0, None]) or (None, [code, text])"""
    import sxxcvr_amd
    try:
        return sxxcvr_amd.Resampler(*args, **kw), [0, None]
    except sxxcvr_amd.NativeError as e:
        return None, [e.code, sxxcvr_amd.load_sxfir(kw.get("profiling", False)).sxfir_last_error().decode()]


def _answer(plan, rc):
    return [rc, plan._lib.sxfir_last_error().decode() if rc else None]


def product_plan(key):
    """What the plan of one product shape answers (a creation that is refused: its code and text alone)."""
    import torch
    from test_gpu_launch_table import shapes
    from sxxcvr_amd.resampler import KERNEL_TILED
    name, fmt, nchan = key.split("/")
    nchan = int(nchan)
    mode, ratio, taps = shapes()[name]
    plan, created = _try_create(mode, taps, ratio, nchan=nchan, fmt=fmt)
    if plan is None:
        return {"create": created}
    try:
        contract = plan.contract
        rot = contract.rot
        out = {"create": created, "contract": list(contract), "rot": rot, "outputs_for_1000": plan.outputs_for(1000)}
        for n in (4096, 1 << 22):
            g = plan.geometry(n)
            out["geometry_%d" % n] = [g["kernel"], g["tiled"]]
        out["set_kernel_tiled"] = _answer(plan, plan._lib.sxfir_set_kernel(plan._plan, KERNEL_TILED))
        # one call of 64 x ratio zero samples into an output that starts one sample behind a 16-byte boundary
        n_in = 64 * ratio
        n_out = plan.outputs_for(n_in)
        sb = 4 if fmt == "CF16" else 8
        x = torch.zeros(nchan * n_in * sb, dtype=torch.uint8, device="cuda")
        y = torch.zeros((nchan * (n_out + 2) + 4) * sb, dtype=torch.uint8, device="cuda")
        assert y.data_ptr() % 16 == 0
        fn = plan._lib.sxfir_decimate if mode == D else plan._lib.sxfir_interpolate
        got = C.c_size_t()
        rc = fn(plan._plan, C.c_void_p(x.data_ptr()), n_in, n_in, C.c_void_p(y.data_ptr() + sb), n_out + 2, C.byref(got),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        out["misaligned_call"] = _answer(plan, rc)
        torch.cuda.synchronize()
        return out
    finally:
        plan.close()


# ---- 3. the profiling library under knobs: (mode, ratio, fmt, nchan, symmetric taps, environment), 32 taps per phase
V, OV, SC = "SXFIR_TILE_VARIANT", "SXFIR_OVERSUB", "SXFIR_SCHED"
_T2 = [(1, 0, "16", "0"), (1, 1, "16", "0"), (1, 2, "64", "2"), (1, 3, "3", "0"), (1, 4, "2", "0"),
       (1, 5, "16", "0"), (1, 6, "1", "2"), (1, 7, "16", "0"), (1, 9, "16", "0"), (1, 11, "7", "0"),
       (2, 0, "16", "0"), (2, 1, "5", "2"), (2, 2, "64", "2"), (2, 3, "16", "0"), (2, 6, "16", "0"),
       (2, 7, "3", "0"), (4, 2, "64", "2"), (4, 3, "16", "0"), (4, 7, "16", "0"), (8, 2, "64", "2"),
       (8, 3, "16", "0"), (1, 16, "16", "0"), (1, 17, "16", "0"), (1, 19, "5", "0"), (2, 17, "16", "0"),
       (2, 19, "64", "0"), (1, 32, "16", "0"), (1, 33, "16", "0"), (2, 35, "16", "0"), (1, 49, "3", "0"),
       (2, 51, "16", "0"), (1, 64, "16", "0"), (1, 65, "16", "0"), (1, 68, "4", "0"), (1, 69, "16", "0"),
       (1, 80, "16", "0"), (1, 81, "7", "0"), (2, 64, "64", "2"), (2, 65, "16", "0"), (4, 65, "16", "0"),
       (16, 192, "1", "0"), (16, 193, "1", "0"), (16, 128, "1", "0"), (8, 192, "1", "0"), (4, 192, "2", "0"),
       (16, 224, "1", "2"), (16, 192, "3", "0")]
# tests/test_gpu_variants.py::test_variant_matches_oracle
_DECIM4 = [{V: "db"}, {V: "db", SC: "1", OV: "1"}, {SC: "1", OV: "1"}, {OV: "3", "SXFIR_OCC": "5"}, {"SXFIR_ABLATE": "3"},
           {V: "sg"}, {V: "sg4"}, {V: "pair"}, {V: "pair", OV: "3"}, {V: "t2:1:320"}, {V: "t2:1:576"}, {V: "t2:1:576", OV: "64"},
           {V: "wide"}, {V: "wide", OV: "3"}, {V: "wident12"}, {V: "wident32", OV: "5"}, {V: "widentp24"}, {V: "widepol200"},
           {V: "widepol310", OV: "5"}, {V: "widepol11"}, {V: "t2s"}, {V: "t2s", OV: "3"}, {V: "t2:1:525376"},
           {V: "t2:1:66624", OV: "64"}, {V: "t2:1:197696"}, {V: "t2:16:66752", OV: "1"}, {V: "wide", OV: "64", SC: "2"},
           {V: "pairx"}, {V: "pairx", OV: "5"}, {V: "pair", OV: "64", SC: "2"}] + \
          [{V: "t2:%d:%d" % (w, o), OV: ov, SC: sc} for (w, o, ov, sc) in _T2]


def _ipass(v, ov=None):
    env = {"SXFIR_IPASS": v[0]}
    if v.endswith("w0"):
        env["SXFIR_IPASS_WAIT0"] = "1"
    if ov:
        env[OV] = ov
    return env


def profile_cases():
    c = [(D, 4, "CF32", 1, True, e) for e in _DECIM4]
    c.append((D, 4, "CF32", 1, True, {V: "t2s", SC: "3", OV: "2"}))                        # test_short_tail_schedule_matches_oracle
    c.append((D, 4, "CF32", 1, True, {"SXFIR_MULTI_PS": "4", V: "mu"}))                    # test_quarter_row_split_variant
    c += [(D, r, fmt, 1, True, {"SXFIR_MULTI_PS": "4"}) for r in (8, 16, 32) for fmt in ("CF32", "CF16")]
    c += [(D, 4, "CF32", 3, True, {V: "t2:16:%d" % o, OV: "1"}) for o in (192, 128)]       # test_cu_queue_variant_multichannel
    c += [(I, 8, "CF32", 2, True, _ipass(v, ov)) for v, ov in
          [("0", "4"), ("1", "1"), ("1", "16"), ("4", "4"), ("4", "1"), ("1w0", "1"), ("1w0", "16")]]
    c += [(I, 4, "CF32", 2, True, _ipass(v, ov)) for v, ov in [("0", "4"), ("0", "16"), ("1", "1"), ("1", "8"), ("1", "16")]]
    c += [(I, r, "CF32", 2, True, _ipass(v, ov)) for r in (16, 32, 48, 96) for v, ov in [("0", "2"), ("1", "1"), ("1", "8"), ("1", "16")]]
    c += [(D, 8, fmt, n, True, {"SXFIR_DENSE_SUBSET": s}) for fmt, ns in (("CF32", (1, 3)), ("S32", (1, 2))) for n in ns for s in "10"]
    c += [(I, 8, "S32", 2, True, _ipass(v)) for v in ("1", "0", "1w0")]
    c += [(D, r, "CF32", 2, True, {"SXFIR_DENSE_HC": "1", OV: ov}) for r, ov in [(32, "8"), (32, "1"), (32, "64"), (16, "8"), (16, "3")]]
    blocks = [(48, "CF32", 1), (96, "CF32", 1), (96, "CF32", 3), (48, "CF16", 2), (96, "S32", 1)]
    c += [(D, r, fmt, n, False, {"SXFIR_BLOCKS_SPLIT": s}) for r, fmt, n in blocks for s in "10"]
    c += [(I, r, fmt, n, False, {"SXFIR_IPASS_SPLIT": s}) for r, fmt, n in [(32, "CF32", 1), (48, "CF32", 2), (96, "CF32", 1), (96, "S32", 1)]
          for s in "10"]
    c += [(D, r, "CF32", 1, False, {"SXFIR_BLOCKS_SPLIT": s, "SXFIR_BLOCKS_RP": rp}) for r, s in [(48, "1"), (96, "1"), (96, "0")] for rp in "01"]
    # tests/test_gpu_join.py: default knobs, the dropped block value, the /4 plan of the load
    c += [(D, r, fmt, n, False, {}) for r, fmt, n in blocks]
    c += [(D, r, "CF32", 1, False, {"SXFIR_BLOCKS_JOIN_DROP": "1"}) for r in (48, 96)]
    c.append((D, 4, "CF32", 1, True, {}))
    # the knobs no test sets
    c += [(D, r, "CF32", 1, True, {"SXFIR_BLOCKS_SMALL": s}) for r in (16, 32) for s in "12"]
    c += [(D, 4, fmt, 1, False, {"SXFIR_WIDE_ASYM": "1"}) for fmt in ("CF32", "S32")]
    c.append((I, 96, "CF32", 1, True, {"SXFIR_IBLOCK16": "1"}))
    c.append((D, 48, "CF32", 1, True, {"SXFIR_BLOCKS_NT": "0"}))
    c.append((D, 4, "CF32", 1, True, {V: "wident24", "SXFIR_LDS_PAD": "16384"}))
    c.append((D, 4, "CF32", 1, True, {V: "mu"}))
    c += [(D, r, fmt, 1, True, {"SXFIR_DENSE": "0"}) for r in (8, 16, 32) for fmt in ("CF32", "CF16")]
    c.append((D, 32, "CF32", 1, True, {"SXFIR_MULTI_W": "8", "SXFIR_MULTI_PS": "4"}))
    c.append((D, 4, "CF32", 1, True, {V: "t2:3:0"}))
    seen, out = set(), []
    for case in c:
        k = profile_key(case)
        if k not in seen:
            seen.add(k)
            out.append(case)
    return out


def profile_key(case):
    mode, ratio, fmt, nchan, sym, env = case
    return "%s%d/%s/%d/%s/%s" % ("decim" if mode == D else "interp", ratio, fmt, nchan, "sym" if sym else "asym",
                                 ",".join("%s=%s" % (k[6:], v) for k, v in sorted(env.items())))


def profile_plan(case):
    """What the profiling library makes of one case: the creation's code and text, the contract, and the geometry rows at
    one tile less one sample, 2^20 and 2^28 input samples."""
    import sxxcvr_amd
    from gpu_util import plan_knobs
    mode, ratio, fmt, nchan, sym, env = case
    taps = np.array(sxxcvr_amd.design_lowpass(32 * ratio, ratio) if mode == D else sxxcvr_amd.design_lowpass(32 * ratio, ratio, 8.0, float(ratio)))
    if not sym:
        taps[3] *= np.float32(1.5)
    with plan_knobs(**env):
        plan, created = _try_create(mode, taps, ratio, nchan=nchan, fmt=fmt, profiling=True)
        if plan is None:
            return {"create": created}
        try:
            contract = plan.contract
            rot = contract.rot
            tile = plan.geometry(1 << 20)["tile_samples"]
            sizes = [(tile if mode == D else tile // ratio) - 1, 1 << 20, 1 << 28]
            return {"create": created, "contract": list(contract), "rot": rot,
                    "rows": [[n] + [plan.geometry(n)[f] for f in FIELDS] for n in sizes]}
        finally:
            plan.close()


def compute_units():
    import sxxcvr_amd
    cu = C.c_int()
    assert sxxcvr_amd.load_sxfir().sxfir_device_info(0, None, None, C.byref(cu), None) == 0
    return cu.value


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        t = json.load(f)
    cu = compute_units()
    if cu != t["compute_units"]:
        pytest.skip("the table was recorded on a device with %d compute units, this one has %d" % (t["compute_units"], cu))
    return t


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for field in want:
        assert got[field] == want[field], "%s, %s: %r, recorded %r" % (what, field, got[field], want[field])


@pytest.mark.parametrize("creator", CREATORS)
def test_refusals_match_recorded(table, creator):
    want = table["refusals"][creator]
    assert sorted(want) == sorted(REFUSALS)
    for name, args in REFUSALS.items():
        got = create_raw(creator, **args)
        assert got == want[name], "sxfir_%s, %s: %r, recorded %r" % (creator, name, got, want[name])


@pytest.mark.parametrize("name", ["decim%d" % r for r in (4, 8, 16, 32, 48, 96)] + ["interp%d" % r for r in (4, 8, 16, 32, 48, 96)] +
                         ["decim4x64", "decim4asym", "decim5x40", "interp5x40", "cx4x128", "cx8x256"])
def test_product_plans_match_recorded(table, name):
    assert name in product_names()
    for key in product_keys(name):
        _same(json.loads(json.dumps(product_plan(key))), table["product"][key], key)


def test_every_product_shape_is_recorded(table):
    assert sorted(table["product"]) == sorted(k for n in product_names() for k in product_keys(n))
    assert sorted(table["profiling"]) == sorted(profile_key(c) for c in profile_cases())


@pytest.mark.parametrize("case", profile_cases(), ids=profile_key)
def test_profiling_knobs_match_recorded(table, case):
    key = profile_key(case)
    _same(json.loads(json.dumps(profile_plan(case))), table["profiling"][key], key)


def record(path):
    t = {"compute_units": compute_units(), "fields": ["n_in"] + FIELDS,
         "refusals": {c: {name: create_raw(c, **args) for name, args in REFUSALS.items()} for c in CREATORS},
         "product": {key: product_plan(key) for name in product_names() for key in product_keys(name)},
         "profiling": {profile_key(case): profile_plan(case) for case in profile_cases()}}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def rows(d, indent):
        return ",\n".join("%s%s: %s" % (indent, json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in d.items())
    with open(path, "w") as f:
        f.write("{\n \"compute_units\": %d,\n \"fields\": %s,\n \"refusals\": {\n" % (t["compute_units"], json.dumps(t["fields"])))
        f.write(",\n".join("  %s: {\n%s\n  }" % (json.dumps(c), rows(r, "   ")) for c, r in t["refusals"].items()))
        f.write("\n },\n \"product\": {\n%s\n },\n \"profiling\": {\n%s\n }\n}\n" % (rows(t["product"], "  "), rows(t["profiling"], "  ")))
    print("recorded %d refusals, %d product plans, %d profiling cases, %d compute units -> %s" % (
        sum(len(r) for r in t["refusals"].values()), len(t["product"]), len(t["profiling"]), t["compute_units"], path))


if __name__ == "__main__":
    sys.path.append(ROOT)           # (behind PYTHONPATH: the table is recorded from whichever tree is put in front)
    record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
