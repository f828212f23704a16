"""The (tile, block) join of the decimators by 48 and 96: decim_blocks_kernel<..., SPLIT> is the one path of the project in which
workgroups hand values to each other through HBM -- sc1 stores, a barrier, one relaxed device-scope add per item, sc1 loads by the
tile's last arriver; no release, no acquire, two workgroups per CU where the microarchitecture guide's table row was measured at
one.  Every readStream pass at the two slowest rates runs it.

What these tests can see that the streamed comparisons of test_gpu_variants.py cannot: a block value left by an EARLIER launch
(different inputs in turn, the scratch poisoned with NaNs before every launch), an output that was never stored (NaN prefill),
the arrival counters' return to zero across back-to-back launches with no host synchronisation in between, call sizes that change
what a scratch slot means, and an unevenly loaded chip (a /4 plan of varying call size on a second stream).  Every output word of
every launch is compared on the GPU with the walking form's bits (another kernel instance, for CF32 itself checked against the CPU
oracle under the contract the plan reports).  test_join_checker_sees_a_dropped_block_value proves that this checker reports a
hand-off that did not arrive -- as a NaN with the poison, as the previous launch's value without.

Shapes: the smallest at which the join can go wrong.  "small" = 64 tiles per channel (one wave of workgroups: a tile's items sit in
different workgroups and, dealt round-robin, on different XCDs); "rounds" = 3 x resident + 5 tiles over all channels (items
outnumber the slots several times: joiners and producers of different tiles are resident together); the last tile ragged
(outputs = 76 mod 512)."""
import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd.resampler import DECIMATE, KERNEL_TILED
from gpu_util import JoinSoak, OUT_FILL, TILE_OUT, assert_bit_exact, join_taps, plan_knobs, to_cpu

pytestmark = pytest.mark.gpu

LAUNCHES = 500
SMALL = 63 * TILE_OUT + 76


def _plan(D, fmt="CF32", nchan=1, profiling=True, **knobs):
    with plan_knobs(**knobs):
        plan = sxxcvr_amd.Resampler(DECIMATE, join_taps(D), D, nchan=nchan, fmt=fmt, profiling=profiling)
    plan.set_kernel(KERNEL_TILED)
    return plan


def _rounds_outputs(D, nchan=1):
    """Outputs per channel of the "several rounds" call: 3 x resident + 5 tiles over all channels, the last one ragged."""
    plan = _plan(D, nchan=nchan)
    resident = plan.geometry(D * SMALL)["resident"]
    plan.close()
    tiles = -(-(3 * resident + 5) // nchan)
    return (tiles - 1) * TILE_OUT + 76


_cases = {}


def _case(oracle, D, fmt, nchan, size):
    """Inputs and references of a case: made once, shared by the tests that soak it, never written afterwards."""
    key = (D, fmt, nchan, size)
    if key not in _cases:
        _cases.clear()                       # (one case's buffers at a time: the large ones are 0.6 GB)
        _cases[key] = JoinSoak(D, fmt, nchan, SMALL if size == "small" else _rounds_outputs(D, nchan), oracle=oracle)
    return _cases[key]


@pytest.mark.parametrize("D,fmt,nchan,size", [(48, "CF32", 1, "small"), (96, "CF32", 1, "small"), (96, "CF32", 3, "small"),
                                              (48, "CF16", 2, "small"), (96, "S32", 1, "small"),
                                              (48, "CF32", 1, "rounds"), (96, "CF32", 1, "rounds")])
def test_split_join_fresh_data_poisoned_scratch(oracle, D, fmt, nchan, size):
    """The profiling library with default knobs: 500 launches on an idle chip and 500 beside the load, three inputs in turn, the
    scratch poisoned before every launch, every 7th launch another call size, no host synchronisation inside the loop: no output word
    differs from the walking form's, and every arrival counter is zero at the end."""
    case = _case(oracle, D, fmt, nchan, size)
    if fmt == "CF32":
        assert case.oracle_outputs >= (SMALL if size == "small" else 4 * 3000) * nchan * 3
    plan = _plan(D, fmt, nchan)
    for load in (False, True):
        res = case.run(plan, LAUNCHES, poison=True, load=load)
        print("/%d %s %d ch %s load=%s: %s" % (D, fmt, nchan, size, load, res))
        assert res["launches"] >= LAUNCHES
        assert res["bad_words"] == 0, res
        assert res["counters"] == 0, res
    plan.close()


@pytest.mark.parametrize("D", [48, 96])
def test_split_join_product_library_fresh_data(oracle, D):
    """The shipped libsxfir.so -- what the Device runs; no hooks, so no poison: inputs in turn, mixed call sizes, beside the load,
    back to back."""
    case = _case(oracle, D, "CF32", 1, "small")
    plan = _plan(D, profiling=False)
    res = case.run(plan, LAUNCHES, poison=False, load=True)
    print("/%d product library: %s" % (D, res))
    assert res["launches"] >= LAUNCHES and res["bad_words"] == 0, res
    with pytest.raises(RuntimeError):
        plan.join_counters()                 # the hooks are the profiling build's
    plan.close()


@pytest.mark.parametrize("D,poisoned", [(48, True), (48, False), (96, True), (96, False)])
def test_join_checker_sees_a_dropped_block_value(oracle, D, poisoned):
    """SXFIR_BLOCKS_JOIN_DROP=1: the items of block 1 count themselves in without storing their value.  20 launches over two inputs in
    turn.  With the poison the joiner reads a NaN: every tile of every launch differs from the reference and every one of its
    words is a NaN.  Without it the joiner adds what block 1 stored in the launch BEFORE -- the other input's value: from the second
    launch on every tile whose inputs differ reports differing words.  (The first launch without poison reads whatever the
    allocation held and is not counted.)"""
    case = _case(oracle, D, "CF32", 1, "small")
    plan = _plan(D, SXFIR_BLOCKS_JOIN_DROP=1)
    n = 20
    two = JoinSoakView(case, 2)
    res = two.run(plan, n, poison=poisoned, load=False, mixed=False, per_tile=True)
    print("/%d drop, poisoned=%s: %s" % (D, poisoned, res))
    tiles = case.n_tiles * case.nchan
    assert res["counters"] == 0
    if poisoned:
        assert res["tiles_bad"] == [tiles] * n, res
        assert res["tiles_nan"] == [tiles] * n, res
    else:
        differ = case.inputs_differ_tiles(0, 1)
        assert differ == tiles                      # (windows of a random buffer: every tile's input differs)
        assert res["tiles_bad"][1:] == [differ] * (n - 1), res
        assert all(t == 0 for t in res["tiles_nan"][1:]), res
    plan.close()
    # ... and the same plan shape without the knob, same loop: clean
    plan = _plan(D)
    res = two.run(plan, n, poison=poisoned, load=False, mixed=False, per_tile=True)
    assert res["bad_words"] == 0 and res["tiles_bad"] == [0] * n and res["counters"] == 0, res
    plan.close()


class JoinSoakView:
    """A case restricted to its first `n_inputs` inputs."""
    def __init__(self, case, n_inputs):
        self._case, self._n = case, n_inputs

    def run(self, *a, **kw):
        saved = self._case.n_inputs
        self._case.n_inputs = self._n
        try:
            return self._case.run(*a, **kw)
        finally:
            self._case.n_inputs = saved


@pytest.mark.parametrize("D", [48, 96])
def test_reset_clears_the_arrival_counters(oracle, D):
    """Arrival counters left non-zero (an abandoned launch, a plan misused on two streams) make a tile join early or never; reset()
    puts them back to zero with the history.  A launch never runs here on a corrupted counter without a reset() in front of it."""
    import torch
    case = _case(oracle, D, "CF32", 1, "small")
    plan = _plan(D)
    case.check_geometry(plan)
    NB = D // 16
    s = case.stream.cuda_stream
    case.launch(plan, 0, "full")
    case.stream.synchronize()
    assert torch.equal(case.y, case.refs[0, "full"])
    assert plan.join_counters(s) == 0
    plan.join_set_counter(3, 1, s)
    plan.join_set_counter(case.n_tiles - 1, NB - 1, s)
    assert plan.join_counters(s) == 2                      # the hook wrote them
    case.launch(plan, 0, "full")                           # (reset() first, on the same stream)
    case.stream.synchronize()
    bad = int((case.y != case.refs[0, "full"]).sum())
    assert bad == 0, "%d words differ after reset() over corrupted arrival counters" % bad
    assert plan.join_counters(s) == 0
    plan.close()
    with pytest.raises(sxxcvr_amd.NativeError):            # a plan without the scratch: SXFIR_EUNSUPPORTED
        p4 = sxxcvr_amd.Resampler(DECIMATE, sxxcvr_amd.design_lowpass(128, 4, 8.0, 1.0), 4, profiling=True)
        p4.join_poison()


def test_counters_are_zero_between_launches_of_different_sizes(oracle):
    """/96, three channels, ONE stream without reset: several rounds of items, one tile, 64 tiles, four outputs, 64 tiles again.
    Every call against the oracle over the concatenated stream; the arrival counters all zero after each call."""
    import torch
    D, nchan = 96, 3
    plan = _plan(D, nchan=nchan)
    contract = plan.contract
    rot = contract.rot
    assert tuple(contract) == (2, 4) and rot == 1
    js, cw = contract
    lens = [_rounds_outputs(D, nchan), TILE_OUT, SMALL, 4, SMALL]
    g = plan.geometry(D * lens[0])
    assert g["n_tiles"] * nchan >= 3 * g["resident"] + 5, g
    total = sum(lens)
    x = torch.empty((nchan, D * total), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 70, 0)
    y = torch.empty((nchan, total), dtype=torch.int64, device="cuda")
    y.view(torch.int32).fill_(OUT_FILL)
    st = torch.cuda.current_stream().cuda_stream
    pos = 0
    for n in lens:
        g = plan.geometry(D * n)
        assert g["kernel"] == "decim_blocks_kernel" and g["split"] == D // 16, (n, g)
        got = plan.process_ptr(x.data_ptr() + 8 * D * pos, D * n, D * total, y.data_ptr() + 8 * pos, total, st)
        assert got == n
        assert plan.join_counters(st) == 0, "arrival counters left non-zero by a call of %d outputs" % n
        pos += n
    yh = to_cpu(y).view(np.complex64)
    for c in range(nchan):
        want = oracle.decim_f32(join_taps(D), D, to_cpu(x[c]), js, cw, rot=rot, threads=oracle.max_threads())
        pos = 0
        for n in lens:
            assert_bit_exact(yh[c, pos:pos + n], want[pos:pos + n], "/96 channel %d, call of %d outputs at %d" % (c, n, pos))
            pos += n
    plan.close()
