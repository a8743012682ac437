"""Kokoro's LSTM with Q8_0 / Q5_0 weights (a quantized Kokoro file) on the HIP backend vs the CPU oracle.

The graph is the reference's unrolled recurrence with quantized matrix leaves (tests/lstm_quant.py).  With
TTS_FUSE_LSTM the planner turns each chain into one k_lstm_step_q launch per time step.  The quantized step
reassociates nothing -- h_prev is quantized as quantize_row_q8_0 does, the int32 block dots are exact, the
f32 terms are added in block order, the gate chain rounds every intermediate to f32 -- so, unlike the
F32 / F16 step (tests/test_lstm_gpu.py, 2e-6), its output equals the oracle's bit for bit, and equals the
unfused node-by-node run bit for bit.  Q5_0 is compared with the oracle run on the Q8_0 twin.
"""
import numpy as np
import pytest

import lstm
import lstm_quant as lq
import nodes as nd
import ttship

F32, F16, Q8_0, Q5_0 = ttship.F32, ttship.F16, ttship.Q8_0, ttship.Q5_0
FUSE_LSTM = 64


def inputs(T, n_in, hd, bi, zero_state=False):
    rng = np.random.default_rng(1000 * T + hd)
    x = (rng.standard_normal((T, n_in)) * 0.5).astype(np.float32)
    dirs = lstm.lstm_weights(T + hd, n_in, hd, bidirectional=bi)
    if zero_state:  # Kokoro's initial state: the first step quantizes an all-zero h (d = 0, id = 0)
        return x, dirs, None, None
    return x, dirs, (rng.standard_normal(hd) * 0.3).astype(np.float32), (rng.standard_normal(hd) * 0.3).astype(np.float32)


def run_hip(hip, build, fused=True):
    g = nd.Graph()
    o = build(g, False)
    if not fused:
        hip.set_option(0, ttship.FUSE_ALL & ~FUSE_LSTM)
    try:
        before = hip.counters()
        g.run_hip(hip)
        after = hip.counters()
    finally:
        hip.set_option(0, ttship.FUSE_ALL)
    return g.node_array(o, shape=[o.ne[1], o.ne[0]]), after["lstm_chains"] - before["lstm_chains"], after["lstm_steps"] - before["lstm_steps"]


def run_oracle(build):
    g = nd.Graph()
    o = build(g, True)
    g.run_oracle(n_threads=8)
    return g.node_array(o, shape=[o.ne[1], o.ne[0]])


CASES = [  # T, n_in, hidden, bidirectional, weight type
    (1, 32, 32, True, Q8_0),     # one block, one step, no concat chain, 34-byte rows
    (2, 32, 32, False, Q5_0),    # 22-byte rows
    (9, 96, 96, False, Q8_0),    # three blocks, not a power of two
    (9, 96, 96, True, Q5_0),     # three blocks, paired chains
    (20, 640, 256, True, Q8_0),  # Kokoro's shape
    (20, 640, 256, True, Q5_0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_lstm_quant_fused(hip, case):
    T, n_in, hd, bi, wt = case
    x, dirs, h0, c0 = inputs(T, n_in, hd, bi, zero_state=(T == 1))
    n_dir = 2 if bi else 1

    def build(g, twin):
        return lq.lstm_cell(g, x, dirs, [wt] * n_dir, twin=twin, h0=h0, c0=c0)
    gpu, chains, steps = run_hip(hip, build)
    assert chains == n_dir
    assert steps == n_dir * T
    ref = run_oracle(build)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 1e-2
    assert np.array_equal(gpu, ref), f"max err {np.abs(gpu - ref).max():.3e}, {np.mean(gpu != ref):.3e} of the elements differ"
    plain, chains0, steps0 = run_hip(hip, build, fused=False)
    assert chains0 == 0 and steps0 == 0
    assert np.array_equal(gpu, plain), f"fused vs unfused: max err {np.abs(gpu - plain).max():.3e}"


@pytest.mark.gpu
def test_lstm_quant_mixed_directions_fuse_unpaired(hip):
    """Forward weights Q8_0, reverse weights F16: each chain fuses with its own kernel, and the two are not
    advanced by one launch (a launch runs one kernel).  A paired cell plans 1 stash + T steps + 1 output
    write; two plain chains plan 2 (T + 1) items."""
    T, n_in, hd = 7, 64, 32
    x, dirs, h0, c0 = inputs(T, n_in, hd, True)

    def build(wts):
        return lambda g, twin: lq.lstm_cell(g, x, dirs, wts, twin=twin, h0=h0, c0=c0)
    gp = nd.Graph()
    build([Q8_0, Q8_0])(gp, False)
    assert gp.plan()["lstm"] == T + 2
    gm = nd.Graph()
    build([Q8_0, F16])(gm, False)
    assert gm.plan()["lstm"] == 2 * (T + 1)
    gpu, chains, steps = run_hip(hip, build([Q8_0, F16]))
    assert chains == 2 and steps == 2 * T
    plain, _, steps0 = run_hip(hip, build([Q8_0, F16]), fused=False)
    assert steps0 == 0
    # the Q8_0 half is bit-equal; the F16 half is the F32 / F16 step (f64 partial sums per lane: 2e-6)
    assert np.array_equal(gpu[:, :hd], plain[:, :hd])
    assert np.max(np.abs(gpu[:, hd:] - plain[:, hd:])) <= 2e-6
    ref = run_oracle(build([Q8_0, F16]))
    assert np.array_equal(gpu[:, :hd], ref[:, :hd])


@pytest.mark.gpu
@pytest.mark.parametrize("wt", [Q8_0, Q5_0])
def test_lstm_quant_not_fused_above_the_row_cap(hip, wt):
    """Rows longer than the quantized step's cap (512) stay with the generic nodes."""
    T, n_in, hd = 2, 32, 544
    x, dirs, h0, c0 = inputs(T, n_in, hd, False)

    def build(g, twin):
        return lq.lstm_cell(g, x, dirs, [wt], twin=twin, h0=h0, c0=c0)
    gpu, chains, steps = run_hip(hip, build)
    assert chains == 0 and steps == 0
    assert np.array_equal(gpu, run_oracle(build))


@pytest.mark.gpu
def test_lstm_quant_fused_at_the_row_cap(hip):
    """K = 512: every lane of a unit's wave owns an item, and the workgroup quantizes two elements a thread."""
    T, n_in, hd = 3, 32, 512
    x, dirs, h0, c0 = inputs(T, n_in, hd, False)

    def build(g, twin):
        return lq.lstm_cell(g, x, dirs, [Q5_0], twin=twin, h0=h0, c0=c0)
    gpu, chains, steps = run_hip(hip, build)
    assert chains == 1 and steps == T
    assert np.array_equal(gpu, run_oracle(build))


@pytest.mark.gpu
def test_lstm_quant_not_fused_when_intermediate_escapes(hip):
    """An intermediate read outside the chain (here the last cell state) keeps the generic path."""
    T, n_in, hd = 6, 32, 32
    x, dirs, h0, c0 = inputs(T, n_in, hd, False)

    def build(g, twin):
        xl = g.leaf(x)
        out, h, c = lq.lstm_run(g, xl, g.leaf(h0), g.leaf(c0), dirs[0], wtype=Q8_0, twin=twin)
        side = g.node("SCALE", F32, [hd, 1], [c], fparams={0: 2.0})  # c_last read outside the chain
        return g.node("CONCAT", F32, [hd, T + 1], [out, side], params=[1])
    gpu, chains, steps = run_hip(hip, build)
    assert chains == 0 and steps == 0
    assert np.array_equal(gpu, run_oracle(build))
