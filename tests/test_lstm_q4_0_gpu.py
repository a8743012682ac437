"""Kokoro's LSTM with Q4_0 weights on the HIP backend: the fused step k_lstm_step_q<Q4_0>.

No numpy model of the tanh / sigmoid chain is bitwise, so the step is pinned by transitivity (tests/q4_0_ref.py):
on general-d weights the fused step equals HIP's own unfused node chain in every bit, whose MUL_MAT is the GEMV
that tests/test_q4_0_gpu.py pins to ggml's ((float)sumi * d_w) * d_x order; on trimmed-d weights the fused step
equals the CPU oracle on the Q8_0 twin.  The recurrent matrix is [Hd rows of K = Hd]: rows of 18 K / 32 bytes,
so at K = 32 and K = 96 every other row starts at an odd multiple of 2 bytes.

The transitivity holds only on inputs where the two association orders part.  Random weights and states are not
such inputs (|sumi| < 2^13: both orders give the same bits), so test_lstm_q4_0_fused checks the step's structure
(loads, odd row starts, the pair, the state carried over) and test_lstm_q4_0_fused_folds_in_ggml_order, on
inputs built to part the orders, checks the term.
"""
import numpy as np
import pytest

import lstm_q4_0 as l4
import nodes as nd
import ttship
from test_lstm_quant_gpu import FUSE_LSTM, inputs

pytestmark = pytest.mark.gpu
T = 3


def run_hip(hip, build, mode, fused=True):
    g = nd.Graph()
    o = build(g, mode)
    if not fused:
        hip.set_option(0, ttship.FUSE_ALL & ~FUSE_LSTM)
    try:
        before = hip.counters()
        g.run_hip(hip)
        after = hip.counters()
    finally:
        hip.set_option(0, ttship.FUSE_ALL)
    return g.node_array(o, shape=[o.ne[1], o.ne[0]]), after["lstm_chains"] - before["lstm_chains"], after["lstm_steps"] - before["lstm_steps"]


def run_oracle(build, mode="twin"):
    g = nd.Graph()
    o = build(g, mode)
    g.run_oracle(n_threads=8)
    return g.node_array(o, shape=[o.ne[1], o.ne[0]])


# K = Hd: 1, 2 (64: two blocks), 3 (odd row starts, no power of two), 8 and 16 blocks (the cap); one direction and the pair
@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("hd", [32, 64, 96, 256, 512])
def test_lstm_q4_0_fused(hip, hd, bi):
    x, dirs, h0, c0 = inputs(T, 64, hd, bi)
    n_dir = 2 if bi else 1

    def build(g, mode):
        return l4.lstm_cell(g, x, dirs, mode, h0=h0, c0=c0)
    # general d: fused against HIP's own unfused chain
    gpu, chains, steps = run_hip(hip, build, "general")
    assert chains == n_dir and steps == n_dir * T
    plain, chains0, steps0 = run_hip(hip, build, "general", fused=False)
    assert chains0 == 0 and steps0 == 0
    assert np.isfinite(plain).all() and np.abs(plain).max() > 1e-2
    assert np.array_equal(gpu, plain), f"fused vs unfused: max err {np.abs(gpu - plain).max():.3e}"
    # trimmed d: fused against the oracle on the twin
    gpu, chains, steps = run_hip(hip, build, "trimmed")
    assert chains == n_dir and steps == n_dir * T
    ref = run_oracle(build)
    assert np.array_equal(gpu, ref), f"max err {np.abs(gpu - ref).max():.3e}, {np.mean(gpu != ref):.3e} of the elements differ"


@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("hd", l4.PART_HD)
def test_lstm_q4_0_fused_folds_in_ggml_order(hip, hd, bi):
    """The case that sees the step's association order.  On the random inputs above |sumi| stays below 2^13 and
    ((float)sumi * d_w) * d_x == sumi * (d_w * d_x) in every term, so a step folding in the Q8_0 / Q5_0 order would
    pass there.  lstm_q4_0.parting_inputs gives W_hh and h0 on which the first step's terms part (a condition that
    tests/test_q4_0_cpu.py checks on these very inputs, down to the gates' inputs).  The fused step must equal the
    unfused chain, whose GEMV is pinned to R1 -- and must differ from the oracle on the untrimmed Q8_0 twin, which
    folds in the other order: were that run equal too, this case would tell nothing."""
    x, dirs, h0, c0 = l4.parting_inputs(T, 64, hd, bi)
    n_dir = 2 if bi else 1

    def build(g, mode):
        return l4.lstm_cell(g, x, dirs, mode, h0=h0, c0=c0)
    gpu, chains, steps = run_hip(hip, build, "general")
    assert chains == n_dir and steps == n_dir * T
    plain, chains0, steps0 = run_hip(hip, build, "general", fused=False)
    assert chains0 == 0 and steps0 == 0
    assert np.isfinite(plain).all() and np.abs(plain).max() > 1e-2
    assert np.array_equal(gpu, plain), f"fused vs unfused: max err {np.abs(gpu - plain).max():.3e}"
    other = run_oracle(build, "twin-general")
    # the same cell all the same: a last-bit difference can at most move one int8 of a later step's quantized h by
    # one, worth d_w * d_x * 8, about 1e-4, in a gate's input
    assert np.allclose(gpu, other, rtol=0, atol=1e-3)
    assert not np.array_equal(gpu, other), "the other association order gives the same bits: the inputs pin nothing"


def test_lstm_q4_0_zero_state(hip):
    """Kokoro's initial state: the first step quantizes an all-zero h (d = 0, id = 0)."""
    x, dirs, _, _ = inputs(T, 32, 32, True, zero_state=True)

    def build(g, mode):
        return l4.lstm_cell(g, x, dirs, mode)
    gpu, chains, _ = run_hip(hip, build, "trimmed")
    assert chains == 2
    assert np.array_equal(gpu, run_oracle(build))


def test_lstm_q4_0_not_fused_above_the_row_cap(hip):
    """Rows longer than the quantized step's cap (512) stay with the generic nodes, and still match."""
    x, dirs, h0, c0 = inputs(2, 32, 544, False)

    def build(g, mode):
        return l4.lstm_cell(g, x, dirs, mode, h0=h0, c0=c0)
    gpu, chains, steps = run_hip(hip, build, "trimmed")
    assert chains == 0 and steps == 0
    assert np.array_equal(gpu, run_oracle(build))
