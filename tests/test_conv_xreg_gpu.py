"""The packed fused conv_1d with its reduction-slot -> x-window table held in registers (TTS_HIP_OPT_CONV_XREG,
k_conv1d_f64p<..., XREG = true> in k_conv.hip) against the same kernel reading the table from LDS per batch
(option 0).  The same table entries address the same x slots and the MFMAs run in the same order, so the two must
agree bit for bit.  The cases are tests/test_conv_pack_gpu.py's, plus one, two and three chunks of a k = 7 conv
(a workgroup's batches with Rp = 64 at every chunk parity), output lengths below, at and past a position tile, and
the graph whose output lies over its input.  CONV_SPLIT 0 as there: the shapes are far below the launcher's split.
"""
import contextlib

import numpy as np
import pytest

import ttship
from test_conv_gpu import assert_rel, rnd
from test_conv_pack_gpu import PACK_CASES, case_graph, run_hip, run_oracle

F32, F16 = ttship.F32, ttship.F16
DEFAULTS = {"CONV_SPLIT": 1, "CONV_XREG": 1}


@contextlib.contextmanager
def options(hip, **kw):
    for k, v in kw.items():
        hip.set_option(ttship.OPT[k], v)
    try:
        yield
    finally:
        for k in kw:
            hip.set_option(ttship.OPT[k], DEFAULTS[k])


def both_ways(hip, build):
    out = []
    for xreg in (1, 0):
        with options(hip, CONV_SPLIT=0, CONV_XREG=xreg):
            o, n = run_hip(hip, build)
        assert n == 1  # the packed kernel ran: the launch had an image
        out.append(o)
    return out


XREG_CASES = PACK_CASES + [  # IC, OC, L, K, s, p, d, epilogue, kernel type
    (9, 96, 130, 7, 1, 3, 1, "", F32),     # K = 7: chunks of 9 channels (Rp = 64); one chunk
    (18, 96, 130, 7, 1, 3, 1, "b", F32),   # two chunks
    (27, 64, 130, 7, 1, 3, 1, "br", F32),  # three chunks, the 64-row tile
    (27, 96, 1, 7, 1, 3, 1, "", F32),      # OL = 1
    (18, 96, 64, 7, 1, 3, 1, "", F16),     # OL = 64: exactly one position tile
    (9, 64, 65, 7, 1, 3, 1, "", F32),      # OL = 65: a tile and one position
    (32, 96, 65, 1, 1, 0, 1, "", F32),     # k = 1 with Rp = 32: one batch per chunk
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", XREG_CASES)
def test_xreg_equals_table_in_lds(hip, case):
    build = case_graph(case)
    (reg,), (lds,) = both_ways(hip, build)
    assert reg.shape == lds.shape
    assert np.array_equal(reg, lds)
    ref, = run_oracle(build)
    assert_rel(reg, ref, rel=1e-6)  # test_packed_equals_unpacked's bar


@pytest.mark.gpu
def test_xreg_aliased_output(hip):
    """test_pack_aliased_output's graphs: the output over the input goes through the staging buffer."""
    IC = OC = 32
    L, K, p = 300, 7, 3
    x, w = rnd(3, IC, L), rnd(4, OC, IC, K, scale=0.1)

    def build(alias):
        def f(g):
            wl, xl = g.leaf(w), g.leaf(x)
            col = g.node("IM2COL", F16, [IC * K, L, 1], [wl, xl], params=[1, 1, p, 0, 1, 1, 0])
            col2 = g.view(col, [IC * K, L, 1, 1], [2, 2 * IC * K, 2 * IC * K * L, 2 * IC * K * L], op="RESHAPE")
            w2 = g.view(wl, [K * IC, OC, 1, 1], [4, 4 * K * IC, 4 * K * IC * OC, 4 * K * IC * OC], op="RESHAPE")
            return [g.node("MUL_MAT", F32, [L, OC], [col2, w2], on=(xl, 0) if alias else None)]
        return f

    (ra,), (la,) = both_ways(hip, build(True))
    (rn,), (ln,) = both_ways(hip, build(False))
    assert np.array_equal(ra, la) and np.array_equal(rn, ln) and np.array_equal(ra, rn)
