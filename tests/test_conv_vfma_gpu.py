"""The fused conv_1d's two newer paths (k_conv.hip) against the CPU oracle:

 - k_conv1d_f64v (TTS_HIP_OPT_CONV_VFMA): f64 vector FMAs, lane = output position, one accumulator per
   output taking its terms in r = ic * K + k ascending -- the oracle's order (ggml_vec_dot_f16), so the f32
   results must be the oracle's bit for bit (np.array_equal, no tolerance);
 - the 96-row MFMA tile (TTS_HIP_OPT_CONV_TILE96): each output's MFMAs are the 64-row tile's in the same
   order, so the two tiles must agree bit for bit; against the oracle the f64 sums differ in order only
   (the bar of test_conv_gpu.py's fused-epilogue test: 1e-6 of the scale, at most 1e-3 of the outputs).

The launcher keeps both off a launch it splits over input channels (short sequences), so the cases that
are to reach them run with TTS_HIP_OPT_CONV_SPLIT 0; the fall-back cases run with the default.
"""
import contextlib

import numpy as np
import pytest

import convs
import nodes as nd
import py_oracle
import ttship
from test_conv_gpu import assert_rel, rnd, run_both
from test_dac_gpu import CFGS, decode

F32, F16 = ttship.F32, ttship.F16


@contextlib.contextmanager
def options(hip, **kw):
    """Set backend options by name for the block; the defaults come back after it."""
    defaults = {"CONV_VFMA": 1, "CONV_TILE96": 1, "CONV_SPLIT": 1}
    for k, v in kw.items():
        hip.set_option(ttship.OPT[k], v)
    try:
        yield
    finally:
        for k in kw:
            hip.set_option(ttship.OPT[k], defaults[k])


def conv_graph(x, w, s, p, d, wtype=F32, bias=None, res=None):
    def build(g):
        OC, OL = w.shape[0], (x.shape[1] + 2 * p - d * (w.shape[2] - 1) - 1) // s + 1
        y = convs.conv_1d(g, x, w, s, p, d, wtype=wtype)
        if bias is not None:
            y = g.node("ADD", F32, [OL, OC], [y, g.leaf(bias)])
        if res is not None:
            y = g.node("ADD", F32, [OL, OC], [g.leaf(res), y])
        return [y]
    return build


def integer_case(OC, seed=7):
    """test_gemm_mfma_integer_exact's construction: every product and partial sum is exact."""
    rng = np.random.default_rng(seed)
    IC, L, K = 40, 70, 3
    x = rng.integers(-3, 4, size=(IC, L)).astype(np.float32)
    w = (rng.integers(-4, 5, size=(OC, IC, K)) + np.arange(OC)[:, None, None] * 0.25).astype(np.float32)
    return x, w


# ---------------------------------------------------------------------------------- vector FMA kernel
@pytest.mark.gpu
@pytest.mark.parametrize("wtype", [F32, F16])
def test_vfma_lane_mapping_integer_exact(hip, wtype):
    x, w = integer_case(37)
    with options(hip, CONV_VFMA=2, CONV_SPLIT=0):
        (gpu, ref), = run_both(hip, conv_graph(x, w, 1, 1, 1, wtype))
    assert np.array_equal(gpu, ref)


VFMA_CASES = [  # IC, OC, L, K, s, p, d, epilogue, kernel type
    (16, 12, 40, 7, 1, 9, 3, "", F32),            # tiny
    (64, 96, 300, 7, 1, 3, 1, "", F32),           # OC = 96
    (64, 96, 300, 7, 1, 3, 1, "", F16),
    (96, 1, 100, 7, 1, 3, 1, "b", F32),           # the DAC output conv's shape (one channel)
    (22, 16, 255, 1, 1, 0, 1, "", F32),           # IC tail, position-tile edge
    (22, 16, 256, 1, 1, 0, 1, "", F32),
    (22, 16, 257, 1, 1, 0, 1, "", F32),
    (9, 24, 500, 11, 1, 25, 5, "", F32),          # halo wider than a 64-lane row
    (64, 64, 300, 7, 1, 9, 3, "br", F32),         # full epilogue
    (8, 70, 33, 1, 1, 0, 1, "", F32),             # OC tail, L shorter than a tile
    (5, 3, 1100, 5, 1, 4, 2, "br", F32),          # more than one 1024-position workgroup tile, tail tile
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", VFMA_CASES)
def test_vfma_bit_equal_to_oracle(hip, case):
    IC, OC, L, K, s, p, d, epi, wtype = case
    OL = (L + 2 * p - d * (K - 1) - 1) // s + 1
    x, w = rnd(3, IC, L), rnd(4, OC, IC, K, scale=0.1)
    bias = rnd(7, OC, 1) if "b" in epi else None
    res = rnd(8, OC, OL) if "r" in epi else None
    with options(hip, CONV_VFMA=2, CONV_SPLIT=0):
        (gpu, ref), = run_both(hip, conv_graph(x, w, s, p, d, wtype, bias, res))
    assert gpu.shape == ref.shape
    assert np.array_equal(gpu, ref)


@pytest.mark.gpu
def test_vfma_default_rule_takes_the_one_channel_conv(hip):
    """Option 1 (the default) sends a conv of fewer than 8 output channels to the vector kernel: the oracle's bits."""
    x, w, b = rnd(3, 96, 1500), rnd(4, 1, 96, 7, scale=0.1), rnd(7, 1, 1)
    with options(hip, CONV_SPLIT=0):
        (gpu, ref), = run_both(hip, conv_graph(x, w, 1, 3, 1, F32, b))
    assert np.array_equal(gpu, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [0, 1, 2])
@pytest.mark.parametrize("case", [(22, 32, 241, 12, 6, 3, 1),    # strided: the MFMA kernel
                                  (64, 96, 300, 7, 1, 3, 1)])    # split over input channels: the MFMA kernel
def test_vfma_fallback_to_mfma(hip, case, opt):
    IC, OC, L, K, s, p, d = case
    x, w = rnd(3, IC, L), rnd(4, OC, IC, K, scale=0.1)
    with options(hip, CONV_VFMA=opt):
        (gpu, ref), = run_both(hip, conv_graph(x, w, s, p, d))
    assert_rel(gpu, ref)


def test_split_case_is_split():
    """The split case above is one: launch_conv1d_fused's split_count for it, restated (k_conv.hip).
    64 channels of K = 7 go in chunks of 9 (conv1d_icc: 63 of 64 reduction slots), 8 chunks; the grid of
    5 x 2 tiles is far below 512 workgroups, so the chunks are split, two at least per split."""
    tiles, nchunk, target = ((300 + 63) // 64) * ((96 + 63) // 64), (64 + 8) // 9, 512
    assert 2 * tiles < target
    assert min((target + tiles - 1) // tiles, nchunk // 2) == 4


@pytest.mark.gpu
def test_vfma_aliased_output(hip):
    """The conv's output placed over its input (a graph allocator reuses x once IM2COL has read it): the fused
    kernel then writes a staging buffer that is copied into place.  Same bits as with an output of its own."""
    IC = OC = 32
    L, K, p = 300, 7, 3
    x, w = rnd(3, IC, L), rnd(4, OC, IC, K, scale=0.1)

    def build(g, alias):
        wl, xl = g.leaf(w), g.leaf(x)
        col = g.node("IM2COL", F16, [IC * K, L, 1], [wl, xl], params=[1, 1, p, 0, 1, 1, 0])
        col2 = g.view(col, [IC * K, L, 1, 1], [2, 2 * IC * K, 2 * IC * K * L, 2 * IC * K * L], op="RESHAPE")
        w2 = g.view(wl, [K * IC, OC, 1, 1], [4, 4 * K * IC, 4 * K * IC * OC, 4 * K * IC * OC], op="RESHAPE")
        return g.node("MUL_MAT", F32, [L, OC], [col2, w2], on=(xl, 0) if alias else None)

    out = []
    with options(hip, CONV_VFMA=2, CONV_SPLIT=0):
        for alias in (False, True):
            g = nd.Graph()
            y = build(g, alias)
            g.run_hip(hip)
            out.append(g.node_array(y))
    g = nd.Graph()
    y = build(g, False)
    g.run_oracle()
    assert np.array_equal(out[0], g.node_array(y))
    assert np.array_equal(out[1], out[0])


# ---------------------------------------------------------------------------------- 96-row MFMA tile
@pytest.mark.gpu
@pytest.mark.parametrize("wtype", [F32, F16])
def test_tile96_lane_mapping_integer_exact(hip, wtype):
    x, w = integer_case(96)
    with options(hip, CONV_VFMA=0, CONV_SPLIT=0):
        (gpu, ref), = run_both(hip, conv_graph(x, w, 1, 1, 1, wtype))
    assert np.array_equal(gpu, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(64, 96, 300, 7, 1, 3, 1, "", F32), (64, 96, 300, 7, 1, 3, 1, "", F16),
                                  (64, 192, 300, 7, 1, 9, 3, "br", F32), (22, 96, 257, 1, 1, 0, 1, "b", F32),
                                  (22, 192, 241, 12, 6, 3, 1, "b", F32)])
def test_tile96_equals_tile64(hip, case):
    IC, OC, L, K, s, p, d, epi, wtype = case
    OL = (L + 2 * p - d * (K - 1) - 1) // s + 1
    x, w = rnd(3, IC, L), rnd(4, OC, IC, K, scale=0.1)
    bias = rnd(7, OC, 1) if "b" in epi else None
    res = rnd(8, OC, OL) if "r" in epi else None
    got = []
    for t96 in (1, 0):
        with options(hip, CONV_VFMA=0, CONV_SPLIT=0, CONV_TILE96=t96):
            (gpu, ref), = run_both(hip, conv_graph(x, w, s, p, d, wtype, bias, res))
        got.append(gpu)
    assert np.array_equal(got[0], got[1])
    assert float(np.mean(got[0] != ref)) <= 1e-3
    assert_rel(got[0], ref, rel=1e-6)


# ---------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def dac_runs(hip):
    """PCM of the two DAC configurations per option set, and the oracle's, computed once."""
    out = {}
    for name, T in (("dac44k_narrow", 4), ("dac44k", 3)):
        cfg = ttship.dac_config(**CFGS[name])
        codes = np.random.default_rng(11).integers(0, cfg.codebook_size, size=(T, cfg.n_codebooks))
        out[name, "oracle"] = decode(py_oracle.iface(8), cfg, codes)
        for key, kw in (("mfma64", dict(CONV_VFMA=0, CONV_TILE96=0)), ("mfma96", dict(CONV_VFMA=0, CONV_TILE96=1)),
                        ("vfma", dict(CONV_VFMA=2, CONV_TILE96=0)), ("default", {})):
            with options(hip, CONV_SPLIT=0, **kw):
                out[name, key] = decode(hip.iface(), cfg, codes)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dac44k_narrow", "dac44k"])
def test_dac_end_to_end(dac_runs, name):
    ref = dac_runs[name, "oracle"]
    for key in ("mfma64", "mfma96", "vfma", "default"):
        err = float(np.max(np.abs(dac_runs[name, key].astype(np.float64) - ref)))
        print(f"dac {name} {key}: max |pcm - oracle| {err:.3e}, samples differing from mfma64 "
              f"{int(np.sum(dac_runs[name, key] != dac_runs[name, 'mfma64']))}")
        assert err <= 1e-4, (key, err)
    assert np.array_equal(dac_runs[name, "mfma96"], dac_runs[name, "mfma64"])
    assert np.array_equal(dac_runs[name, "vfma"], dac_runs[name, "mfma64"])
    assert np.array_equal(dac_runs[name, "default"], dac_runs[name, "mfma64"])
