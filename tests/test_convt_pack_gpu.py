"""conv_transpose_1d staged from a packed weight image (TTS_HIP_OPT_CONVT_PACK, k_convt_f64_img / k_convt_pack in
k_conv.hip) against the kernel that fetches and transposes its weight slice itself (option 0, k_convt_f64_lds).

The image kernel walks the same chunks of 16 input channels and gives every output the same MFMAs in the same
order (strides 6, 8 and 10 on eight waves of 16 channels instead of four of 32), so the two must agree bit for bit
(np.array_equal); small-integer data, exact whatever the order, pins the image's tap, half, channel and lane
mapping against the oracle.  The image shares the fused conv_1d's table (tests/test_conv_pack_gpu.py): one per
(weight, geometry), following every write of the weight's bytes, gone with the weight's buffer; a launch split
over input channels asks for none.  The shapes are far below the 512 workgroups under which the launcher splits,
so most cases run with TTS_HIP_OPT_CONV_SPLIT 0; `images` (tts_hip_counters) says whether a launch had an image.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import convs
import nodes as nd
import py_oracle
import ttship
from test_conv_gpu import assert_rel, rnd
from test_conv_pack_gpu import DeviceGraph, images, run_hip, run_oracle
from test_dac_gpu import CFGS, decode

F32, F16 = ttship.F32, ttship.F16
DEFAULTS = {"CONV_SPLIT": 1, "CONVT_PACK": 1, "CONV_XREG": 1, "GRAPHS": 0}


@contextlib.contextmanager
def options(hip, **kw):
    for k, v in kw.items():
        hip.set_option(ttship.OPT[k], v)
    try:
        yield
    finally:
        for k in kw:
            hip.set_option(ttship.OPT[k], DEFAULTS[k])


def both_ways(hip, build, **opts):
    """(image outputs, option-0 outputs, images alive with CONVT_PACK 1); option 0 must never make an image."""
    with options(hip, CONVT_PACK=1, **opts):
        packed, n1 = run_hip(hip, build)
    with options(hip, CONVT_PACK=0, **opts):
        plain, n0 = run_hip(hip, build)
    assert n0 == 0
    return packed, plain, n1


def convt_graph(x, w, S, wtype=F32):
    """The codecs' upsampler: kernel 2 S, padding S / 2, so OL = L S and the first and last S / 2 outputs are cut."""
    return lambda g: [convs.conv_transpose_1d(g, x, w, S, S // 2, 1, 0, 1, wtype)]


OCS = (16, 32, 48)             # half a channel tile, one, one and a tail
LS = (1, 5, 63, 64, 65, 130)   # below, at and past a tile of 64 positions; three tiles with a tail


@pytest.mark.gpu
@pytest.mark.parametrize("wtype", [F32, F16])
@pytest.mark.parametrize("IC", [16, 24, 40])  # one chunk, a tail chunk of 8, three chunks with a tail (odd and even counts)
@pytest.mark.parametrize("S", [2, 4, 6, 8, 10])
def test_image_equals_option0(hip, S, IC, wtype):
    for OC in OCS:
        w = rnd(2, IC, OC, 2 * S, scale=0.2)
        for L in LS:
            build = convt_graph(rnd(1, IC, L), w, S, wtype)
            (packed,), (plain,), n = both_ways(hip, build, CONV_SPLIT=0)
            assert n == 1, (OC, L)  # the launch had an image
            assert packed.shape == plain.shape and packed.shape[-2:] == (OC, L * S)
            assert np.array_equal(packed, plain), (OC, L)
            ref, = run_oracle(build)
            assert_rel(packed, ref, rel=1e-5)  # test_conv_transpose_1d's bar


def integer_case(S, IC, OC, L, seed=7):
    """Inputs and weights in {-2 .. 2} plus quarters that differ by channel, input channel and tap: every product
    and partial sum is exact, so a wrong lane, tap or slot is a wrong number and not a rounding."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, size=(IC, L)).astype(np.float32)
    q = (np.arange(IC)[:, None, None] + 2 * np.arange(OC)[None, :, None] + 3 * np.arange(2 * S)[None, None, :]) % 4 * 0.25
    w = (rng.integers(-2, 3, size=(IC, OC, 2 * S)) + q).astype(np.float32)
    return x, w


@pytest.mark.gpu
@pytest.mark.parametrize("wtype", [F32, F16])
@pytest.mark.parametrize("S", [2, 4, 6, 8, 10])
def test_image_mapping_integer_exact(hip, S, wtype):
    x, w = integer_case(S, 40, 48, 130)
    build = convt_graph(x, w, S, wtype)
    with options(hip, CONV_SPLIT=0):
        (gpu,), n = run_hip(hip, build)
    assert n == 1
    ref, = run_oracle(build)
    assert np.array_equal(gpu, ref)


def weight_leaf(g, w):
    """The weight leaf of a convt_graph: ne = (K, OC, IC)."""
    IC, OC, K = w.shape
    leaf, = [t for t in g.tensors if t.op == 0 and not getattr(t, "_view_of", None) and [t.ne[i] for i in range(3)] == [K, OC, IC]]
    return leaf


@pytest.mark.gpu
@pytest.mark.parametrize("how,S,graphs", [("weight_set", 8, 1), ("tensor_set", 4, 0)])
def test_weight_rewritten_after_first_run(hip, how, S, graphs):
    """The image follows the weight: run twice (with GRAPHS 1 the second run is the recorded graph, which holds the
    image's address), rewrite the weight through the API, run again.  Integer data: the oracle's bits."""
    x, w = integer_case(S, 40, 48, 70)
    w2 = (w[::-1] * 2 - 1).astype(np.float32)
    assert not np.array_equal(w, w2)
    g = nd.Graph()
    y, = convt_graph(x, w, S)(g)
    wl = weight_leaf(g, w)
    with options(hip, CONV_SPLIT=0, GRAPHS=graphs):
        base = images(hip)
        dg = DeviceGraph(hip, g)
        try:
            dg.run()
            dg.run()
            first = dg.read(y)
            assert images(hip) == base + 1
            w2c = np.ascontiguousarray(w2)
            if how == "weight_set":
                assert ttship.lib().tts_hip_weight_set(hip.ptr, ctypes.byref(wl), w2c.ctypes.data) == 0
            else:
                hip.set(wl.data, w2c)
            dg.run()
            second = dg.read(y)
            assert images(hip) == base + 1  # the same image, packed again
        finally:
            dg.close()
        assert images(hip) == base  # freeing the buffers frees the image
    ref1, = run_oracle(convt_graph(x, w, S))
    ref2, = run_oracle(convt_graph(x, w2, S))
    assert np.array_equal(first, ref1)
    assert np.array_equal(second, ref2)
    assert not np.array_equal(second, first)


SPLIT_CASE = (8, 64, 32, 40)  # S, IC, OC, L


def test_split_case_is_split():
    """launch_conv_transpose_1d's split_count for SPLIT_CASE, restated: (L S + p) / S + 1 = 41 positions are one
    tile of 64, 32 channels one tile, 64 input channels four chunks of 16; 1 workgroup is far below 512."""
    S, IC, OC, L = SPLIT_CASE
    tiles, nchunk, target = (((L * S + S // 2) // S + 1 + 63) // 64) * ((OC + 31) // 32), (IC + 15) // 16, 512
    assert 2 * tiles < target
    assert min((target + tiles - 1) // tiles, nchunk // 2) == 2


@pytest.mark.gpu
def test_split_launch_has_no_image(hip):
    S, IC, OC, L = SPLIT_CASE
    build = convt_graph(rnd(1, IC, L), rnd(2, IC, OC, 2 * S, scale=0.2), S)
    (packed,), (plain,), n = both_ways(hip, build)
    assert n == 0  # no image was asked for
    assert np.array_equal(packed, plain)


@pytest.mark.gpu
def test_shared_weight_tensor(hip):
    """One weight tensor under two transposed convs of one graph: one image."""
    S, IC, OC = 8, 40, 48
    w = rnd(2, IC, OC, 2 * S, scale=0.2)
    xs = [rnd(1, IC, 130), rnd(3, IC, 65)]

    def build(g):
        wl = g.leaf(w)
        return [g.node("CONV_TRANSPOSE_1D", F32, [x.shape[1] * S, OC], [wl, g.leaf(x)], params=[S, S // 2, 1, 0, 1]) for x in xs]

    packed, plain, n = both_ways(hip, build, CONV_SPLIT=0)
    assert n == 1
    for a, b in zip(packed, plain):
        assert np.array_equal(a, b)
    refs = run_oracle(build)
    for a, r in zip(packed, refs):
        assert_rel(a, r, rel=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
def test_dac_narrow_end_to_end(hip, split):
    """The narrow DAC-44k decoder (transposed convs of stride 8, 8, 4 and 2), a few frames: identical PCM with
    TTS_HIP_OPT_CONVT_PACK and TTS_HIP_OPT_CONV_XREG on and off (CONV_SPLIT 0: every transposed conv reads an image
    and every fused conv runs the packed kernel; the default: the splits do neither)."""
    cfg = ttship.dac_config(**CFGS["dac44k_narrow"])
    codes = np.random.default_rng(11).integers(0, cfg.codebook_size, size=(4, cfg.n_codebooks))
    pcm = []
    for on in (1, 0):
        with options(hip, CONV_SPLIT=split, CONVT_PACK=on, CONV_XREG=on):
            pcm.append(decode(hip.iface(), cfg, codes))
    assert np.array_equal(pcm[0], pcm[1])
    if split == 0:
        ref = decode(py_oracle.iface(8), cfg, codes)
        assert float(np.max(np.abs(pcm[0].astype(np.float64) - ref))) <= 1e-4
