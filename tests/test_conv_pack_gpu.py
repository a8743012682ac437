"""The fused conv_1d staged from a packed kernel image (TTS_HIP_OPT_CONV_PACK, k_conv1d_f64p / k_conv1d_pack in
k_conv.hip) against the kernel that rounds and scatters its slice itself (option 0).

The packed kernel walks the same chunks and issues the same MFMAs in the same order, so the two must agree bit
for bit (np.array_equal); small-integer data, exact whatever the order, pins the image's lane and slot mapping
against the oracle.  The image is made once per (weight, tile geometry) and must follow every write of the
weight's bytes; a launch the launcher splits over input channels keeps the unpacked kernel.  Most cases are far
below the 512 workgroups under which the launcher splits, so they run with TTS_HIP_OPT_CONV_SPLIT 0 to reach the
packed kernel; `images` (tts_hip_counters) says whether a launch really had an image.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import nodes as nd
import py_oracle
import ttship
from test_conv_gpu import assert_rel, rnd
from test_conv_vfma_gpu import conv_graph, integer_case
from test_dac_gpu import CFGS, decode

F32, F16 = ttship.F32, ttship.F16
DEFAULTS = {"CONV_VFMA": 1, "CONV_TILE96": 1, "CONV_SPLIT": 1, "CONV_PACK": 1, "GRAPHS": 0}


@contextlib.contextmanager
def options(hip, **kw):
    """test_conv_vfma_gpu.options with this file's options: set by name for the block, the defaults after it."""
    for k, v in kw.items():
        hip.set_option(ttship.OPT[k], v)
    try:
        yield
    finally:
        for k in kw:
            hip.set_option(ttship.OPT[k], DEFAULTS[k])


class DeviceGraph:
    """nodes.Graph.run_hip in steps -- upload, run (any number of times), read, close -- so that a graph runs more
    than once on the same device buffers and a weight can be rewritten in between."""

    def __init__(self, hip, g):
        self.hip, self.g = hip, g
        self.dev = {}
        for t in g.tensors:
            if id(t) in g.arrays:
                self.dev[id(t)] = hip.alloc(g.arrays[id(t)].nbytes)
                hip.set(self.dev[id(t)], g.arrays[id(t)])
        self.host = {id(t): t.data for t in g.tensors}
        for t in g.tensors:
            if id(t) in self.dev:
                t.data = self.dev[id(t)]
        for t in g.tensors:
            if getattr(t, "_root", None) is not None:
                owner, at = g.buffer_of(t)
                t.data = self.dev[id(owner)] + at

    def run(self):
        st = ttship.lib().tts_hip_graph_compute(self.hip.ptr, self.g.node_ptrs(), len(self.g.nodes))
        assert st == 0, st
        self.hip.sync()

    def read(self, t):
        owner, _ = self.g.buffer_of(t)
        self.hip.get(self.g.arrays[id(owner)], self.dev[id(owner)])
        return self.g.node_array(t)

    def close(self):
        for d in self.dev.values():
            self.hip.free(d)
        for t in self.g.tensors:
            t.data = self.host[id(t)]


def images(hip):
    return hip.counters()["conv_pack_images"]


def run_hip(hip, build, runs=1):
    """The outputs of build's graph on the device, and the packed images it made (alive right after it ran; gone
    again once its buffers are freed)."""
    g = nd.Graph()
    outs = build(g)
    base = images(hip)
    dg = DeviceGraph(hip, g)
    try:
        for _ in range(runs):
            dg.run()
        n = images(hip) - base
        out = [dg.read(o) for o in outs]
    finally:
        dg.close()
    assert images(hip) == base  # freeing the weights frees their images
    return out, n


def run_oracle(build):
    g = nd.Graph()
    outs = build(g)
    g.run_oracle()
    return [g.node_array(o) for o in outs]


def case_graph(case):
    IC, OC, L, K, s, p, d, epi, wtype = case
    OL = (L + 2 * p - d * (K - 1) - 1) // s + 1
    x, w = rnd(3, IC, L), rnd(4, OC, IC, K, scale=0.1)
    bias = rnd(7, OC, 1) if "b" in epi else None
    res = rnd(8, OC, OL) if "r" in epi else None
    return conv_graph(x, w, s, p, d, wtype, bias, res)


def both_ways(hip, build, **opts):
    """(packed outputs, unpacked outputs, images alive with CONV_PACK 1); option 0 must never make an image."""
    with options(hip, CONV_PACK=1, **opts):
        packed, n1 = run_hip(hip, build)
    with options(hip, CONV_PACK=0, **opts):
        plain, n0 = run_hip(hip, build)
    assert n0 == 0
    return packed, plain, n1


PACK_CASES = [  # IC, OC, L, K, s, p, d, epilogue, kernel type
    (22, 96, 130, 7, 1, 9, 3, "", F32),    # 96-row tile, IC tail chunk 9 + 9 + 4, three position tiles with a tail
    (22, 96, 130, 7, 1, 9, 3, "", F16),    # the same with an F16 kernel
    (64, 192, 70, 1, 1, 0, 1, "br", F32),  # k = 1, icc 64, Rp exactly 64, two channel tiles, full epilogue
    (12, 70, 33, 7, 1, 3, 1, "b", F32),    # 64-row tile, OC tail, L shorter than a tile
    (9, 24, 200, 11, 1, 25, 5, "", F32),   # wide dilated halo
    (20, 64, 97, 3, 1, 1, 1, "", F32),     # k = 3 chunking
    (22, 32, 241, 12, 6, 3, 1, "", F32),   # strided
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACK_CASES)
def test_packed_equals_unpacked(hip, case):
    build = case_graph(case)
    (packed,), (plain,), n = both_ways(hip, build, CONV_SPLIT=0)
    assert n == 1  # the launch had an image
    assert packed.shape == plain.shape
    assert np.array_equal(packed, plain)
    ref, = run_oracle(build)
    assert_rel(packed, ref, rel=1e-6)  # test_tile96_equals_tile64's bar: the f64 sums differ in order only


@pytest.mark.gpu
@pytest.mark.parametrize("wtype", [F32, F16])
@pytest.mark.parametrize("OC", [96, 64])
def test_pack_lane_mapping_integer_exact(hip, OC, wtype):
    """test_tile96_lane_mapping_integer_exact on the packed kernel: a wrong lane or slot in the image is a wrong
    integer, not a rounding."""
    x, w = integer_case(OC)
    build = conv_graph(x, w, 1, 1, 1, wtype)
    with options(hip, CONV_VFMA=0, CONV_SPLIT=0):
        (gpu,), n = run_hip(hip, build)
    assert n == 1
    ref, = run_oracle(build)
    assert np.array_equal(gpu, ref)


def kernel_leaf(g, w):
    """The conv kernel's leaf of a conv_graph: ne = (K, IC, OC)."""
    OC, IC, K = w.shape
    leaf, = [t for t in g.tensors if t.op == 0 and not getattr(t, "_view_of", None) and [t.ne[i] for i in range(3)] == [K, IC, OC]]
    return leaf


@pytest.mark.gpu
@pytest.mark.parametrize("how,OC,graphs", [("weight_set", 64, 1),    # 64 columns: graph_compute records the repeat (GRAPHS 1)
                                           ("tensor_set", 96, 0)])
def test_weight_rewritten_after_first_run(hip, how, OC, graphs):
    """The image follows the weight: run (twice, so that with GRAPHS 1 the second run is the recorded graph, which
    holds the image's address), rewrite the kernel through the API, run again.  Integer data: the oracle's bits."""
    x, w = integer_case(OC)
    w2 = (w[::-1] * 2 - 1).astype(np.float32)  # other small integers (+ quarters), still exact
    assert not np.array_equal(w, w2)
    g = nd.Graph()
    y, = conv_graph(x, w, 1, 1, 1)(g)
    wl = kernel_leaf(g, w)
    with options(hip, CONV_VFMA=0, CONV_SPLIT=0, GRAPHS=graphs):
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
    ref1, = run_oracle(conv_graph(x, w, 1, 1, 1))
    ref2, = run_oracle(conv_graph(x, w2, 1, 1, 1))
    assert np.array_equal(first, ref1)
    assert np.array_equal(second, ref2)
    assert not np.array_equal(second, first)


def conv_on(g, wl, x, p, d=1):
    """convs.conv_1d (s = 1, F32) on an existing kernel leaf wl [K, IC, OC]."""
    K, IC, OC = wl.ne[0], wl.ne[1], wl.ne[2]
    L = x.shape[1]
    OL = L + 2 * p - d * (K - 1)
    col = g.node("IM2COL", ttship.F16, [IC * K, OL, 1], [wl, g.leaf(x)], params=[1, 1, p, 0, d, 1, 0])
    col2 = g.view(col, [IC * K, OL, 1, 1], [2, 2 * IC * K, 2 * IC * K * OL, 2 * IC * K * OL], op="RESHAPE")
    w2 = g.view(wl, [K * IC, OC, 1, 1], [4, 4 * K * IC, 4 * K * IC * OC, 4 * K * IC * OC], op="RESHAPE")
    return g.node("MUL_MAT", F32, [OL, OC], [col2, w2])


@pytest.mark.gpu
def test_shared_kernel_tensor(hip):
    """One kernel tensor under three convs of one graph, default options: two long sequences (2 x 129 tiles, at
    least half of the 512 workgroups the launcher aims for: unsplit, 96-row tiles, one image for both) and a short
    one (2 x 3 tiles of 5 chunks: split in two, so it reads the kernel itself)."""
    IC, OC, K = 40, 96, 7
    w = rnd(4, OC, IC, K, scale=0.1)
    xs = [rnd(3, IC, 8200), rnd(5, IC, 8200), rnd(6, IC, 130)]
    assert 2 * ((8200 + 63) // 64) * 2 >= 512 and min((512 + 5) // 6, ((IC + 8) // 9) // 2) == 2

    def build(g):
        wl = g.leaf(w)
        return [conv_on(g, wl, xs[0], 3), conv_on(g, wl, xs[1], 9, 3), conv_on(g, wl, xs[2], 3)]

    packed, plain, n = both_ways(hip, build)
    assert n == 1
    for a, b in zip(packed, plain):
        assert np.array_equal(a, b)
    assert not np.array_equal(packed[0], packed[1])


SPLIT_CASE = (256, 96, 20, 7, 1, 3, 1, "", F32)


def test_split_case_is_split():
    """launch_conv1d_fused's split_count for SPLIT_CASE, restated (as test_conv_vfma_gpu.test_split_case_is_split):
    256 channels of K = 7 go in chunks of 9, 29 chunks; 1 x 2 tiles are far below 512 workgroups."""
    tiles, nchunk, target = ((20 + 63) // 64) * ((96 + 63) // 64), (256 + 8) // 9, 512
    assert 2 * tiles < target
    assert min((target + tiles - 1) // tiles, nchunk // 2) == 14


@pytest.mark.gpu
def test_split_launch_stays_unpacked(hip):
    build = case_graph(SPLIT_CASE)
    (packed,), (plain,), n = both_ways(hip, build)
    assert n == 0  # no image was asked for
    assert np.array_equal(packed, plain)


@pytest.mark.gpu
def test_pack_aliased_output(hip):
    """test_vfma_aliased_output's graphs on the MFMA kernels: the output over the input goes through the staging
    buffer.  Packed equals unpacked, aliased equals not aliased."""
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

    (pa,), (ua,), na = both_ways(hip, build(True), CONV_SPLIT=0)
    (pn,), (un,), nn = both_ways(hip, build(False), CONV_SPLIT=0)
    assert na == 1 and nn == 1
    assert np.array_equal(pa, ua) and np.array_equal(pn, un) and np.array_equal(pa, pn)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
def test_dac_narrow_end_to_end(hip, split):
    """The narrow DAC-44k decoder, a few frames: identical PCM with and without the images (CONV_SPLIT 0: every
    conv the MFMA kernel takes is packed; the default: the short sequences' splits stay unpacked)."""
    cfg = ttship.dac_config(**CFGS["dac44k_narrow"])
    codes = np.random.default_rng(11).integers(0, cfg.codebook_size, size=(4, cfg.n_codebooks))
    pcm = []
    for pack in (1, 0):
        with options(hip, CONV_SPLIT=split, CONV_PACK=pack):
            pcm.append(decode(hip.iface(), cfg, codes))
    assert np.array_equal(pcm[0], pcm[1])
    if split == 0:
        ref = decode(py_oracle.iface(8), cfg, codes)
        assert float(np.max(np.abs(pcm[0].astype(np.float64) - ref))) <= 1e-4
