"""The K-relay Q4_K kernel's tail (k_gemv_q4K_kr, TTS_HIP_OPT_GEMV_KR_TAIL): the residual of a fused ADD requested at
kernel entry, and K = 1024 folded after one barrier instead of relayed through three.

Bar: bits.  Both change when values are read and which wave adds them, never an addition or its order, so every
option value must give ggml's result (py_oracle.gemv; with a residual, that product followed by one f32 add) and the
result of the relay with the residual read at the store (option 0).
K = 1024 folds (one block per wave), 2048 relays two blocks per wave, 4096 four; M = 9 / 17 leave a partial column
tile, 16 / 32 fill theirs; N = 16 is a single row tile, 176 an odd count of them.
"""
import functools

import numpy as np
import pytest

import helpers
import py_oracle
import ttship

TAIL = ttship.OPT["GEMV_KR_TAIL"]
DEFAULT = ttship.GEMV_KR_TAIL_DEFAULT
ON = [1, 2, 3, 4]  # fold over the operand tile (default), fold beside it, early residual alone, fold alone
KS = [1024, 2048, 4096]
NS = [16, 64, 176]
MS = [9, 16, 17, 32]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(K, N, M):
    """Weights, activations (column 1 all zero: every term a signed zero), residual (its column 1 all -0) and the
    oracle's product, computed once per shape and shared read-only."""
    rng = np.random.default_rng(K * 11 + N * 3 + M)
    w = helpers.rand_q4_K(rng, N, K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[1] = 0.0
    res = rng.standard_normal((M, N)).astype(np.float32)
    res[1] = -0.0
    ref = py_oracle.gemv(ttship.Q4_K, w, x, N)
    for a in (w, x, res, ref):
        a.setflags(write=False)
    return w, x, res, ref


class Dev:
    """One shape's weights (lane or tile layout) and activations on the device."""

    def __init__(self, hip, w, x, N, tiled):
        self.hip, self.N, (self.M, self.K) = hip, N, x.shape
        w = np.ascontiguousarray(w, dtype=np.uint8)
        rp = np.empty_like(w)
        if tiled:
            ttship.lib().tts_repack_q4_K_tiled(w.ctypes.data, rp.ctypes.data, N, self.K // 256, 0)
        else:
            ttship.lib().tts_repack_q4_K(w.ctypes.data, rp.ctypes.data, w.nbytes // 144, 0)
        self.flags = 32 if tiled else 0  # TTS_FLAG_TILED
        self.dw, self.dx, self.dy, self.dr = hip.alloc(rp.nbytes), hip.alloc(x.nbytes), hip.alloc(4 * self.M * N), hip.alloc(4 * self.M * N)
        hip.set(self.dw, rp)
        hip.set(self.dx, np.ascontiguousarray(x))

    def run(self, opt, res=None, alias=False):
        """The product (+ res) with the option at `opt`; alias: the output is the residual's own buffer."""
        hip = self.hip
        y = np.full((self.M, self.N), np.nan, dtype=np.float32)
        hip.set(self.dy, y)
        dres = None
        if res is not None:
            dres = self.dy if alias else self.dr
            hip.set(dres, np.ascontiguousarray(res))
        hip.set_option(TAIL, opt)
        try:
            st = ttship.lib().tts_hip_gemv_res(hip.ptr, ttship.Q4_K, self.dw, self.dx, self.dy, dres, self.K, self.N, self.M, self.flags)
        finally:
            hip.set_option(TAIL, DEFAULT)
        assert st == 0
        hip.get(y, self.dy)
        return y

    def close(self):
        for p in (self.dw, self.dx, self.dy, self.dr):
            self.hip.free(p)


def check(hip, w, x, res, ref, N, tiled):
    d = Dev(hip, w, x, N, tiled)
    try:
        off = d.run(0)
        assert np.array_equal(bits(off), bits(ref)), f"option 0: product differs from the oracle's, {np.abs(off - ref).max()}"
        for opt in ON:
            got = d.run(opt)
            assert np.array_equal(bits(got), bits(ref)), f"option {opt}: product differs from the oracle's, {np.abs(got - ref).max()}"
        want = ref + res  # one rounded f32 add per element, as the ADD node
        off = d.run(0, res)
        assert np.array_equal(bits(off), bits(want)), f"option 0: product + residual differs, {np.abs(off - want).max()}"
        for opt in ON:
            got = d.run(opt, res)
            assert np.array_equal(bits(got), bits(want)), f"option {opt}: product + residual differs, {np.abs(got - want).max()}"
            got = d.run(opt, res, alias=True)
            assert np.array_equal(bits(got), bits(want)), f"option {opt}: output in the residual's buffer differs, {np.abs(got - want).max()}"
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", [False, True], ids=["lane", "tile"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_kr_tail(hip, tiled, K, N, M):
    """Plain product and product + residual (also with the output in the residual's buffer) for every option value:
    bits equal the oracle's and option 0's.  Column 1 of the activation is all zero and its residual all -0."""
    w, x, res, ref = case(K, N, M)
    check(hip, w, x, res, ref, N, tiled)


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", [False, True], ids=["lane", "tile"])
@pytest.mark.parametrize("M", [1, 8])
def test_kr_tail_gemv(hip, tiled, M):
    """The same at <= 8 columns, where K = 1024 runs the kernel as a GEMV (one workgroup per row tile)."""
    K, N = 1024, 176
    rng = np.random.default_rng(5 + M)
    w = helpers.rand_q4_K(rng, N, K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[0, : K // 2] = 0.0
    res = rng.standard_normal((M, N)).astype(np.float32)
    check(hip, w, x, res, py_oracle.gemv(ttship.Q4_K, w, x, N), N, tiled)


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", [False, True], ids=["lane", "tile"])
@pytest.mark.parametrize("K", [1024, 2048])
def test_kr_tail_extreme_blocks(hip, tiled, K):
    """The largest terms the chain adds (test_q4_K_mfma_extreme_blocks: every scale and min 63, nibbles 15, activations
    quantized to +-127), beside an all-zero column, through the fold (K = 1024) and the relay (2048)."""
    N, M = 64, 17
    rng = np.random.default_rng(7 + K)
    w = helpers.rand_q4_K(rng, N, K)
    blk = w.reshape(-1, 144)
    blk[:, 4:16] = 0xFF               # every 6-bit scale and min = 63
    blk[: len(blk) // 2, 16:] = 0xFF  # nibbles 15
    x = np.full((M, K), 3.0, dtype=np.float32)
    x[1::4] = -3.0
    x[2::4, ::2] = -1.0
    x[3::4] = rng.standard_normal((len(x[3::4]), K)).astype(np.float32)
    x[4] = 0.0
    res = (rng.standard_normal((M, N)) * 1e3).astype(np.float32)
    res[4] = -0.0
    check(hip, w, x, res, py_oracle.gemv(ttship.Q4_K, w, x, N), N, tiled)
