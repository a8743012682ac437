"""Comparisons shared by test_ops_ref_cpu.py and test_ops_strided_gpu.py: a case of ops_matrix run by some
executor (the oracle, the HIP backend) against ops_ref, at the case's bar."""
import ctypes

import numpy as np

import nodes as nd
import ops_ref
import ttship


def supports(t):
    L = ttship.lib()
    L.tts_hip_supports_op.argtypes = [ctypes.POINTER(ttship.TtsTensor)]
    L.tts_hip_supports_op.restype = ctypes.c_int
    return int(L.tts_hip_supports_op(ctypes.byref(t)))


def build(case):
    g = nd.Graph()
    out = case.build(g)
    return g, (out if isinstance(out, list) else [out])


def _ordered(a):
    """f32 bit patterns mapped so that consecutive floats are consecutive integers (-0 and +0 coincide)."""
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def compare(what, got, want, bar):
    """got / want: arrays of one dtype.  bits: identical but for NaN payloads.  ulp1: f32 only; NaN in the same
    places, every other element within 1 ulp, and at least 99.9 % of all elements bit-equal."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.int32:
        bad = got != want
        assert not bad.any(), f"{what}: {bad.sum()} / {got.size} integers differ, first {got[bad][:4]} for {want[bad][:4]}"
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN at {gn.sum()} places, the reference has {wn.sum()}"
    ub = np.uint16 if got.dtype == np.float16 else np.uint32
    same = (got.view(ub) == want.view(ub)) | gn
    if bar == "ulp1" and got.dtype == np.float32:
        d = np.abs(_ordered(got) - _ordered(want))[~gn]
        worst = int(d.max()) if d.size else 0
        print(f"{what}: {int((~same).sum())} / {got.size} differ, worst {worst} ulp")
        assert worst <= 1, f"{what}: {worst} ulp from the reference"
        assert same.mean() >= 0.999, f"{what}: only {same.mean():.4%} of {got.size} elements bit-equal"
        return
    if not same.all():
        k = np.flatnonzero(~same.reshape(-1))[:4]
        raise AssertionError(f"{what}: {int((~same).sum())} / {got.size} differ; got {got.reshape(-1)[k]} for {want.reshape(-1)[k]}")


def check_against_ref(case, g, outs, ref_bufs):
    """g's buffers after a run against the reference's: the outputs at the case's bar, and every byte of a
    source buffer or of an output's buffer that is no output element unchanged (padding, slack, neighbours)."""
    masks = {}
    for k, t in enumerate(outs):
        compare(f"{case.id}[{k}]", ops_ref.read(g, g.arrays, t), ops_ref.read(g, ref_bufs, t), case.bar)
        owner, m = ops_ref.elem_mask(g, t)
        masks[owner] = masks.get(owner, False) | m
    computed = {ctypes.addressof(n) for n in g.nodes}
    for t in g.tensors:
        if id(t) not in g.arrays:
            continue
        if ctypes.addressof(t) in computed and id(t) not in masks:
            continue            # an intermediate of a chain: a fused plan need not write it
        keep = ~masks[id(t)] if id(t) in masks else slice(None)
        assert np.array_equal(g.arrays[id(t)][keep], ref_bufs[id(t)][keep]), f"{case.id}: bytes outside the outputs changed"
