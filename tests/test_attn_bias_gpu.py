"""Encoder attention with a per-head additive bias (k_attn_bias, k_attn.hip) vs the oracle running the
unfused T5 chain (attn_bias_chain.py).  Every sum of the kernel is sequential in the oracle's order, so
the result is bit-identical at every shape: one key, fewer keys than a 64-key chunk, exactly one chunk,
one key past a chunk, more keys than queries, several chunks, and the longest context (512 keys).
Outside the kernel's range (513 keys, head size 128) the planner must leave the chain to the unfused
nodes, whose batched f32 product is sequential too (16 or more queries and keys: k_bgemm_f32)."""
import numpy as np
import pytest

import attn_bias_chain as abc
import nodes as nd
import ttship

SHAPES = [(1, 1, 2, 64), (5, 5, 4, 64), (64, 64, 4, 64), (65, 65, 2, 64), (70, 3, 2, 64), (130, 130, 2, 64), (512, 40, 2, 64)]


def run_both(hip, P, n, H, hd, fusion=None, out_on=None):
    args = abc.inputs(P, n, H, hd)
    g1, g2 = nd.Graph(), nd.Graph()
    o1, o2 = abc.build(g1, *args, out_on=out_on), abc.build(g2, *args, out_on=out_on)
    stats = abc.plan(g1, fusion)
    if fusion is not None:
        hip.set_option(ttship.OPT["FUSION"], fusion)
    try:
        g1.run_hip(hip)
    finally:
        if fusion is not None:
            hip.set_option(ttship.OPT["FUSION"], ttship.FUSE_ALL)
    g2.run_oracle(n_threads=8)
    return abc.result(g1, o1), abc.result(g2, o2), stats


@pytest.mark.gpu
@pytest.mark.parametrize("out_on", ["q", "k", "v"])
@pytest.mark.parametrize("P,H", [(5, 4), (130, 2)])
def test_output_on_an_operands_memory(hip, P, H, out_on):
    """The graph's output tensor lies on the memory of q (the same rows: written in place), of k or of v (other
    workgroups still read them: written through the staging buffer): still fused, still the oracle's bits."""
    gpu, ref, st = run_both(hip, P, P, H, 64, out_on=out_on)
    assert st["attn"] == 1, st
    assert np.isfinite(ref).all()
    assert np.array_equal(gpu, ref), (np.abs(gpu - ref).max(), float(np.mean(gpu != ref)))


@pytest.mark.gpu
@pytest.mark.parametrize("P,n,H,hd", SHAPES)
def test_attn_bias_bit_identical_to_unfused_chain(hip, P, n, H, hd):
    gpu, ref, st = run_both(hip, P, n, H, hd)
    assert st["attn"] == 1, st
    assert np.isfinite(ref).all()
    assert np.array_equal(gpu, ref), (np.abs(gpu - ref).max(), float(np.mean(gpu != ref)))


@pytest.mark.gpu
@pytest.mark.parametrize("P,n,H,hd", [(513, 16, 2, 64), (40, 16, 2, 128)])
def test_outside_the_kernels_range_runs_unfused(hip, P, n, H, hd):
    gpu, ref, st = run_both(hip, P, n, H, hd)
    assert st["attn"] == 0, st
    assert np.array_equal(gpu, ref), (np.abs(gpu - ref).max(), float(np.mean(gpu != ref)))


@pytest.mark.gpu
def test_fused_equals_unfused_on_the_device(hip):
    """P = 65 with TTS_FUSE_ATTN off (five launches) against the fused launch: the same bits."""
    fused, ref, st = run_both(hip, 65, 65, 2, 64)
    unfused, _, st_off = run_both(hip, 65, 65, 2, 64, fusion=ttship.FUSE_ALL & ~ttship.FUSE["ATTN"])
    assert st["attn"] == 1 and st_off["attn"] == 0
    assert np.array_equal(fused, unfused)
    assert np.array_equal(fused, ref)
