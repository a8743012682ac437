"""Decode attention on the device (k_attn.hip) over the declared case list (attn_matrix), every case under the
default options and, past 64 keys, under every kernel choice the options offer (attn_matrix.Case.modes), compared with

  attn_ref  (numpy, shares nothing with the kernels or the oracle) at the case's bar: bit equality where every sum
            is sequential, at most 1 ulp with >= 99.9 % of the elements bit-equal elsewhere, the derived absolute
            bound for the `large` score range (attn_ref's docstring);
  the oracle's unfused chain at the same bar (the suite's standing attention bar), NaN for NaN on a fully masked row;
  its clean twin, bit for bit, where the memory past the window is NaN (a poison case).

The output buffer holds 0xFF bytes before every run, and every element of it must have been written.  With -s each
run prints how many elements differ from attn_ref and the worst ulp.
"""
import ctypes

import numpy as np
import pytest

import attn_matrix as am
import attn_ref
import ttship
from test_attn_gpu import set_mode
from test_attn_ref_cpu import dead_rows_match


def run(hip, case, mode, one):
    """split_uv16: split_pv16's options with ATTN_PV16 on (k_attn_pv<true, 16>, backend default off)."""
    set_mode(hip, "split_pv16" if mode == "split_uv16" else mode)
    hip.set_option(ttship.OPT["ATTN_PV16"], 1 if mode == "split_uv16" else 0)
    hip.set_option(ttship.OPT["ATTN_ONE"], one)
    try:
        got = am.run_device(case, hip)
    finally:
        set_mode(hip, "default")
        hip.set_option(ttship.OPT["ATTN_PV16"], 0)
        hip.set_option(ttship.OPT["ATTN_ONE"], ttship.ATTN_ONE_DEFAULT)
    assert not (got.view(np.uint32) == 0xFFFFFFFF).any(), f"{case.id} [{mode}, ATTN_ONE {one}]: an output element was not written"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", am.CASES, ids=am.IDS)
def test_attn_matrix(hip, case):
    ref = am.reference(case)
    orc, stats = am.oracle(case)
    if stats is not None:
        assert stats["attn"] == (1 if case.fuses else 0), (case.id, stats)
    orc_ref = attn_ref.Result(orc, ref.wmax, ref.pav, ref.dead)
    for mode, one in case.modes():
        tag = f"{case.id} [{mode}, ATTN_ONE {one}]"
        got = run(hip, case, mode, one)
        attn_ref.check(f"{tag} vs attn_ref", got, ref, case.bar)
        attn_ref.check(f"{tag} vs oracle", got, orc_ref, case.bar if case.fuses else "bits", verbose=False)   # unfused nodes: the oracle's bits
        dead_rows_match(case, got, ref, orc)
        if case.poison:
            clean = run(hip, am.twin(case), mode, one)
            assert np.array_equal(got.view(np.uint32), clean.view(np.uint32)), f"{tag}: memory past the window reached the output"


@pytest.mark.gpu
def test_abi_refuses_head_sizes_outside_the_kernels(hip):
    """tts_hip_attn_decode's own range check (the graph route's is the planner's, the refuse_* cases): head sizes that
    are no multiple of 4 or exceed 256 and more than 8192 keys return TTS_STATUS_BAD_ARG before anything is launched."""
    d = hip.alloc(1 << 16)
    try:
        for hd, P in ((260, 8), (6, 8), (64, 8193)):
            x = am.inputs(am.Case("abi_range", hd, P, route="abi"))
            tq, tk, tv = am._td(d, x.q), am._td(d, x.k), am._td(d, x.v)
            st = hip.L.tts_hip_attn_decode(hip.ptr, ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), None, 0, 0.125, d, None,
                                           None, None, None, None)
            assert st == -4, (hd, P, st)   # TTS_STATUS_BAD_ARG
    finally:
        hip.free(d)
