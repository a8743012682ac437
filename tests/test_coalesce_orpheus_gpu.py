"""Coalesced decode steps of one-prompt Orpheus workers.

Every case is tests/test_coalesce_paths_gpu.py's pattern on Orpheus runners: n workers, each with its own
backend and thread, prompts of n different lengths (so every member has its own rope position, its own
cache rows and its own key count), a barrier after the prefills, then 8 teacher-forced decode steps
through Orpheus.decode under reference_flow (graph_compute, logits read back at once).  The tokens fed
are the argmax of the same runner's logits when it runs alone with the coalescer off, so no run can
diverge through a near-tie.  Per case:

  (a) every step's logits are np.array_equal to that runner's run alone on the HIP backend with the
      coalescer off (same config, weights seed, prompt and tokens): the coalescer's contract;
  (b) for Q4_K, Q8_0 and F32 weights (not the Q4_K_M-style mix: the oracle has no Q6_K), argmax equal to and logits within 1e-4 * max|logit| + 1e-4 of the
      CPU oracle's batch-1 run (tests/test_orpheus_gpu.py's bar); array_equal where the case says the
      uncoalesced runner is the oracle's bit for bit (tiny Q4_K, as the existing fall-back test asserts);
  (c) member_steps grows by at least n * 8 // 2: the steps were carried by shared launches;
  (d) at 12 members member_steps grows by more than 8 * launches: more than 8 columns were carried;
  (e) member_node_runs does not grow: no node of the steps ran once per member.

The host bounds check of the batched KV store (tts_hip_coalesce_store_ok) is tested without a device in
tests/test_coalesce_store_cpu.py."""
import threading

import numpy as np
import pytest

import py_oracle
import ttship
from test_coalesce_gpu import run_threads
from test_coalesce_paths_gpu import oracle_runners  # noqa: F401  (closes the Parler oracle runners run_parler_case opens)
from test_coalesce_paths_gpu import H256, first_difference, run_parler_case, serve_logits
from weights_pin import ORPHEUS_TINY

STEPS = 8
Q4_K, Q8_0, Q5_0, Q4_0, F16, F32 = ttship.Q4_K, ttship.Q8_0, ttship.Q5_0, ttship.Q4_0, ttship.F16, ttship.F32
ORACLE_TYPES = (Q4_K, Q8_0, F32)

TINY = dict(ORPHEUS_TINY)
# one layer at K = 2048 (the single-matrix split launches, the K relay), repeat = 4: all four CpyMulti destinations
WIDE = dict(n_layers=1, hidden_size=2048, n_attn_heads=16, n_kv_attn_heads=4, head_size=128, ffn_size=2048, vocab_size=1000, max_ctx=48)
# repeat = 3, real Orpheus' ratio: an odd destination count
REP3 = dict(n_layers=1, hidden_size=768, n_attn_heads=6, n_kv_attn_heads=2, head_size=128, ffn_size=1024, vocab_size=1000, max_ctx=48)
# tests/test_orpheus_gpu.py::test_orpheus_hd128_mid_context's config
HD128 = dict(n_layers=1, hidden_size=512, n_attn_heads=4, n_kv_attn_heads=2, head_size=128, ffn_size=512, vocab_size=1000, max_ctx=160)


@pytest.fixture(autouse=True)
def coalescer_on():
    prev = ttship.coalesce_enable(True)
    yield
    ttship.coalesce_enable(prev)


def prompt(r, n, V):
    return ((np.arange(n, dtype=np.int32) * (7919 + 2 * r) + 3 + r) % V).reshape(1, -1)


def backend(tile_bytes):
    """A backend whose Q4_K matrices all go to the tile layout when tile_bytes = 1 (set before the runner is
    created, as test_orpheus_tiny_all_tiled does)."""
    be = ttship.HipBackend(0)
    if tile_bytes is not None:
        be.set_option(ttship.OPT["Q4K_TILE_BYTES"], tile_bytes)
    return be


_REF = {}  # (config, tile_bytes, r, prompt length) -> (tokens fed [STEPS], the runner's logits alone [STEPS]), left unchanged
_ORA = {}  # (config, r, prompt length) -> the oracle's logits [STEPS] on its own argmax


def key_of(kw):
    return tuple(sorted(kw.items()))


def alone_reference(kw, tile_bytes, r, plen):
    """Runner r alone on the HIP backend with the coalescer off: the tokens it feeds (the argmax of its own
    logits, from the prompt's on) and its logits at every step."""
    k = (key_of(kw), tile_bytes, r, plen)
    if k not in _REF:
        cfg = ttship.orpheus_config(batch=1, **kw)
        prev = ttship.coalesce_enable(False)
        be = backend(tile_bytes)
        try:
            g = ttship.Orpheus(be.iface(reference_flow=True), cfg)
            try:
                lg = [g.prefill(prompt(r, plen, cfg.vocab_size))]
                for s in range(STEPS):
                    lg.append(g.decode(lg[-1].argmax(axis=1).astype(np.int32)))
            finally:
                g.close()
        finally:
            be.close()
            ttship.coalesce_enable(prev)
        toks = [l.argmax(axis=1).astype(np.int32) for l in lg[:-1]]
        for l in lg:
            l.setflags(write=False)
        _REF[k] = (toks, lg[1:])
    return _REF[k]


def oracle_reference(kw, r, plen):
    k = (key_of(kw), r, plen)
    if k not in _ORA:
        cfg = ttship.orpheus_config(batch=1, **kw)
        c = ttship.Orpheus(py_oracle.iface(8), cfg)
        try:
            lg = [c.prefill(prompt(r, plen, cfg.vocab_size))]
            for s in range(STEPS):
                lg.append(c.decode(lg[-1].argmax(axis=1).astype(np.int32)))
        finally:
            c.close()
        for l in lg:
            l.setflags(write=False)
        _ORA[k] = lg[1:]
    return _ORA[k]


def serve(kw, tile_bytes, lens, steps_of=None):
    """The members' coalesced run: [member][step] logits (None past a member's own step count) and the counters."""
    n = len(lens)
    cfg = ttship.orpheus_config(batch=1, **kw)
    refs = [alone_reference(kw, tile_bytes, r, lens[r]) for r in range(n)]
    bes = [backend(tile_bytes) for _ in range(n)]
    if n > 8:
        ttship.coalesce_set_wait(50000)
    try:
        def step(run, i, s):
            if steps_of is not None and s >= steps_of[i]:
                return None
            return run.decode(refs[i][0][s])

        got, before, after = serve_logits(lambda i: ttship.Orpheus(bes[i].iface(reference_flow=True), cfg),
                                          lambda run, i: run.prefill(prompt(i, lens[i], cfg.vocab_size), want_logits=False), step, n, STEPS)
    finally:
        if n > 8:
            ttship.coalesce_set_wait(5000)
        for b in bes:
            b.close()
    return got, refs, before, after


def check_oracle(kw, lens, got, exact):
    tol_of = lambda ref: 1e-4 * np.abs(ref).max() + 1e-4
    for r in range(len(lens)):
        ora = oracle_reference(kw, r, lens[r])
        for s in range(STEPS):
            if got[r][s] is None:
                continue
            assert np.array_equal(got[r][s].argmax(axis=1), ora[s].argmax(axis=1)), f"member {r} step {s}: argmax differs from the oracle's"
            d = float(np.abs(got[r][s].astype(np.float64) - ora[s]).max())
            assert d <= tol_of(ora[s]), f"member {r} step {s}: max |logit - oracle| {d} > {tol_of(ora[s])}"
            if exact:
                assert np.array_equal(got[r][s], ora[s]), f"member {r} step {s}: logits differ from the oracle's (max abs {d})"


def run_case(kw, n, tile_bytes=None, lens=None, exact_oracle=False):
    lens = lens or [4 + 2 * r for r in range(n)]
    got, refs, before, after = serve(kw, tile_bytes, lens)
    delta = {k: after[k] - before[k] for k in after}
    diff = first_difference(got, [ref[1] for ref in refs])
    print(f"coalesced orpheus: {delta}; first difference from the runner alone (step, member, count, max abs) {diff}")
    assert diff is None, f"logits differ from the runner's own run alone first at (step, member, count, max abs) {diff}"  # (a)
    if kw.get("weight_type", Q4_K) in ORACLE_TYPES and not kw.get("weight_mix"):  # (the oracle has no Q6_K dot product)
        check_oracle(kw, lens, got, exact_oracle)  # (b)
    assert delta["member_steps"] >= n * STEPS // 2, f"{before} {after}"  # (c)
    if n > 8:
        assert delta["member_steps"] > 8 * delta["launches"], f"{before} {after}"  # (d)
    assert delta["member_node_runs"] == 0, f"{before} {after}"  # (e)


# A: Q4_K lane layout: the unfused SiLU / MUL per-slice path, the KV store and rope forms, the chunk loop at 12
@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 12])
def test_tiny_q4k_lane(n):
    run_case(dict(TINY, weight_type=Q4_K), n, exact_oracle=True)


# B: every Q4_K matrix tiled: the SwiGLU form at <= 8 columns and above, the 1000-row vocabulary on the tiled head
@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 8, 12])
def test_tiny_q4k_all_tiled(n):
    run_case(dict(TINY, weight_type=Q4_K), n, tile_bytes=1)


# C: the SiLU-mul form on the slab kernel and over chunks
@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 12])
@pytest.mark.parametrize("wtype", [Q8_0, Q5_0, Q4_0], ids=["q8_0", "q5_0", "q4_0"])
def test_tiny_block32(wtype, n):
    run_case(dict(TINY, weight_type=wtype), n)


# D: float weights
@pytest.mark.gpu
@pytest.mark.parametrize("wtype", [F16, F32], ids=["f16", "f32"])
def test_tiny_float(wtype):
    run_case(dict(TINY, weight_type=wtype), 3)


# E: K = 2048, repeat = 4: the split launches with per-member store offsets (lane layout), the K relay with the
# SwiGLU launch beside it (all tiled, 8 members)
@pytest.mark.gpu
@pytest.mark.parametrize("n,tile_bytes", [(3, None), (8, 1)], ids=["lane-n3", "tiled-n8"])
def test_wide_repeat4(n, tile_bytes):
    run_case(dict(WIDE, weight_type=Q4_K), n, tile_bytes=tile_bytes)


# F: repeat = 3
@pytest.mark.gpu
def test_repeat3():
    run_case(dict(REP3, weight_type=Q4_K), 3)


# G: a Q6_K v_proj between the Q4_K k_proj and q_proj, a Q6_K down_proj and head
@pytest.mark.gpu
def test_tiny_q4_k_m_mix():
    run_case(dict(TINY, weight_type=Q4_K, weight_mix=ttship.QUANT_MIX_Q4_K_M), 3)


# H: members cross the attention kernels' 64-key boundary at different steps, at different rope positions
@pytest.mark.gpu
def test_hd128_across_64_keys():
    run_case(dict(HD128, weight_type=Q4_K), 3, lens=[60, 63, 66])


# I: a member leaves; the others keep coalescing
@pytest.mark.gpu
def test_member_leaves():
    kw, lens, left = dict(TINY, weight_type=Q4_K), [4, 6, 8, 10], 3
    got, refs, before, after = serve(kw, None, lens, steps_of=[STEPS, STEPS, STEPS, left])
    delta = {k: after[k] - before[k] for k in after}
    print(f"member leaves: {delta}")
    for r in range(4):
        for s in range(STEPS if r < 3 else left):
            assert np.array_equal(got[r][s], refs[r][1][s]), f"member {r} step {s}"
    assert all(g is None for g in got[3][left:])
    # more than the first `left` steps of four could have carried: the three went on sharing launches
    assert delta["member_steps"] >= 4 * left + 3 * (STEPS - left) // 2, f"{before} {after}"
    assert delta["member_node_runs"] == 0, f"{before} {after}"


# J: Orpheus and Parler workers at once: each kind coalesces with its own, neither ends up refused for good
@pytest.mark.gpu
def test_orpheus_and_parler_together():
    kw = dict(TINY, weight_type=Q4_K)
    res, err = {}, []

    def orpheus():
        try:
            res["o"] = serve(kw, None, [4, 6])
        except BaseException as e:  # noqa: BLE001
            err.append(e)

    for r in range(2):
        alone_reference(kw, None, r, 4 + 2 * r)
    before = ttship.coalesce_stats(0)
    t = threading.Thread(target=orpheus)
    t.start()
    try:
        run_parler_case(Q4_K, H256, 2)  # asserts its own logits (the oracle's) and that its steps were carried
    finally:
        t.join()
    assert not err, err
    got, refs, _, _ = res["o"]
    assert first_difference(got, [ref[1] for ref in refs]) is None
    mid = ttship.coalesce_stats(0)
    assert mid["launches"] > before["launches"]
    # afterwards each kind still coalesces on its own: neither signature was marked as having no coalesced form
    got, refs, b, a = serve(kw, None, [4, 6])
    assert first_difference(got, [ref[1] for ref in refs]) is None
    assert a["member_steps"] - b["member_steps"] >= 2 * STEPS // 2, f"{b} {a}"
    assert a["member_node_runs"] == b["member_node_runs"]
    mid = ttship.coalesce_stats(0)
    run_parler_case(Q4_K, H256, 2)
    assert ttship.coalesce_stats(0)["launches"] > mid["launches"]
