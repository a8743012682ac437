"""Coalesced decode steps on every route through launch_gemv_job (tts.cpp_amd/csrc/k_gemv.hip).

In a coalesced step each member's self-attention K and V rows go to that member's own cache through
the GEMV job's per-column store offsets (GemvJob::yoff / yoff_ld / yoff_mats, filled in
run_gemv_item / co_prepare, applied in gemv_put).  The offsets have to survive every route a job can
take: the split into single-matrix launches, the 8-column chunk loop, the tile-layout matrix-core
kernels, the K-relay GEMM, the Q8_0 / Q5_0 slab, general and matrix-core GEMM kernels, the float GEMV
and the F32 tiled GEMM.  Each case below is chosen from the dispatch conditions so that its q / k / v
group takes one of those routes (the kernel named in the case id is the one the coalesced K / V store
runs on).

Every case: one layer, n one-prompt Parler runners, each on its own backend from its own thread
(TTS.cpp's server shape), prompts of n different lengths -- so every member sits at its own KV
position and needs its own store offset -- released together by a barrier after their prefills, then
8 decode steps through Parler.decode (graph_compute, logits read back at once: the path the
coalescer serves) on the CPU oracle's tokens.  Every step's [n_output_heads, output_vocab] logits
must equal (np.array_equal, no tolerance) the oracle's batch-1 run of the same runner on the same
tokens: a wrong cache row can leave an argmax unchanged for a step or two, the logits not.  The
coalescer's counters must show that the steps were carried by shared launches and, at 12 members,
that launches of more than 8 columns ran.  Parler.decode under reference_flow does reach the
coalescer (member_steps grows by n * 8 less the first, unaligned step), so no case falls back to
generate() and token equality.  The oracle has no Q5_0 dot product: the Q5_0 cases run it on the
Q8_0 twin of the same weights (q5_files), as tests/test_q5_0_gpu.py does.

The kernels named in the case ids were confirmed once with a kernel trace of this module, one
traced process per case, reading the launches on the coalescer's executor stream."""
import pathlib
import tempfile
import threading

import numpy as np
import pytest

import py_oracle
import q5_0_ref
import ttship
from test_coalesce_gpu import prompt, run_threads
from weights_pin import ORPHEUS_TINY

STEPS = 8
BASE = dict(n_layers=1, output_vocab=1088, prompt_vocab=512, max_ctx=128, max_positions=160, batch=1, head_type=ttship.F32)
H2048 = dict(hidden_size=2048, n_attn_heads=32, ffn_size=2048)
H256 = dict(hidden_size=256, n_attn_heads=4, ffn_size=1024)
H320 = dict(hidden_size=320, n_attn_heads=5, ffn_size=1024)


@pytest.fixture(autouse=True)
def coalescer_on():
    """The coalescer is on by default (tts_hip_coalesce_enable); kept on for these tests whatever the
    environment says, then back to what it was."""
    prev = ttship.coalesce_enable(True)
    yield
    ttship.coalesce_enable(prev)


def parler_cfg(wtype, shape):
    return ttship.parler_config(weight_type=wtype, **BASE, **shape)


_REF = {}     # (weights, shape, r) -> (inputs, logits), shared by the cases and left unchanged
_ORACLE = {}  # (weights, shape) -> the oracle's runner (one set of weights for every r)
_Q5 = {}      # shape -> (directory, the synthetic weights as a Q5_0 file, its Q8_0 twin)


@pytest.fixture(scope="module", autouse=True)
def oracle_runners():
    yield
    for c in _ORACLE.values():
        c.close()
    _ORACLE.clear()
    for d, _, _ in _Q5.values():
        d.cleanup()
    _Q5.clear()


def q5_files(shape):
    """The oracle has no Q5_0 dot: it runs the Q8_0 twin of the same weights (tests/q5_0_ref.py: the same d,
    quants q - 16; ggml's Q5_0 x Q8_0 and Q8_0 x Q8_0 dots round alike), as tests/test_q5_0_gpu.py does.  The
    synthetic Q5_0 weights go to a file, the HIP runners load it and the oracle loads its twin."""
    key = tuple(sorted(shape.items()))
    if key not in _Q5:
        d = tempfile.TemporaryDirectory()
        dev, twin = pathlib.Path(d.name) / "parler-q5_0.gguf", pathlib.Path(d.name) / "parler-q5_0-twin.gguf"
        ttship.write_parler_synthetic_gguf(dev, parler_cfg(ttship.Q5_0, shape))
        q5_0_ref.twin_gguf(dev, twin)
        _Q5[key] = (d, dev, twin)
    return _Q5[key][1:]


def parler_runner(iface, wtype, shape, oracle=False):
    """A one-prompt runner of the case's model on `iface` (oracle: the CPU oracle's copy of the weights)."""
    if wtype != ttship.Q5_0:
        return ttship.Parler(iface, parler_cfg(wtype, shape))
    with ttship.Gguf(q5_files(shape)[1 if oracle else 0]) as g:
        cfg = ttship.parler_config_from_gguf(g, max_ctx=BASE["max_ctx"], batch=1)
        assert (cfg.weight_type, cfg.head_type) == (ttship.Q8_0 if oracle else ttship.Q5_0, ttship.F32)
        return ttship.Parler(iface, cfg, gguf=g)


def step_inputs(cfg, tokens):
    """The tokens tts_parler_generate feeds at each step (next_decoder_token_ids: BOS until step > head,
    then the head's last token, EOS once the head has produced EOS), from the tokens [steps, heads] it drew."""
    steps, nh = tokens.shape
    inp = np.empty((steps, nh), dtype=np.int32)
    seen = np.zeros(nh, dtype=bool)
    for s in range(steps):
        for h in range(nh):
            inp[s, h] = cfg.bos_token if s <= h else cfg.eos_token if seen[h] else tokens[s - 1, h]
        seen |= tokens[s] == cfg.eos_token
    return inp


def parler_reference(wtype, shape, r):
    """(inputs [steps, heads], logits [steps, heads, vocab]) of runner r's own batch-1 greedy run on the
    CPU oracle, computed once per (weights, shape, r).  The run is generate()'s, taken step by step with
    decode() so that the logits are kept: the tokens are sampler::max's (first maximum) and the inputs
    generate()'s rule (step_inputs); for each model's first runner generate() itself is run first and
    must have drawn the same tokens."""
    kind = (wtype, tuple(sorted(shape.items())))
    if kind + (r,) not in _REF:
        cfg = parler_cfg(wtype, shape)
        if kind not in _ORACLE:
            _ORACLE[kind] = parler_runner(py_oracle.iface(8), wtype, shape, oracle=True)
        c, p = _ORACLE[kind], prompt(r, 5 + r)
        drawn = None
        if r == 0:
            c.reset()
            c.prefill(p)
            drawn = c.generate(STEPS)[0]
        c.reset()
        c.prefill(p)
        tok = np.zeros((STEPS, cfg.n_output_heads), dtype=np.int32)
        logits = []
        for s in range(STEPS):
            logits.append(c.decode(step_inputs(cfg, tok[:s + 1])[s])[0])
            tok[s] = logits[s].argmax(axis=1)
        assert drawn is None or np.array_equal(tok, drawn)
        logits = np.stack(logits)
        logits.setflags(write=False)
        _REF[kind + (r,)] = (step_inputs(cfg, tok), logits)
    return _REF[kind + (r,)]


def serve_logits(make, prefill, step, n, steps):
    """n runners (make(i)), each prefilled (prefill(run, i)) and stepped (step(run, i, s) -> logits) from its
    own thread, the threads released together after all prefills; returns [runner][step] logits and
    the coalescer's counters before and after."""
    runs = [make(i) for i in range(n)]
    out = [[None] * steps for _ in range(n)]
    gate = threading.Barrier(n)
    try:
        before = ttship.coalesce_stats(0)

        def go(i):
            try:
                prefill(runs[i], i)
            except BaseException:
                gate.abort()
                raise
            gate.wait()
            for s in range(steps):
                out[i][s] = step(runs[i], i, s)

        run_threads(go, n)
        after = ttship.coalesce_stats(0)
    finally:
        for r in runs:
            r.close()
    return out, before, after


def first_difference(got, refs):
    """(step, member, differing logits, max |difference|) of the earliest step whose logits differ, or None."""
    for s in range(len(got[0])):
        for r in range(len(got)):
            if not np.array_equal(got[r][s], refs[r][s]):
                d = np.abs(got[r][s].astype(np.float64) - refs[r][s])
                return s, r, int((got[r][s] != refs[r][s]).sum()), float(d.max())
    return None


def run_parler_case(wtype, shape, n, ifaces=None):
    refs = [parler_reference(wtype, shape, r) for r in range(n)]
    bes = [] if ifaces else [ttship.HipBackend(0) for _ in range(n)]
    its = ifaces or [b.iface(reference_flow=True) for b in bes]
    if n > 8:
        ttship.coalesce_set_wait(50000)
    try:
        got, before, after = serve_logits(lambda i: parler_runner(its[i], wtype, shape), lambda run, i: run.prefill(prompt(i, 5 + i)),
                                          lambda run, i, s: run.decode(refs[i][0][s])[0], n, STEPS)
    finally:
        if n > 8:
            ttship.coalesce_set_wait(5000)
        for b in bes:
            b.close()
    carried = after["member_steps"] - before["member_steps"]
    launches = after["launches"] - before["launches"]
    diff = first_difference(got, [ref[1] for ref in refs])
    print(f"coalesced: member_steps +{carried}, launches +{launches}, refused +{after['refused'] - before['refused']}, "
          f"alone +{after['alone'] - before['alone']}; first difference (step, member, count, max abs) {diff}")
    assert diff is None, f"logits differ from the oracle's first at (step, member, count, max abs) {diff}"
    assert carried >= n * STEPS // 2, f"{before} {after}"  # most steps ran coalesced
    if n > 8:  # at least one launch carried more than 8 columns
        assert carried > 8 * launches, f"{before} {after}"


Q4_K, Q8_0, Q5_0, F16, F32 = ttship.Q4_K, ttship.Q8_0, ttship.Q5_0, ttship.F16, ttship.F32

# (weights, shape, members): the id names the kernel the coalesced q / k / v group is meant to run on.  The Q8_0 / Q5_0
# ids are kept stable from when each format had kernels of its own: q8_0s / q5_0s is k_gemv_b32s, q8_0 / q5_0
# k_gemv_b32 and the gemm ids k_gemm_b32, over BlkQ8_0 / BlkQ5_0
CASES = [
    # lane layout, K >= 8 * QK_K: the q / k / v group split into single-matrix unique-load launches
    pytest.param(Q4_K, H2048, 3, id="q4k-h2048-n3-k_gemv_q4_K_u-split"),
    # tile-layout copies, three matrices in one matrix-core launch: launch_q4k_mf's operand pass (k_quant_mf)
    # and the K relay at <= 8 columns (the trace shows k_gemv_q4K_kr, neither k_gemv_q4K_ks nor _mf)
    pytest.param(Q4_K, H2048, 8, id="q4k-h2048-n8-k_gemv_q4K_kr-gemv"),
    # launch_gemm_q4k_kr, K / 256 = 8
    pytest.param(Q4_K, H2048, 12, id="q4k-h2048-n12-k_gemv_q4K_kr-gemm"),
    # the K relay refuses K / 256 = 1: the 8-column chunk loop (yoff + m0) over the lane-layout kernel
    pytest.param(Q4_K, H256, 12, id="q4k-h256-n12-k_gemv_q4_K-chunks"),
    # slab kernels with the LN / quantize prologue; 8 + 4 column chunks over them
    pytest.param(Q8_0, H256, 3, id="q8_0-h256-n3-k_gemv_q8_0s"),
    pytest.param(Q5_0, H256, 3, id="q5_0-h256-n3-k_gemv_q5_0s"),
    pytest.param(Q8_0, H256, 12, id="q8_0-h256-n12-k_gemv_q8_0s-chunks"),
    pytest.param(Q5_0, H256, 12, id="q5_0-h256-n12-k_gemv_q5_0s-chunks"),
    # K % 256 != 0: prepared Q8_0 operands, the general kernels; the matrix-core GEMMs above 8 columns
    pytest.param(Q8_0, H320, 3, id="q8_0-h320-n3-k_gemv_q8_0"),
    pytest.param(Q5_0, H320, 3, id="q5_0-h320-n3-k_gemv_q5_0"),
    pytest.param(Q8_0, H320, 12, id="q8_0-h320-n12-k_gemm_q8_0"),
    pytest.param(Q5_0, H320, 12, id="q5_0-h320-n12-k_gemm_q5_0"),
    # float GEMV, chunked at 12 (F16); the F32 tiled GEMM above 8 columns
    pytest.param(F16, H256, 3, id="f16-h256-n3-k_gemv_float"),
    pytest.param(F16, H256, 12, id="f16-h256-n12-k_gemv_float-chunks"),
    pytest.param(F32, H256, 3, id="f32-h256-n3-k_gemv_float"),
    pytest.param(F32, H256, 12, id="f32-h256-n12-k_gemm_f32_f64"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("wtype,shape,n", CASES)
def test_coalesced_logits_match_oracle(wtype, shape, n):
    run_parler_case(wtype, shape, n)


@pytest.mark.gpu
def test_async_uploads_before_compute_with_fence_skip():
    """The pre-launch fence skip (coalesce.hip, run_group): a member whose stream has drained is not
    fenced.  Two tiny Q4_K runners upload every step's inputs with the asynchronous set (the vtable's
    `set` slot holds set_async, so the uploads are still queued on the member's stream when graph_compute
    submits the step) with TTS_CO_FENCE_ALL unset: the logits stay the oracle's, bit for bit."""
    import os
    assert "TTS_CO_FENCE_ALL" not in os.environ
    bes = [ttship.HipBackend(0) for _ in range(2)]
    try:
        its = []
        for b in bes:
            asy = b.iface().set_async
            it = b.iface(reference_flow=True)
            it.set = asy
            its.append(it)
        run_parler_case(Q4_K, H256, 2, ifaces=its)
    finally:
        for b in bes:
            b.close()


@pytest.mark.gpu
def test_orpheus_workers_fall_back_and_parler_still_coalesces():
    """Three Orpheus workers (tiny Q4_K, batch 1, three prompt lengths) decoding from three threads:
    co_prepare refuses SiLU-mul / SwiGLU epilogues, so their steps run alone (whether they coalesced is
    not asserted); every runner's logits are the oracle's, no step fails, and a Parler pair started
    afterwards in the same process still coalesces."""
    n = 3
    cfg = ttship.orpheus_config(batch=1, weight_type=Q4_K, **ORPHEUS_TINY)
    V = cfg.vocab_size
    prompts = [((np.arange(4 + 2 * r, dtype=np.int32) * (7919 + 2 * r) + 3 + r) % V).reshape(1, -1) for r in range(n)]
    refs = []
    for r in range(n):
        c = ttship.Orpheus(py_oracle.iface(8), cfg)
        try:
            lg = [c.prefill(prompts[r])]
            for s in range(STEPS):
                lg.append(c.decode(lg[-1].argmax(axis=1).astype(np.int32)))
            refs.append(lg)
        finally:
            c.close()
    bes = [ttship.HipBackend(0) for _ in range(n)]
    first = [None] * n
    try:
        def prefill(run, i):
            first[i] = run.prefill(prompts[i])

        got, before, after = serve_logits(lambda i: ttship.Orpheus(bes[i].iface(reference_flow=True), cfg), prefill,
                                          lambda run, i, s: run.decode(refs[i][s].argmax(axis=1).astype(np.int32)), n, STEPS)
    finally:
        for b in bes:
            b.close()
    print("orpheus workers:", {k: after[k] - before[k] for k in ("launches", "member_steps", "alone", "refused")})
    for r in range(n):
        assert np.array_equal(first[r], refs[r][0]), f"runner {r}: prompt logits"
    diff = first_difference(got, [ref[1:] for ref in refs])
    assert diff is None, f"logits differ from the oracle's first at (step, member, count, max abs) {diff}"
    # a Parler pair afterwards still coalesces
    mid = ttship.coalesce_stats(0)
    run_parler_case(Q4_K, H256, 2)
    assert ttship.coalesce_stats(0)["launches"] > mid["launches"]
