"""Coalesced decode steps on a Q4_K_M-style mix file, in the shape of tests/test_coalesce_paths_gpu.py (whose helpers
this module uses): n one-prompt Parler runners from the file, each on its own backend and thread, prompts of n lengths,
8 decode steps.  A layer's q / k / v group holds a Q6_K v_proj beside Q4_K q_proj and k_proj, and each member's K and V
rows go to its own cache through the GEMV job's per-column store offsets, which have to survive the Q6_K kernel too.
Each step's logits must equal the same runner's when it runs alone, and the coalescer's counters must show shared
launches."""
import pathlib
import tempfile

import numpy as np
import pytest

import py_oracle
import q6_k_ref as q6
import test_coalesce_paths_gpu as cp
import ttship
from test_coalesce_gpu import prompt
from test_coalesce_paths_gpu import coalescer_on  # noqa: F401 -- autouse fixture

Q6, Q4K, F32 = ttship.Q6_K, ttship.Q4_K, ttship.F32
SHAPE = dict(cp.H256, n_layers=8)  # more_bits(i, 8): layers 0, 3, 6, 7 hold Q6_K v_proj and fc2


def host_rows(ty, x):
    return q6.quantize_row_q6_K(x) if ty == Q6 else py_oracle.quantize(ty, x)


@pytest.fixture(scope="module")
def mix_file():
    with tempfile.TemporaryDirectory() as d:
        p = pathlib.Path(d)
        cfg = ttship.parler_config(weight_type=F32, **dict(cp.BASE, **SHAPE))
        ttship.write_parler_synthetic_gguf(p / "f32.gguf", cfg)
        ttship.quantize_gguf(p / "f32.gguf", p / "mix.gguf", ttship.quantize_params(Q4K, mix=ttship.QUANT_MIX_Q4_K_M, quantize_output_heads=1),
                             rows_fn=host_rows)
        yield p / "mix.gguf"


def runner(iface, path):
    with ttship.Gguf(path) as g:
        cfg = ttship.parler_config_from_gguf(g, max_ctx=cp.BASE["max_ctx"], batch=1)
        assert (cfg.weight_type, cfg.head_type) == (Q4K, Q6) and g.tensor_type("decoder.layers.0.self_attn.v_proj.weight") == Q6
        return ttship.Parler(iface, cfg, gguf=g), cfg


def alone(path, r):
    """(inputs [steps, heads], logits [steps, heads, vocab]) of runner r's greedy run on a backend of its own, alone."""
    be = ttship.HipBackend(0)
    try:
        run, cfg = runner(be.iface(reference_flow=True), path)
        try:
            run.prefill(prompt(r, 5 + r))
            tok = np.zeros((cp.STEPS, cfg.n_output_heads), dtype=np.int32)
            logits = []
            for s in range(cp.STEPS):
                logits.append(run.decode(cp.step_inputs(cfg, tok[:s + 1])[s])[0])
                tok[s] = logits[s].argmax(axis=1)
            return cp.step_inputs(cfg, tok), np.stack(logits)
        finally:
            run.close()
    finally:
        be.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_coalesced_mix_file_matches_each_runner_alone(mix_file, n):
    prev = ttship.coalesce_enable(False)
    try:
        refs = [alone(mix_file, r) for r in range(n)]
    finally:
        ttship.coalesce_enable(prev)
    bes = [ttship.HipBackend(0) for _ in range(n)]
    its = [b.iface(reference_flow=True) for b in bes]
    try:
        got, before, after = cp.serve_logits(lambda i: runner(its[i], mix_file)[0], lambda run, i: run.prefill(prompt(i, 5 + i)),
                                             lambda run, i, s: run.decode(refs[i][0][s])[0], n, cp.STEPS)
    finally:
        for b in bes:
            b.close()
    carried = after["member_steps"] - before["member_steps"]
    diff = cp.first_difference(got, [ref[1] for ref in refs])
    print(f"coalesced: member_steps +{carried}, launches +{after['launches'] - before['launches']}; first difference {diff}")
    assert diff is None, f"logits differ from the runner alone first at (step, member, count, max abs) {diff}"
    assert np.all(np.isfinite(refs[0][1]))
    assert carried >= n * cp.STEPS // 2, f"{before} {after}"  # most steps ran coalesced
