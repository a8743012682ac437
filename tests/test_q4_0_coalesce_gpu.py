"""Coalesced decode steps on Q4_0 weights, in the shape of tests/test_coalesce_paths_gpu.py (whose helpers this
module uses): n one-prompt Parler runners, each on its own backend from its own thread, prompts of n lengths, 8
decode steps.  Each member's K and V rows go to its own cache through the GEMV job's per-column store offsets,
which have to survive the Q4_0 kernels too.  The runners load a synthetic Q4_0 file with every d trimmed; each
step's logits must equal the CPU oracle's batch-1 run on the file's Q8_0 twin (tests/q4_0_ref.py, R2), and the
coalescer's counters must show shared launches."""
import pathlib
import tempfile

import numpy as np
import pytest

import py_oracle
import q4_0_ref as q4
import test_coalesce_paths_gpu as cp
import ttship
from test_coalesce_gpu import prompt
from test_coalesce_paths_gpu import coalescer_on  # noqa: F401 -- autouse fixture

Q4, Q8, F32 = ttship.Q4_0, ttship.Q8_0, ttship.F32
_FILES = {}  # shape -> (directory, trimmed Q4_0 file, its Q8_0 twin)
_REF = {}    # (shape, r) -> (inputs, logits), computed once and left unchanged
_ORACLE = {}


@pytest.fixture(scope="module", autouse=True)
def cleanup():
    yield
    for c in _ORACLE.values():
        c.close()
    _ORACLE.clear()
    for d, _, _ in _FILES.values():
        d.cleanup()
    _FILES.clear()


def files(shape):
    key = tuple(sorted(shape.items()))
    if key not in _FILES:
        d = tempfile.TemporaryDirectory()
        p = pathlib.Path(d.name)
        ttship.write_parler_synthetic_gguf(p / "synth.gguf", cp.parler_cfg(Q4, shape))
        q4.trim_gguf(p / "synth.gguf", p / "trim.gguf")
        q4.twin_gguf(p / "trim.gguf", p / "twin.gguf")
        _FILES[key] = (d, p / "trim.gguf", p / "twin.gguf")
    return _FILES[key][1:]


def runner(iface, shape, oracle=False):
    with ttship.Gguf(files(shape)[1 if oracle else 0]) as g:
        cfg = ttship.parler_config_from_gguf(g, max_ctx=cp.BASE["max_ctx"], batch=1)
        assert (cfg.weight_type, cfg.head_type) == (Q8 if oracle else Q4, F32)
        return ttship.Parler(iface, cfg, gguf=g)


def reference(shape, r):
    """cp.parler_reference for the twin file: runner r's batch-1 greedy run on the oracle, step by step."""
    key = tuple(sorted(shape.items()))
    if (key, r) not in _REF:
        cfg = cp.parler_cfg(Q4, shape)
        if key not in _ORACLE:
            _ORACLE[key] = runner(py_oracle.iface(8), shape, oracle=True)
        c, p = _ORACLE[key], prompt(r, 5 + r)
        drawn = None
        if r == 0:  # generate() itself must draw the tokens of the step-by-step run
            c.reset()
            c.prefill(p)
            drawn = c.generate(cp.STEPS)[0]
        c.reset()
        c.prefill(p)
        tok = np.zeros((cp.STEPS, cfg.n_output_heads), dtype=np.int32)
        logits = []
        for s in range(cp.STEPS):
            logits.append(c.decode(cp.step_inputs(cfg, tok[:s + 1])[s])[0])
            tok[s] = logits[s].argmax(axis=1)
        assert drawn is None or np.array_equal(tok, drawn)
        logits = np.stack(logits)
        logits.setflags(write=False)
        _REF[(key, r)] = (cp.step_inputs(cfg, tok), logits)
    return _REF[(key, r)]


# H256: the slab kernel with the LN / quantize prologue (12 members: 8 + 4 column chunks over it); H320 (K % 256 != 0):
# the general kernel k_gemv_b32<BlkQ4_0> at 3 members, and at 12 the K / V store runs on the matrix-core GEMM
# k_gemm_b32<BlkQ4_0>.  The ids are kept stable from when Q4_0 had kernels of its own (q4_0s: k_gemv_b32s)
@pytest.mark.gpu
@pytest.mark.parametrize("shape,n", [pytest.param(cp.H256, 3, id="h256-n3-k_gemv_q4_0s"), pytest.param(cp.H256, 12, id="h256-n12-k_gemv_q4_0s-chunks"),
                                     pytest.param(cp.H320, 3, id="h320-n3-k_gemv_q4_0"), pytest.param(cp.H320, 12, id="h320-n12-k_gemm_q4_0")])
def test_coalesced_q4_0_logits_match_oracle(shape, n):
    refs = [reference(shape, r) for r in range(n)]
    bes = [ttship.HipBackend(0) for _ in range(n)]
    its = [b.iface(reference_flow=True) for b in bes]
    if n > 8:
        ttship.coalesce_set_wait(50000)
    try:
        got, before, after = cp.serve_logits(lambda i: runner(its[i], shape), lambda run, i: run.prefill(prompt(i, 5 + i)),
                                             lambda run, i, s: run.decode(refs[i][0][s])[0], n, cp.STEPS)
    finally:
        if n > 8:
            ttship.coalesce_set_wait(5000)
        for b in bes:
            b.close()
    carried = after["member_steps"] - before["member_steps"]
    launches = after["launches"] - before["launches"]
    diff = cp.first_difference(got, [ref[1] for ref in refs])
    print(f"coalesced: member_steps +{carried}, launches +{launches}; first difference (step, member, count, max abs) {diff}")
    assert diff is None, f"logits differ from the oracle's first at (step, member, count, max abs) {diff}"
    assert carried >= n * cp.STEPS // 2, f"{before} {after}"  # most steps ran coalesced
    if n > 8:  # at least one launch carried more than 8 columns
        assert carried > 8 * launches, f"{before} {after}"
