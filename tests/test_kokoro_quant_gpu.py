"""Kokoro with Q8_0 / Q5_0 weights on the HIP backend: from GGUF files the quantize tool wrote, and synthetic.

Files.  The TINYQ F32 file (tts_kokoro_write_synthetic_gguf) is quantized to Q8_0 and Q5_0 on the device
(tts_hip_gguf_quantize); the bytes equal the host quantizers'.  The HIP backend runs from the Q8_0 and the Q5_0
file, the CPU oracle from the Q8_0 file and from the Q5_0 file's Q8_0 twin (tests/q5_0_ref.py), under
the bars of tests/test_kokoro_model_gpu.py (north_star): rounded lengths identical, hidden within
1e-3 * max(1, max|ref|), the main graph run from the oracle's durations with PCM within 1e-4 absolute,
run() = durations() + decode(); at fusion mask 0 too.  Synthetic Q8_0 runners are compared the same way (82M
widths included); the 82M Q5_0 case needs a 330 MB F32 file, its quantized copy and its twin, and is skipped.

Inputs.  An activation quantizer can turn a 1-ulp difference upstream into a flipped int8 level, and the F32
attention between ALBERT's quantized matrices legitimately differs by that much between two correct
implementations.  The issue's rule is to keep inputs on which the oracle's scalar and SIMD modes give identical
lengths and PCM within 1e-4 of each other.  The PCM half of that rule selects nothing: the two modes' PCM is
0.17-0.34 apart on every input tried, with F32 weights too (profiles/r03/simd_gap_cpu.jsonl: 0.28), because the
sine source integrates F0 in Hz over 600 samples a frame.  It is REPLACED here by: identical lengths and hidden
states within 1e-6 between the two modes, checked on the CPU before any GPU run
(profiles/r10/oracle_scalar_vs_simd_kokoro_q8_0.txt, ..._kokoro_files.txt).  Synthetic TINYQ: every seed tried
qualifies.  TINYQ files, n = 7: seed 0 puts the twin's two modes 0.055 apart and seed 4 the Q8_0 file's 0.069, seed 5
changes a length on the twin; seed 1 qualifies for both files, as does n = 13 seed 1.  82M widths, n = 6: of
seeds 1-8 only seed 1 qualifies (the others are 0.09-0.26 apart in the hidden states: a flipped level carried
through twelve ALBERT passes), so the 82M case rests on one input.  The PCM bar (1e-4) is asserted against the
scalar oracle, as the existing Kokoro tests assert it.
"""
import numpy as np
import pytest

import py_oracle
import q5_0_ref
import ttship
from test_kokoro_gguf_cpu import RUN, host_rows
from test_kokoro_model_cpu import tokens
from test_kokoro_quant_cpu import TINYQ, dequant, rule

F32, F16, Q8_0, Q5_0 = ttship.F32, ttship.F16, ttship.Q8_0, ttship.Q5_0
FUSE_LSTM = 64
CFGS = {"tinyq": dict(TINYQ), "kokoro82m": dict(max_tokens=16, max_total=64)}


def compare_with_oracle(hip, name, n, seed, mask=None, make=None):
    """make(iface, on_gpu) -> runner; default: synthetic Q8_0 runners of CFGS[name]."""
    toks = tokens(n, seed)
    if make is None:
        def make(iface, on_gpu):
            return ttship.Kokoro(iface, ttship.kokoro_config(**dict(CFGS[name], weight_type=Q8_0)))
    o = make(py_oracle.iface(16), False)
    g = make(hip.iface(), True)
    cfg = g.cfg
    if mask is not None:
        hip.set_option(0, mask)
    try:
        ho, lo = o.durations(toks)
        c0 = hip.counters()
        hg, lg = g.durations(toks)
        c1 = hip.counters()
        herr = float(np.max(np.abs(hg - ho)))
        print(f"kokoro {name} n={n} lengths {lo.astype(int).tolist()} hidden max err {herr:.3e}")
        assert np.array_equal(lg, lo), (lg, lo)
        assert herr <= 1e-3 * max(1.0, float(np.max(np.abs(ho))))
        total = int(lo.sum())
        rand = np.random.default_rng(seed + 7).random((cfg.gen.harmonic_num + 1, 600 * total), dtype=np.float32)
        pg = g.decode(toks, ho, lo, rand)
        po = o.decode(toks, ho, lo, rand)
        assert pg.shape == po.shape == (600 * total,)
        assert np.all(np.isfinite(pg))
        err = float(np.max(np.abs(pg.astype(np.float64) - po)))
        print(f"kokoro {name} total {total} frames pcm max err {err:.3e} (peak {float(np.max(np.abs(po))):.3f})")
        assert err <= 1e-4, f"max |pcm_gpu - pcm_oracle| = {err:.3e}"
        assert float(np.std(po)) > 1e-2
        a = g.run(toks)
        b = g.decode(toks, hg, lg)
        assert np.array_equal(a, b) and np.array_equal(a, g.run(toks))
        return cfg, c1["lstm_steps"] - c0["lstm_steps"]
    finally:
        hip.set_option(0, ttship.FUSE_ALL)
        g.close()
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,seed", [("tinyq", 7, 0), ("tinyq", 13, 1), ("kokoro82m", 6, 1)])
def test_kokoro_q8_0_matches_oracle(hip, name, n, seed):
    cfg, steps = compare_with_oracle(hip, name, n, seed)
    # the duration graph: n_dur_layers + 1 bidirectional LSTMs, every chain fused and every pair in one launch
    n_lstm = cfg.n_dur_layers + 1
    assert steps == 2 * n * n_lstm


@pytest.mark.gpu
def test_kokoro_q8_0_matches_oracle_without_fusions(hip):
    compare_with_oracle(hip, "tinyq", 7, 0, mask=0)


@pytest.fixture(scope="module")
def files(hip, tmp_path_factory):
    """TINYQ: the F32 file, its device- and host-quantized Q8_0 / Q5_0 copies, the Q5_0 file's Q8_0 twin."""
    d = tmp_path_factory.mktemp("kokoro_q")
    out = {"f32": d / "f32.gguf"}
    ttship.write_kokoro_synthetic_gguf(out["f32"], ttship.kokoro_config(**TINYQ))
    for name, qt in (("q8_0", Q8_0), ("q5_0", Q5_0)):
        out[name], out[name + "_host"] = d / f"{name}.gguf", d / f"{name}-host.gguf"
        ttship.quantize_gguf(out["f32"], out[name], ttship.quantize_params(qt), backend=hip)
        ttship.quantize_gguf(out["f32"], out[name + "_host"], ttship.quantize_params(qt), rows_fn=host_rows)
    out["twin"] = d / "q5_0-twin.gguf"
    q5_0_ref.twin_gguf(out["q5_0"], out["twin"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,qt", [("q8_0", Q8_0), ("q5_0", Q5_0)])
def test_kokoro_file_device_quantizer_equals_host(files, name, qt):
    with ttship.Gguf(files[name]) as a, ttship.Gguf(files[name + "_host"]) as b:
        ta, tb = a.tensors(), b.tensors()
        assert [t[:3] for t in ta] == [t[:3] for t in tb]
        assert sum(1 for t in ta if t[1] == qt) == 6 + 2 + 16 * 6 and {t[1] for t in ta} == {F32, qt}
        for t in ta:
            assert np.array_equal(a.tensor_bytes(t[0]), b.tensor_bytes(t[0])), t[0]
    if qt == Q5_0:
        with ttship.Gguf(files["twin"]) as t:
            assert {x[1] for x in t.tensors()} == {F32, Q8_0}


def file_runners(files, name):
    """HIP from the quantized file; the oracle from the Q8_0 file, or from the Q5_0 file's twin."""
    def make(iface, on_gpu):
        with ttship.Gguf(files[name if on_gpu or name == "q8_0" else "twin"]) as g:
            return ttship.Kokoro.from_gguf(iface, g, **RUN)
    return make


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["q8_0", "q5_0"])
@pytest.mark.parametrize("n,seed,mask", [(7, 1, None), (13, 1, None), (7, 1, 0), (13, 1, 0)])
def test_kokoro_quant_file_matches_oracle(hip, files, name, n, seed, mask):
    cfg, steps = compare_with_oracle(hip, f"file-{name}", n, seed, mask=mask, make=file_runners(files, name))
    assert steps == (2 * n * (cfg.n_dur_layers + 1) if mask is None else 0)


@pytest.mark.gpu
def test_kokoro_q5_0_82m_file_matches_oracle_on_the_twin():
    """Kokoro-82M widths, Q5_0, n = 6: the twin is made from a file, and this one is 82 M weights in F32."""
    cfg = ttship.kokoro_config(max_tokens=16, max_total=64)
    hid, H2, DS = cfg.hidden, cfg.d_model // 2, cfg.d_model + cfg.gen.style_dim
    lower_bound = 4 * (4 * hid * hid + 2 * hid * cfg.ffn + 4 * 8 * H2 * (DS + H2) + 4 * 3 * 3 * (cfg.dec_dim + 66) * cfg.dec_dim)
    assert lower_bound > 100e6  # ALBERT, four of the six LSTM cells and the decoder's conv1 kernels alone
    pytest.skip("the 82M F32 file is about 330 MB (and needs a Q5_0 copy and a twin beside it): more than a test run should write; "
                "Q5_0 runs from files at TINYQ, and the 82M widths run with Q8_0 (synthetic) against the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("wtype", [Q8_0, Q5_0])
@pytest.mark.parametrize("name,n,seed", [("tinyq", 7, 0), ("tinyq", 13, 1), ("kokoro82m", 6, 1)])
def test_kokoro_quant_fused_lstm_changes_no_bit(hip, name, n, seed, wtype):
    """Both graphs with the LSTM fusion on and off (every other fusion as it is): identical lengths, hidden
    states and PCM, and the planner leaves no LSTM chain of the quantized duration graph unfused."""
    cfg = ttship.kokoro_config(**dict(CFGS[name], weight_type=wtype))
    toks = tokens(n, seed)
    g = ttship.Kokoro(hip.iface(), cfg)
    try:
        c0 = hip.counters()
        h, l = g.durations(toks)
        c1 = hip.counters()
        n_lstm = cfg.n_dur_layers + 1
        assert c1["lstm_steps"] - c0["lstm_steps"] == 2 * n * n_lstm
        assert c1["lstm_chains"] - c0["lstm_chains"] == 2 * n_lstm
        # a paired bidirectional cell plans 1 stash + n steps + 1 output write
        assert g.plan_stats(0)["lstm"] == n_lstm * (n + 2)
        total = int(l.sum())
        rand = np.random.default_rng(seed + 7).random((cfg.gen.harmonic_num + 1, 600 * total), dtype=np.float32)
        pcm = g.decode(toks, h, l, rand)
        c2 = hip.counters()
        assert c2["lstm_steps"] - c1["lstm_steps"] == 2 * total + 2 * n  # the shared LSTM over frames, the text encoder's over tokens
        hip.set_option(0, ttship.FUSE_ALL & ~FUSE_LSTM)
        try:
            h0, l0 = g.durations(toks)
            pcm0 = g.decode(toks, h, l, rand)
            assert hip.counters()["lstm_steps"] == c2["lstm_steps"]
        finally:
            hip.set_option(0, ttship.FUSE_ALL)
        assert np.array_equal(l, l0) and np.array_equal(h, h0)
        assert np.isfinite(pcm).all() and float(np.std(pcm)) > 1e-2
        assert np.array_equal(pcm, pcm0), f"max |fused - unfused| = {np.abs(pcm - pcm0).max():.3e}"
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wtype", [Q8_0, Q5_0])
def test_kokoro_quant_weights_read_back(hip, wtype):
    """The stored bytes of every quantized tensor, and the f32 getter = ggml's dequantize_row_* of them."""
    g = ttship.Kokoro(hip.iface(), ttship.kokoro_config(**TINYQ, weight_type=wtype))
    try:
        raw, vals = g.weights_raw(), g.weights()
    finally:
        g.close()
    n_q = 0
    for name, (ty, ne, b) in raw.items():
        if rule(name) == 1 and ne[1] > 1:
            assert ty == wtype, name
            v = dequant(wtype, b)
            assert np.array_equal(vals[name].reshape(-1), v), name
            assert 0 < float(v.std()) and float(np.abs(v).max()) < 10
            n_q += 1
        else:
            assert ty == F32, name
    # ALBERT q k v o ffn ffn_out, encode, duration_proj, and 16 matrices in each of the six LSTM cells
    assert n_q == 6 + 2 + 16 * 6
