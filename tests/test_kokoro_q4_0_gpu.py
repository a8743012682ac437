"""Kokoro with Q4_0 weights on the HIP backend: from a GGUF file the quantize tool wrote, and synthetic.

The TINYQ F32 file is quantized to Q4_0 on the device (bytes equal the host quantizer's), every d is trimmed to
nine bits and the trimmed file's Q8_0 twin is written (tests/q4_0_ref.py, R2).  HIP runs the trimmed Q4_0 file,
the CPU oracle its twin, under the rule tests/test_kokoro_quant_gpu.py uses for Q5_0 (compare_with_oracle):
rounded lengths identical, hidden states within 1e-3 * max(1, max|ref|), PCM from the oracle's durations within
1e-4 absolute, run() = durations() + decode(); with every fusion on and at fusion mask 0.  Inputs, as there: those
on which the oracle's scalar and SIMD modes give identical lengths and hidden states within 1e-6 of each other on
this twin, checked on the CPU first (profiles/r11/oracle_scalar_vs_simd_kokoro_q4_0_twin.txt): n = 7 seed 1 and
n = 13 seed 1 qualify (n = 7 seed 0 does not: 0.095 apart).  The general-d file and the synthetic runner are
HIP against HIP: the fused LSTM step changes no bit."""
import numpy as np
import pytest

import py_oracle
import q4_0_ref as q4
import ttship
from test_kokoro_gguf_cpu import RUN
from test_kokoro_model_cpu import tokens
from test_kokoro_quant_cpu import TINYQ, rule
from test_kokoro_quant_gpu import FUSE_LSTM, compare_with_oracle

pytestmark = pytest.mark.gpu
F32, Q8_0, Q4_0 = ttship.F32, ttship.Q8_0, ttship.Q4_0
N_QUANT = 6 + 2 + 16 * 6  # ALBERT q k v o ffn ffn_out, encode, duration_proj, and 16 matrices in each of the six LSTM cells


def host_rows(ty, x):
    assert ty == Q4_0
    return q4.quantize_row_q4_0(x)


@pytest.fixture(scope="module")
def files(hip, tmp_path_factory):
    d = tmp_path_factory.mktemp("kokoro_q4_0")
    out = {k: d / f"{k}.gguf" for k in ("f32", "q4_0", "q4_0_host", "trim", "twin")}
    ttship.write_kokoro_synthetic_gguf(out["f32"], ttship.kokoro_config(**TINYQ))
    ttship.quantize_gguf(out["f32"], out["q4_0"], ttship.quantize_params(Q4_0), backend=hip)
    ttship.quantize_gguf(out["f32"], out["q4_0_host"], ttship.quantize_params(Q4_0), rows_fn=host_rows)
    q4.trim_gguf(out["q4_0"], out["trim"])
    q4.twin_gguf(out["trim"], out["twin"])
    return out


def test_kokoro_q4_0_file_device_quantizer_equals_host(files):
    with ttship.Gguf(files["q4_0"]) as a, ttship.Gguf(files["q4_0_host"]) as b, ttship.Gguf(files["twin"]) as t:
        ta, tb = a.tensors(), b.tensors()
        assert [x[:3] for x in ta] == [x[:3] for x in tb]
        assert sum(1 for x in ta if x[1] == Q4_0) == N_QUANT and {x[1] for x in ta} == {F32, Q4_0}
        for x in ta:
            assert np.array_equal(a.tensor_bytes(x[0]), b.tensor_bytes(x[0])), x[0]
        assert {x[1] for x in t.tensors()} == {F32, Q8_0}


@pytest.mark.parametrize("n,seed,mask", [(7, 1, None), (13, 1, None), (7, 1, 0), (13, 1, 0)])
def test_kokoro_q4_0_file_matches_oracle_on_the_twin(hip, files, n, seed, mask):
    def make(iface, on_gpu):
        with ttship.Gguf(files["trim" if on_gpu else "twin"]) as g:
            return ttship.Kokoro.from_gguf(iface, g, **RUN)
    cfg, steps = compare_with_oracle(hip, "file-q4_0", n, seed, mask=mask, make=make)
    assert cfg.weight_type == Q4_0
    assert steps == (2 * n * (cfg.n_dur_layers + 1) if mask is None else 0)


def fused_lstm_changes_no_bit(hip, g, n, seed):
    cfg, toks = g.cfg, tokens(n, seed)
    c0 = hip.counters()
    h, l = g.durations(toks)
    c1 = hip.counters()
    n_lstm = cfg.n_dur_layers + 1
    assert c1["lstm_steps"] - c0["lstm_steps"] == 2 * n * n_lstm and c1["lstm_chains"] - c0["lstm_chains"] == 2 * n_lstm
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


def test_kokoro_q4_0_general_d_file_fused_lstm_changes_no_bit(hip, files):
    """HIP against HIP: the untrimmed device-quantized file loads, and the LSTM fusion changes no bit of it."""
    with ttship.Gguf(files["q4_0"]) as f:
        g = ttship.Kokoro.from_gguf(hip.iface(), f, **RUN)
    try:
        assert g.cfg.weight_type == Q4_0
        fused_lstm_changes_no_bit(hip, g, 7, 1)
    finally:
        g.close()


def test_kokoro_q4_0_synthetic_fused_lstm_and_weights_read_back(hip):
    g = ttship.Kokoro(hip.iface(), ttship.kokoro_config(**TINYQ, weight_type=Q4_0))
    try:
        fused_lstm_changes_no_bit(hip, g, 7, 0)
        raw, vals = g.weights_raw(), g.weights()
    finally:
        g.close()
    n_q = 0
    for name, (ty, ne, b) in raw.items():
        if rule(name) == 1 and ne[1] > 1:
            assert ty == Q4_0 and b.size == int(np.prod(ne)) // 32 * 18, name
            v = q4.dequantize(b, 32, b.size // 18).reshape(-1)  # the f32 getter = dequantize_row_q4_0 of the stored bytes
            assert np.array_equal(vals[name].reshape(-1), v), name
            assert 0 < float(v.std()) and float(np.abs(v).max()) < 10
            n_q += 1
        else:
            assert ty == F32, name
    assert n_q == N_QUANT


def test_kokoro_file_with_a_q4_0_bias_is_refused(hip, files, tmp_path, capfd):
    bad, keep = tmp_path / "bad.gguf", []
    w = ttship.GgufWriter()
    with ttship.Gguf(files["f32"]) as g:
        w.copy_kv(g)
        for name, ty, ne, _, _ in g.tensors():
            data = g.tensor_bytes(name)
            if name == "kokoro.albert.layer.0.q_bias":
                ty, data = Q4_0, q4.quantize_row_q4_0(data.view(np.float32).reshape(1, -1))
            keep.append(np.ascontiguousarray(data))
            w.add_tensor(name, ty, ne, keep[-1])
        w.write(bad)
    w.close()
    with ttship.Gguf(bad) as g:
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            ttship.Kokoro.from_gguf(hip.iface(), g, **RUN)
        assert "kokoro.albert.layer.0.q_bias" in capfd.readouterr().err
