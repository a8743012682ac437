"""Kokoro with Q8_0 / Q5_0 weights (tts_kokoro_config.weight_type, f16_rest) on the CPU oracle's interface:
which tensors take which storage type, what the two weight getters return, and which configurations are
refused.  The rule is the quantize tool's (tts_gguf_tensor_rule("kokoro", ...), examples/quantize/
quantize_impl.cpp:14-40), so a synthetic runner holds the types a quantized Kokoro file holds."""
import ctypes

import numpy as np
import pytest

import py_oracle
import q5_0_ref
import ttship
from test_kokoro_model_cpu import TINY, tokens

F32, F16, Q8_0, Q5_0 = ttship.F32, ttship.F16, ttship.Q8_0, ttship.Q5_0
# every quantizable row is 32, 64, 96 or 128 long
TINYQ = dict(TINY, d_model=64, gen=dict(TINY["gen"], style_dim=32))


def rule(name, nqf=0):
    p = ttship.QuantizeParams()
    p.quantize_type = Q8_0
    p.convert_non_quantizable_to_f16 = nqf
    return ttship.lib().tts_gguf_tensor_rule(b"kokoro", ("kokoro." + name).encode(), ctypes.byref(p))


def dequant(ty, raw):
    if ty == Q8_0:
        return py_oracle.dequant_q8_0(raw, 32, raw.size // 34).reshape(-1)
    d, q = q5_0_ref.unpack(raw)
    return (q.astype(np.float32) * d.astype(np.float32)[:, None]).reshape(-1)


@pytest.mark.parametrize("wtype", [Q8_0, Q5_0])
@pytest.mark.parametrize("f16_rest", [0, 1])
def test_kokoro_quant_tensor_types_follow_the_rule(wtype, f16_rest):
    k = ttship.Kokoro(py_oracle.iface(4), ttship.kokoro_config(**TINYQ, weight_type=wtype, f16_rest=f16_rest))
    try:
        raw = k.weights_raw()
        vals = k.weights()
    finally:
        k.close()
    assert set(raw) == set(vals)
    n_q = n_f16 = 0
    for name, (ty, ne, b) in raw.items():
        matrix = sum(1 for d in ne if d != 1) >= 2 or ne[1] > 1
        quant = rule(name) == 1 and matrix
        if quant:
            assert ty == wtype and ne[0] % 32 == 0, (name, ty, ne)
            assert b.size == int(np.prod(ne)) // 32 * ttship.TYPE_SIZE[wtype]
            if wtype == Q8_0:  # the oracle's interface stores no Q5_0 bytes: tests/test_kokoro_quant_gpu.py reads those back
                assert np.array_equal(vals[name].reshape(-1), dequant(wtype, b)), name
                assert 0 < float(np.abs(vals[name]).max()) < 10
            n_q += 1
        else:
            assert ty in ((F32, F16) if f16_rest else (F32,)), (name, ty)
            assert not (name.endswith(("bias", "embd", "norm")) or "gamma" in name or "beta" in name or "voice_tensors" in name) or ty == F32
            n_f16 += ty == F16
    # ALBERT q k v o ffn ffn_out, encode, duration_proj, and 16 matrices in each of the six LSTM cells
    # (n_dur_layers DurationEncoder cells, duration_lstm, shared_lstm, text_encoder.lstm)
    assert n_q == 6 + 2 + 16 * (TINYQ.get("n_dur_layers", 3) + 3)
    assert (n_f16 > 0) == bool(f16_rest)
    for name in ("albert.embd", "albert.token_embd", "duration_predictor.layers.1.gamma_weight", "decoder.asr_conv_weight",
                 "text_encoder.lstm.0.biases.1", "duration_predictor.shared_lstm.0.hidden", "gen.ups.0.weight"):
        assert raw[name][0] not in (Q8_0, Q5_0), name
    for name in ("albert.layer.0.q", "text_encoder.lstm.0.weights.1", "duration_predictor.layers.0.lstm.0.reverse_weights.6",
                 "duration_predictor.duration_proj", "duration_predictor.encode"):
        assert raw[name][0] == wtype, name


def test_kokoro_quant_leaves_f32_and_f16_runners_as_they_were():
    """weight_type F16 means what it meant, and f16_rest alone is the same file (`-qt F16 -nqf`)."""
    def types(**kw):
        k = ttship.Kokoro(py_oracle.iface(4), ttship.kokoro_config(**TINYQ, **kw))
        try:
            return {n: (ty, bytes(b)) for n, (ty, ne, b) in k.weights_raw().items()}
        finally:
            k.close()
    f32, f16 = types(weight_type=F32), types(weight_type=F16)
    assert {ty for ty, _ in f32.values()} == {F32}
    assert {ty for ty, _ in f16.values()} == {F32, F16}
    assert types(weight_type=F32, f16_rest=1) == f16


@pytest.mark.parametrize("wtype", [Q8_0, Q5_0])
def test_kokoro_quant_refuses_rows_that_are_no_whole_blocks(wtype, capfd):
    """TINY: d_model 32 + style 16 = 48-long LSTM input rows."""
    with pytest.raises(RuntimeError):
        ttship.Kokoro(py_oracle.iface(2), ttship.kokoro_config(**TINY, weight_type=wtype))
    err = capfd.readouterr().err
    assert "duration_predictor.layers.0.lstm.0.weights.0 (rows of 48)" in err, err
    with pytest.raises(RuntimeError):
        ttship.Kokoro(py_oracle.iface(2), ttship.kokoro_config(**TINYQ, weight_type=ttship.Q4_K))


def test_kokoro_generator_ignores_a_quantized_type():
    cfg = dict(in_channels=32, style_dim=32, max_frames=16)
    for f16_rest in (0, 1):
        g = ttship.KokoroGenerator(py_oracle.iface(2), ttship.kokoro_gen_config(**cfg, weight_type=Q8_0, f16_rest=f16_rest))
        try:
            tys = {ty for ty, _, _ in g.weights_raw().values()}
        finally:
            g.close()
        assert tys == ({F32, F16} if f16_rest else {F32})


def test_kokoro_q8_0_runs_on_the_oracle():
    """What can be pinned on the CPU alone: both graphs run on the Q8_0 weights, repeat themselves, and the
    hidden states move with the tokens.  tests/test_kokoro_quant_gpu.py compares the HIP backend with this run."""
    k = ttship.Kokoro(py_oracle.iface(8), ttship.kokoro_config(**TINYQ, weight_type=Q8_0))
    try:
        assert k.weights_raw()["text_encoder.lstm.0.weights.1"][0] == Q8_0  # not the F32 an unknown type once silently meant
        toks = tokens(9, 4)
        h, l = k.durations(toks)
        h2, l2 = k.durations(toks)
        assert np.array_equal(h, h2) and np.array_equal(l, l2)
        assert np.isfinite(h).all() and l.min() >= 1 and l.max() <= k.cfg.max_dur
        assert float(np.std(h[:, :k.cfg.d_model], axis=0).min()) > 0
        pcm = k.decode(toks, h, l, np.random.default_rng(1).random((k.cfg.gen.harmonic_num + 1, 600 * int(l.sum())), dtype=np.float32))
        assert np.isfinite(pcm).all() and float(np.std(pcm)) > 1e-3
    finally:
        k.close()
