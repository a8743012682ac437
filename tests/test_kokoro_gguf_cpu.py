"""Kokoro GGUF files on the CPU oracle's interface: the synthetic writer, the config reader, the loader and the
quantize tool's Kokoro rule on such a file.  No published Kokoro file is at hand: names and keys follow the
reference loader (kokoro_model::prep_constants / assign_* and the generator's *_from_file builders)."""
import numpy as np
import pytest

import py_oracle
import q5_0_ref
import ttship
from test_gguf_cpu import parse_gguf
from test_kokoro_model_cpu import tokens
from test_kokoro_quant_cpu import TINYQ

F32, F16, Q8_0, Q5_0 = ttship.F32, ttship.F16, ttship.Q8_0, ttship.Q5_0
RUN = dict(max_tokens=TINYQ["max_tokens"], max_total=TINYQ["max_total"])
POST_LOAD = ("hidden", "state", "sqrt_tensor", "stft_window", "harmonic_sampling_norm", "sampling_factor_scalar", "n_kernels_tensor", "one")


def host_rows(ty, x):
    """The quantize tool's host callback: ggml's reference quantizers in numpy / the oracle."""
    return py_oracle.quantize(Q8_0, x) if ty == Q8_0 else q5_0_ref.quantize_row_q5_0(x)


@pytest.fixture(scope="module")
def f32_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("kokoro") / "tinyq-f32.gguf"
    ttship.write_kokoro_synthetic_gguf(path, ttship.kokoro_config(**TINYQ))
    return path


def test_kokoro_synthetic_file_parses_independently(f32_file):
    version, kv, infos, data0, raw = parse_gguf(f32_file)
    assert version == 3 and kv["general.architecture"] == "kokoro"
    c = ttship.kokoro_config(**TINYQ)
    want = {"kokoro.duration_predictor.albert.context_length": c.max_context, "kokoro.tokenizer.vocab_size": c.n_vocab,
            "kokoro.duration_predictor.albert.hidden_size": c.hidden, "kokoro.duration_predictor.albert.attn_heads": c.n_heads,
            "kokoro.duration_predictor.albert.layers": c.n_layers, "kokoro.duration_predictor.albert.recurrence": c.n_recurrence,
            "kokoro.duration_predictor.hidden_size": c.d_model, "kokoro.duration_predictor.f0_n_blocks": 3,
            "kokoro.duration_predictor.layers": c.n_dur_layers, "kokoro.text_encoder.layers": c.te_depth,
            "kokoro.decoder.generator.layers": c.n_decode, "kokoro.decoder.generator.kernels": c.gen.n_kernels,
            "kokoro.decoder.generator.upsamples": c.gen.n_ups, "kokoro.decoder.generator.n_fft": c.gen.n_fft,
            "kokoro.decoder.generator.hop": c.gen.hop, "kokoro.decoder.generator.up_sampling_factor": 300,
            "kokoro.decoder.generator.padding": 3, "kokoro.decoder.generator.up_convs.0.stride": 10,
            "kokoro.decoder.generator.up_convs.1.padding": 3, "kokoro.decoder.generator.noise_blocks.0.stride": 6,
            "kokoro.decoder.generator.noise_blocks.1.res_block.2.dilation": 5, "kokoro.decoder.generator.res_blocks.5.1.padding": 15}
    for key, v in want.items():
        assert kv.get(key) == v, (key, kv.get(key), v)
    names = {name: (ne, ty) for name, ne, ty, off in infos}
    assert all(n.startswith("kokoro.") for n in names) and {ty for _, ty in names.values()} == {F32}
    for n in ("kokoro.albert.token_embd", "kokoro.albert.layer.0.q", "kokoro.albert.layer.0.ffn_norm", "kokoro.albert.layer.0.attn_norm_bias",
              "kokoro.duration_predictor.layers.0.lstm.0.reverse_weights.7", "kokoro.duration_predictor.layers.1.gamma_weight",
              "kokoro.duration_predictor.shared_lstm.0.biases.0", "kokoro.duration_predictor.f0_blocks.1.pool_weight",
              "kokoro.text_encoder.embedding_weight", "kokoro.text_encoder.lstm.0.weights.1", "kokoro.decoder.asr_conv_weight",
              "kokoro.decoder.decoder_blocks.3.conv1x1_weight", "kokoro.decoder.generator.ups.0.weight",
              "kokoro.decoder.generator.noise_blocks.0.conv_weight", "kokoro.decoder.generator.noise_blocks.1.resblock.2.alpha1",
              "kokoro.decoder.generator.resblocks.5.0.convs1_weight", "kokoro.decoder.generator.m_source_weight",
              "kokoro.decoder.generator.conv_post_bias", "kokoro.voice_tensors.synthetic"):
        assert n in names, n
    assert not [n for n in names if n.rsplit(".", 1)[-1] in POST_LOAD or "layer_out_norm" in n or ".gen." in n]
    assert names["kokoro.albert.layer.0.q_bias"][0] == [c.hidden] and names["kokoro.voice_tensors.synthetic"][0] == [2 * c.gen.style_dim, c.n_voice_rows]


def test_kokoro_from_gguf_equals_the_synthetic_runner(f32_file):
    toks = tokens(9, 4)
    s = ttship.Kokoro(py_oracle.iface(8), ttship.kokoro_config(**TINYQ))
    with ttship.Gguf(f32_file) as g:
        cfg = ttship.kokoro_config_from_gguf(g, **RUN)
        want = ttship.kokoro_config(**TINYQ)
        for f in ("n_vocab", "embd", "hidden", "n_heads", "ffn", "n_layers", "n_recurrence", "max_context", "d_model", "n_dur_layers", "max_dur",
                  "te_kernel", "te_depth", "dec_dim", "asr_res_dim", "n_decode", "n_voice_rows", "max_tokens", "max_total", "weight_type"):
            assert getattr(cfg, f) == getattr(want, f), f
        for f in ("in_channels", "style_dim", "n_ups", "n_kernels", "n_fft", "hop", "harmonic_num"):
            assert getattr(cfg.gen, f) == getattr(want.gen, f), f
        for f in ("up_rates", "up_kernels", "res_kernels", "res_dilations", "noise_res_kernels"):
            assert list(getattr(cfg.gen, f)) == list(getattr(want.gen, f)), f
        k = ttship.Kokoro.from_gguf(py_oracle.iface(8), g, **RUN)
        with pytest.raises(RuntimeError):
            ttship.Kokoro.from_gguf(py_oracle.iface(2), g, voice="nobody", **RUN)
        k2 = ttship.Kokoro.from_gguf(py_oracle.iface(2), g, voice="synthetic", **RUN)
        k2.close()
    try:
        a, b = s.weights_raw(), k.weights_raw()
        assert list(a) == list(b)
        for name in a:
            assert a[name][:2] == b[name][:2] and np.array_equal(a[name][2], b[name][2]), name
        hs, ls = s.durations(toks)
        hk, lk = k.durations(toks)
        assert np.array_equal(hs, hk) and np.array_equal(ls, lk)
        rand = np.random.default_rng(1).random((s.cfg.gen.harmonic_num + 1, 600 * int(ls.sum())), dtype=np.float32)
        assert np.array_equal(s.decode(toks, hs, ls, rand), k.decode(toks, hs, ls, rand))
    finally:
        s.close()
        k.close()


@pytest.mark.parametrize("qt", [F16, Q8_0, Q5_0])
def test_kokoro_quantized_file_types_follow_the_rule(f32_file, tmp_path, qt):
    dst = tmp_path / "q.gguf"
    p = ttship.quantize_params(qt, convert_non_quantizable_to_f16=1 if qt == F16 else 0)
    ttship.quantize_gguf(f32_file, dst, p, rows_fn=host_rows)
    n = {F32: 0, F16: 0, Q8_0: 0, Q5_0: 0}
    with ttship.Gguf(f32_file) as src, ttship.Gguf(dst) as g:
        assert g.get("general.architecture") == "kokoro"
        for name, ty, ne, _, _ in g.tensors():
            r = ttship.gguf_tensor_rule("kokoro", name, p)
            assert ty == (F32 if r == 0 else F16 if r == 2 or qt == F16 else qt), (name, ty, r)
            n[ty] += 1
            if r == 1 and qt != F16:
                x = src.tensor_bytes(name).view(np.float32).reshape(-1, ne[0])
                assert np.array_equal(g.tensor_bytes(name), host_rows(qt, x)), name
        if qt == F16:
            assert n[F16] > 104 and n[Q8_0] == n[Q5_0] == 0
        else:
            assert n[qt] == 6 + 2 + 16 * 6 and n[F16] == 0
        if qt == Q5_0:
            return  # the oracle holds no Q5_0: tests/test_kokoro_quant_gpu.py runs this file's Q8_0 twin
        # the file loads with the file's types and runs on the oracle
        k = ttship.Kokoro.from_gguf(py_oracle.iface(8), g, **RUN)
        try:
            raw = k.weights_raw()
            for name, ty, ne, _, _ in g.tensors():
                rn = name[len("kokoro."):]
                if rn in raw and "_norm" not in rn:  # the front half keeps the file's names but for ALBERT's two norms
                    assert raw[rn][0] == ty and np.array_equal(raw[rn][2], g.tensor_bytes(name)), name
            # the file's "ffn_norm" is the norm after attention, its "attn_norm" the norm after the FFN
            for ours, theirs in (("attn_norm", "ffn_norm"), ("layer_out_norm", "attn_norm"), ("attn_norm_bias", "ffn_norm_bias")):
                assert np.array_equal(raw["albert.layer.0." + ours][2], g.tensor_bytes("kokoro.albert.layer.0." + theirs))
            assert sum(1 for ty, _, _ in raw.values() if ty == qt) == n[qt]
            toks = tokens(9, 4)
            h, l = k.durations(toks)
            pcm = k.decode(toks, h, l, np.random.default_rng(1).random((k.cfg.gen.harmonic_num + 1, 600 * int(l.sum())), dtype=np.float32))
            assert np.isfinite(h).all() and np.isfinite(pcm).all() and float(np.std(pcm)) > 1e-3
        finally:
            k.close()


def test_kokoro_file_with_a_quantized_bias_is_refused(f32_file, tmp_path, capfd):
    bad, keep = tmp_path / "bad.gguf", []
    w = ttship.GgufWriter()
    with ttship.Gguf(f32_file) as g:
        w.copy_kv(g)
        for name, ty, ne, _, _ in g.tensors():
            data = g.tensor_bytes(name)
            if name == "kokoro.albert.layer.0.q_bias":
                ty, data = Q8_0, py_oracle.quantize(Q8_0, data.view(np.float32).reshape(1, -1))
            keep.append(np.ascontiguousarray(data))
            w.add_tensor(name, ty, ne, keep[-1])
        w.write(bad)
    w.close()
    with ttship.Gguf(bad) as g:
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            ttship.Kokoro.from_gguf(py_oracle.iface(2), g, **RUN)
        assert "kokoro.albert.layer.0.q_bias" in capfd.readouterr().err
