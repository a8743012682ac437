"""Q5_0 on the host: type traits, the twin identity that makes the unchanged CPU oracle a bit-exact Q5_0
reference (tests/q5_0_ref.py), the quantize tool writing Q5_0 files, and the synthetic Q5_0 fill."""
import numpy as np
import pytest

import py_oracle
import q5_0_ref as q5
import ttship
from test_gguf_cpu import DAC_TINY, TINY


def test_type_traits():
    L = ttship.lib()
    assert (L.tts_type_size(ttship.Q5_0), L.tts_blck_size(ttship.Q5_0)) == (22, 32)
    assert L.tts_row_size(ttship.Q5_0, 2048) == 1408 and L.tts_type_name(ttship.Q5_0) == b"q5_0"
    assert (ttship.TYPE_SIZE[ttship.Q5_0], ttship.BLCK_SIZE[ttship.Q5_0]) == (22, 32)
    assert ttship.row_size(ttship.Q5_0, 2048) == 1408


def test_unpack_covers_the_range_and_layout():
    # one block by hand: weight j = (qs[j] & 15 | bit j of qh << 4) - 16, weight j + 16 from the high nibble and bit j + 16
    b = np.zeros(22, np.uint8)
    b[0:2] = np.array([1.0], np.float16).view(np.uint8)
    b[2:6] = np.array([0x00018001], np.uint32).view(np.uint8)  # bits 0, 15, 16
    b[6] = 0xF3   # weight 0: 3 | 16 -> 3;  weight 16: 15 | 16 -> 15
    b[21] = 0x0A  # weight 15: 10 | 16 -> 10; weight 31: 0 -> -16
    d, w = q5.unpack(b)
    assert d[0] == 1.0 and (w[0, 0], w[0, 16], w[0, 15], w[0, 31], w[0, 1]) == (3, 15, 10, -16, -16)
    d, w = q5.unpack(q5.rand_q5_0(np.random.default_rng(0), 8, 256))
    assert w.min() == -16 and w.max() == 15


@pytest.mark.parametrize("K", [96, 256, 1024])
def test_twin_identity(K):
    """ggml's Q5_0 x Q8_0 loop == the oracle's Q8_0 x Q8_0 GEMV on the twin, bit for bit."""
    rng = np.random.default_rng(K)
    N, M = 7, 3
    w = q5.rand_q5_0(rng, N, K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    ref = py_oracle.gemv(ttship.Q8_0, q5.twin_q8_0(w), x, N)
    got = q5.vec_dot_q5_0_q8_0(w, x, N)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # and the twin dequantizes to the Q5_0 weights d * (q - 16)
    d, q = q5.unpack(w)
    deq = (q.astype(np.float32) * d.astype(np.float32)[:, None]).reshape(N, K)
    assert np.array_equal(py_oracle.dequant_q8_0(q5.twin_q8_0(w), K, N), deq)


def test_numpy_quantizer_known_answers():
    x = np.zeros((1, 96), np.float32)
    x[0, :32] = np.arange(-16, 16)          # max = -16 -> d = 1: q - 16 = x exactly
    x[0, 32:64] = -np.arange(-16, 16) * 0.5  # max = +8 -> d = -0.5: q - 16 = x / d
    d, w = q5.unpack(q5.quantize_row_q5_0(x))
    assert list(d) == [1.0, -0.5, 0.0]
    assert np.array_equal(w[0], np.arange(-16, 16)) and np.array_equal(w[1], np.arange(-16, 16))
    assert np.all(w[2] == 0)  # zeros: id = 0, q = (int8_t)16.5 = 16
    # a positive maximum saturates at q = 0 (-16 * d), its mirror value clips at 31
    y = np.zeros((1, 32), np.float32)
    y[0, 3], y[0, 9] = 4.0, -4.0
    d, w = q5.unpack(q5.quantize_row_q5_0(y))
    assert d[0] == -0.25 and w[0, 3] == -16 and w[0, 9] == 15


def _numpy_rows(ttype, x):
    assert ttype == ttship.Q5_0
    return q5.quantize_row_q5_0(x)


def test_quantize_tool_writes_q5_0(tmp_path):
    cfg32 = ttship.parler_config(weight_type=ttship.F32, head_type=ttship.F32, **TINY)
    src, dst = tmp_path / "parler-f32.gguf", tmp_path / "parler-q5_0.gguf"
    ttship.write_parler_synthetic_gguf(src, cfg32, ttship.dac_config(**DAC_TINY))
    ttship.quantize_gguf(src, dst, ttship.quantize_params(ttship.Q5_0), rows_fn=_numpy_rows)
    n_q = 0
    with ttship.Gguf(src) as a, ttship.Gguf(dst) as b:  # the file reloads
        assert b.get("general.quantization_type") == ttship.Q5_0
        ta, tb = a.tensors(), b.tensors()
        assert [t[0] for t in ta] == [t[0] for t in tb]
        for (name, ty, ne, _, _), (_, ty2, ne2, _, nbytes) in zip(ta, tb):
            assert ne == ne2
            if ttship.gguf_tensor_rule("parler-tts", name) == 1:
                n_q += 1
                assert ty2 == ttship.Q5_0 and nbytes == int(np.prod(ne)) // 32 * 22, name
                x = a.tensor_bytes(name).view(np.float32).reshape(-1, ne[0])
                assert np.array_equal(b.tensor_bytes(name), q5.quantize_row_q5_0(x)), name
            else:
                assert ty2 == ty and np.array_equal(b.tensor_bytes(name), a.tensor_bytes(name)), name
        cfg = ttship.parler_config_from_gguf(b, max_ctx=TINY["max_ctx"])
        assert cfg.weight_type == ttship.Q5_0 and cfg.head_type == ttship.F32
    assert n_q == 9 + 8 * TINY["n_layers"]


def test_synthetic_q5_0_file(tmp_path):
    cfg = ttship.parler_config(weight_type=ttship.Q5_0, head_type=ttship.F32, **TINY)
    path = tmp_path / "parler-q5_0-synth.gguf"
    ttship.write_parler_synthetic_gguf(path, cfg)
    with ttship.Gguf(path) as g:
        ts = {t[0]: t for t in g.tensors()}
        for name, std in (("decoder.layers.1.fc1.weight", 0.02), ("decoder.embed_tokens.3.weight", 0.25)):
            _, ty, ne, _, nbytes = ts[name]
            assert ty == ttship.Q5_0 and nbytes == ne[0] * ne[1] // 32 * 22
            w = py_oracle.dequant_q8_0(q5.twin_q8_0(g.tensor_bytes(name)), ne[0], ne[1])
            assert abs(w.std() / std - 1) < 0.2 and abs(w.mean()) < 0.1 * std, (name, w.std(), w.mean())
        assert ts["decoder.lm_heads.0.weight.head"][1] == ttship.F32 and ts["decoder.embed_prompts"][1] == ttship.F32
