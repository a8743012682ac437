"""Q4_0 on the host: type traits, the numpy quantizer against hand-written bytes, the two references of
tests/q4_0_ref.py (R2 is sound: trimmed blocks equal their Q8_0 twins under the unchanged oracle; R1
discriminates: on the GPU module's own inputs ggml's Q4_0 order and the twin's order differ), the quantize tool
writing Q4_0 files, and a Kokoro file quantized to Q4_0."""
import numpy as np
import pytest

import lstm_q4_0 as l4
import py_oracle
import q4_0_ref as q4
import q5_0_ref as q5
import ttship
from test_gguf_cpu import DAC_TINY, TINY
from test_kokoro_gguf_cpu import RUN
from test_kokoro_model_cpu import tokens
from test_kokoro_quant_cpu import TINYQ

F32, F16, Q4, Q5, Q8 = ttship.F32, ttship.F16, ttship.Q4_0, ttship.Q5_0, ttship.Q8_0


def test_type_traits():
    L = ttship.lib()
    assert (L.tts_type_size(Q4), L.tts_blck_size(Q4)) == (18, 32)
    assert L.tts_row_size(Q4, 2048) == 1152 and L.tts_type_name(Q4) == b"q4_0"
    assert (ttship.TYPE_SIZE[Q4], ttship.BLCK_SIZE[Q4]) == (18, 32) and ttship.row_size(Q4, 256) == 144
    assert [ttship.OPT[k] for k in ("GEMV_Q40_SLAB", "GEMV_Q40_RW", "GEMM_Q4_0", "GEMM_Q4_0_STAGED")] == [49, 50, 51, 52]


def test_known_answer_block():
    x = np.concatenate([np.arange(-8, 8), np.arange(-8, 8)]).astype(np.float32)[None]
    want = bytes([0x00, 0x3C] + [j | (j << 4) for j in range(16)])  # d = 1.0, qs[j] = j | j << 4
    got = q4.quantize_row_q4_0(x)
    assert got.tobytes() == want
    assert np.array_equal(q4.dequantize(got, 32, 1), x)


def test_quantizer_cases_against_hand_written_bytes():
    # all zeros: max = 0, d = 0 / -8 = -0.0 (f16 0x8000), id = 0, q = (int8_t)8.5 = 8 everywhere
    assert q4.quantize_row_q4_0(np.zeros((1, 32), np.float32)).tobytes() == bytes([0x00, 0x80] + [0x88] * 16)
    # a positive maximum: d = 4 / -8 = -0.5 (f16 0xB800); x = 4 -> 4 * -2 + 8.5 = 0.5 -> 0; its mirror -4 -> 16.5 -> MIN(15);
    # x = 1 (element 17) -> 6.5 -> 6; the zeros -> 8
    y = np.zeros((1, 32), np.float32)
    y[0, 3], y[0, 9], y[0, 17] = 4.0, -4.0, 1.0
    want = [0x88] * 16
    want[3], want[9], want[1] = 0x80, 0x8F, 0x68
    assert q4.quantize_row_q4_0(y).tobytes() == bytes([0x00, 0xB8] + want)
    # a tie in magnitude: the first wins.  -2 first: d = 0.25 (0x3400): -2 -> 0.5 -> 0, +2 -> 16.5 -> 15
    t = np.zeros((1, 32), np.float32)
    t[0, 0], t[0, 16] = -2.0, 2.0
    assert q4.quantize_row_q4_0(t).tobytes() == bytes([0x00, 0x34, 0xF0] + [0x88] * 15)
    # +2 first: d = -0.25 (0xB400): +2 -> 0.5 -> 0, -2 -> 16.5 -> 15 -- the same quants under the other sign of d
    assert q4.quantize_row_q4_0(-t).tobytes() == bytes([0x00, 0xB4, 0xF0] + [0x88] * 15)


def test_unpack_layout_and_trim():
    b = np.zeros(18, np.uint8)
    b[0:2] = np.array([1.0], np.float16).view(np.uint8)
    b[2], b[17] = 0xF3, 0x0A  # weight 0: 3 - 8, weight 16: 15 - 8; weight 15: 10 - 8, weight 31: 0 - 8
    d, w = q4.unpack(b)
    assert d[0] == 1.0 and (w[0, 0], w[0, 16], w[0, 15], w[0, 31], w[0, 1]) == (-5, 7, 2, -8, -8)
    r = q4.rand_q4_0(np.random.default_rng(0), 8, 256)
    d, w = q4.unpack(r)
    assert w.min() == -8 and w.max() == 7 and (d.view(np.uint16) & 3).any()
    dt, wt = q4.unpack(q4.trim_d(r))
    assert np.array_equal(wt, w) and not (dt.view(np.uint16) & 3).any() and np.array_equal(dt.view(np.uint16), d.view(np.uint16) & 0xFFFC)


@pytest.mark.parametrize("K,N,M", [(96, 5, 1), (256, 33, 2), (1024, 64, 8)])
def test_r2_is_sound(K, N, M):
    """On trimmed blocks ggml's Q4_0 x Q8_0 loop == the oracle's Q8_0 x Q8_0 GEMV on the twin, bit for bit."""
    rng = np.random.default_rng(K + N)
    w = q4.trim_d(q4.rand_q4_0(rng, N, K))
    x = rng.standard_normal((M, K)).astype(np.float32)
    ref = py_oracle.gemv(Q8, q4.twin_q8_0(w), x, N)
    got = q4.vec_dot_q4_0_q8_0(w, x, N)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(py_oracle.dequant_q8_0(q4.twin_q8_0(w), K, N).view(np.uint32), q4.dequantize(w, K, N).view(np.uint32))


# Exempt (N * M < 32; a handful of sums may well agree): GEMV (96, 5) at M = 1, 2, 5, (256, 1) and (256, 3) at every M.
KERNEL_CASES = [("gemv", K, N, M) for K, N in q4.GEMV_SHAPES for M in q4.GEMV_COLS if N * M >= 32] + \
               [("gemm", K, N, M) for K, N in q4.GEMM_SHAPES for M in q4.GEMM_COLS if N * M >= 32] + \
               [("residual", K, N, M) for K, N, M in q4.RESIDUAL_SHAPES]
CASE_FN = {"gemv": q4.gemv_case, "gemm": q4.gemm_case, "residual": q4.residual_case}


@pytest.mark.parametrize("kind,K,N,M", KERNEL_CASES)
def test_r1_discriminates(kind, K, N, M):
    """A condition on the GPU module's inputs: on its untrimmed weights ggml's Q4_0 order and the twin's (Q8_0)
    order give different bits somewhere, so a kernel that folded in the twin's order would fail there."""
    w, x = CASE_FN[kind](K, N, M)
    r1 = q4.vec_dot_q4_0_q8_0(w, x, N)
    tw = py_oracle.gemv(Q8, q4.twin_q8_0(w), x, N)
    assert np.any(r1.view(np.uint32) != tw.view(np.uint32))
    assert np.allclose(r1, tw, rtol=1e-4, atol=1e-5)  # and still the same product


@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("hd", l4.PART_HD)
def test_r1_discriminates_on_the_lstm_step(hd, bi):
    """The same condition on the inputs of tests/test_lstm_q4_0_gpu.py's order-sensitive case: per direction, the
    first step's recurrent product W_hh h0 differs between ggml's Q4_0 order and the twin's, and so do the gates'
    inputs after the f32 adds of the node chain -- in at least four rows, one of them of the tanh gate, which hands a
    last-bit difference on to the state.  A fused step folding in the twin's order would therefore leave the
    unfused chain at its first step."""
    x, dirs, h0, c0 = l4.parting_inputs(3, 64, hd, bi)
    assert len(dirs) == (2 if bi else 1) and h0.shape == c0.shape == (hd,)
    for k, d in enumerate(dirs):
        assert d["w_hh_q"].size == 4 * hd * hd // 32 * 18 and d["w_hh"].shape == (4 * hd, hd)
        a, mm_a = l4.first_step_gate_inputs(x, d, h0, k == 1, "q4_0")
        b, mm_b = l4.first_step_gate_inputs(x, d, h0, k == 1, "twin")
        assert np.any(mm_a.view(np.uint32) != mm_b.view(np.uint32))
        diff = a.view(np.uint32) != b.view(np.uint32)
        assert diff.sum() >= 4 and diff[2 * hd:3 * hd].any(), (k, int(diff.sum()))
        assert np.allclose(a, b, rtol=0, atol=1e-5) and np.abs(a).max() < 4.0  # the same gates, none saturated


def _numpy_rows(ttype, x):
    return {Q4: q4.quantize_row_q4_0, Q5: q5.quantize_row_q5_0}[ttype](x)


def test_quantize_tool_writes_q4_0(tmp_path):
    cfg32 = ttship.parler_config(weight_type=F32, head_type=F32, **TINY)
    src, dst, dst5 = tmp_path / "parler-f32.gguf", tmp_path / "parler-q4_0.gguf", tmp_path / "parler-q5_0.gguf"
    ttship.write_parler_synthetic_gguf(src, cfg32, ttship.dac_config(**DAC_TINY))
    ttship.quantize_gguf(src, dst, ttship.quantize_params(Q4), rows_fn=_numpy_rows)
    ttship.quantize_gguf(src, dst5, ttship.quantize_params(Q5), rows_fn=_numpy_rows)
    n_q = 0
    with ttship.Gguf(src) as a, ttship.Gguf(dst) as b, ttship.Gguf(dst5) as b5:
        assert b.get("general.quantization_type") == 2 == Q4
        ta, tb, t5 = a.tensors(), b.tensors(), b5.tensors()
        assert [t[0] for t in ta] == [t[0] for t in tb] == [t[0] for t in t5]
        for (name, ty, ne, _, _), (_, ty2, ne2, _, nbytes), (_, ty5, _, _, _) in zip(ta, tb, t5):
            assert ne == ne2 and (ty2 == Q4) == (ty5 == Q5), name  # Q4_0 lands where Q5_0 lands
            assert ttship.gguf_tensor_rule("parler-tts", name, ttship.quantize_params(Q4)) == (1 if ty2 == Q4 else 0), name
            if ty2 == Q4:
                n_q += 1
                assert nbytes == int(np.prod(ne)) // 32 * 18, name
                x = a.tensor_bytes(name).view(np.float32).reshape(-1, ne[0])
                assert np.array_equal(b.tensor_bytes(name), q4.quantize_row_q4_0(x)), name
            else:
                assert ty2 == ty and np.array_equal(b.tensor_bytes(name), a.tensor_bytes(name)), name
        cfg = ttship.parler_config_from_gguf(b, max_ctx=TINY["max_ctx"])
        assert cfg.weight_type == Q4 and cfg.head_type == F32
    assert n_q == 9 + 8 * TINY["n_layers"]


def test_synthetic_q4_0_file(tmp_path):
    cfg = ttship.parler_config(weight_type=Q4, head_type=F32, **TINY)
    path = tmp_path / "parler-q4_0-synth.gguf"
    ttship.write_parler_synthetic_gguf(path, cfg)
    with ttship.Gguf(path) as g:
        ts = {t[0]: t for t in g.tensors()}
        for name, std in (("decoder.layers.1.fc1.weight", 0.02), ("decoder.embed_tokens.3.weight", 0.25)):
            _, ty, ne, _, nbytes = ts[name]
            assert ty == Q4 and nbytes == ne[0] * ne[1] // 32 * 18
            w = q4.dequantize(g.tensor_bytes(name), ne[0], ne[1])
            assert abs(w.std() / std - 1) < 0.2 and abs(w.mean()) < 0.2 * std, (name, w.std(), w.mean())
        assert ts["decoder.lm_heads.0.weight.head"][1] == F32 and ts["decoder.embed_prompts"][1] == F32


def test_kokoro_q4_0_file_follows_the_rule_and_loads_as_its_twin(tmp_path):
    """A synthetic Kokoro file quantized to Q4_0 through the tool's rule: types tensor by tensor, and -- the oracle
    holding no Q4_0 -- the loader's names and shapes checked on the file's Q8_0 twin."""
    src, dst, twin = tmp_path / "k-f32.gguf", tmp_path / "k-q4_0.gguf", tmp_path / "k-q4_0-twin.gguf"
    ttship.write_kokoro_synthetic_gguf(src, ttship.kokoro_config(**TINYQ))
    p = ttship.quantize_params(Q4)
    ttship.quantize_gguf(src, dst, p, rows_fn=_numpy_rows)
    n = 0
    with ttship.Gguf(src) as s, ttship.Gguf(dst) as g:
        assert g.get("general.architecture") == "kokoro" and g.get("general.quantization_type") == Q4
        for name, ty, ne, _, _ in g.tensors():
            r = ttship.gguf_tensor_rule("kokoro", name, p)
            assert ty == (F32 if r == 0 else F16 if r == 2 else Q4), (name, ty, r)
            if ty == Q4:
                n += 1
                x = s.tensor_bytes(name).view(np.float32).reshape(-1, ne[0])
                assert np.array_equal(g.tensor_bytes(name), q4.quantize_row_q4_0(x)), name
        assert n == 6 + 2 + 16 * 6
    q4.twin_gguf(dst, twin)  # the oracle computes no Q4_0 product: it runs the file's twin
    with ttship.Gguf(dst) as g, ttship.Gguf(twin) as t:
        k = ttship.Kokoro.from_gguf(py_oracle.iface(8), t, **RUN)
        try:
            raw = k.weights_raw()
            for name, ty, ne, _, _ in g.tensors():
                rn = name[len("kokoro."):]
                if rn in raw and "_norm" not in rn:
                    assert raw[rn][0] == (Q8 if ty == Q4 else ty), name
                    if ty == Q4:
                        assert np.array_equal(raw[rn][2], q4.twin_q8_0(g.tensor_bytes(name))), name
            assert sum(1 for ty, _, _ in raw.values() if ty == Q8) == n
            toks = tokens(9, 4)
            h, l = k.durations(toks)
            assert np.isfinite(h).all() and int(l.sum()) > 0
        finally:
            k.close()
