"""Q6_K on the host: type traits, the numpy reference of tests/q6_k_ref.py against a hand-built block, its quantizer's
round trip, that its product order can be told from another one on the GPU module's own inputs, the quantize tool's
Q4_K_M-style mix rule, its refusals, and a mix file written with the numpy row callback."""
import numpy as np
import pytest

import py_oracle
import q6_k_ref as q6
import ttship
from runner_gguf import DAC, DIA
from test_gguf_cpu import DAC_TINY, TINY, parse_gguf

F32, F16, Q4K, Q6K, Q8 = ttship.F32, ttship.F16, ttship.Q4_K, ttship.Q6_K, ttship.Q8_0
MIX = ttship.QUANT_MIX_Q4_K_M
TINY8 = dict(TINY, n_layers=8)
MORE_BITS_8 = (0, 3, 6, 7)  # more_bits(i, 8): i < 1 || i >= 7 || (i - 1) % 3 == 2


def test_type_traits():
    L = ttship.lib()
    assert Q6K == 14 and (L.tts_type_size(Q6K), L.tts_blck_size(Q6K)) == (210, 256)
    assert L.tts_row_size(Q6K, 768) == 630 and L.tts_type_name(Q6K) == b"q6_K"
    assert (ttship.TYPE_SIZE[Q6K], ttship.BLCK_SIZE[Q6K]) == (210, 256) and ttship.row_size(Q6K, 256) == 210


def test_supports_op_host_logic():
    import ctypes

    from test_abi_cpu import _t
    L = ttship.lib()
    L.tts_hip_supports_op.argtypes = [ctypes.POINTER(ttship.TtsTensor)]
    for K, want in ((128, 0), (256, 1), (384, 0), (1024, 1)):
        w = _t(Q6K, [max(K // 256, 1) * 256, 4])
        w.ne[0] = K
        mm = _t(F32, [4, 2], op=ttship.OP["MUL_MAT"], srcs=(w, _t(F32, [K, 2])))
        gr = _t(F32, [K, 2], op=ttship.OP["GET_ROWS"], srcs=(w, _t(ttship.I32, [2])))
        assert L.tts_hip_supports_op(ctypes.byref(mm)) == want, K
        assert L.tts_hip_supports_op(ctypes.byref(gr)) == want, K


def test_hand_built_block():
    """Known bytes -> a[e], the scale index and the dequantized value, element by element, in each 32-element group."""
    b = np.zeros(210, np.uint8)
    ql, qh, sc = b[:128], b[128:192], b[192:208].view(np.int8)
    b[208:210] = np.array([0.5], np.float16).view(np.uint8)
    sc[:] = np.arange(16) - 8  # scales[j] = j - 8
    # half 0, l = 5 (byte ql[5], ql[37], qh[5]) and l = 20 (ql[20], ql[52], qh[20])
    ql[5], ql[37], qh[5] = 0xA3, 0x4F, 0b11_10_01_00
    ql[20], ql[52], qh[20] = 0x07, 0xF0, 0b00_01_10_11
    # half 1, l = 0 (ql[64], ql[96], qh[32]) and l = 31 (ql[95], ql[127], qh[63])
    ql[64], ql[96], qh[32] = 0x21, 0x43, 0b01_00_11_10
    ql[95], ql[127], qh[63] = 0xFF, 0xFF, 0xFF
    want = {  # e: (a, scale index)
        5: ((0x3 | (0 << 4)) - 32, 0), 37: ((0xF | (1 << 4)) - 32, 2), 69: ((0xA | (2 << 4)) - 32, 4), 101: ((0x4 | (3 << 4)) - 32, 6),
        20: ((0x7 | (3 << 4)) - 32, 1), 52: ((0x0 | (2 << 4)) - 32, 3), 84: ((0x0 | (1 << 4)) - 32, 5), 116: ((0xF | (0 << 4)) - 32, 7),
        128: ((0x1 | (2 << 4)) - 32, 8), 160: ((0x3 | (3 << 4)) - 32, 10), 192: ((0x2 | (0 << 4)) - 32, 12), 224: ((0x4 | (1 << 4)) - 32, 14),
        159: (31, 9), 191: (31, 11), 223: (31, 13), 255: (31, 15),
        0: (-32, 0), 100: (-32, 6), 200: (-32, 12),  # untouched bytes: code 0
    }
    d, s, a = q6.unpack(b)
    y = q6.dequantize(b, 256, 1)[0]
    assert d[0] == 0.5 and list(s[0]) == list(range(-8, 8))
    for e, (av, si) in want.items():
        assert si == e // 16 and a[0, e] == av, e
        assert y[e] == np.float32(0.5 * (si - 8)) * np.float32(av), e
    assert np.array_equal(q6.pack(d, s, a.astype(np.int32) + 32), b)  # pack inverts unpack


def test_q8_K_restatement_equals_the_oracle():
    x = np.random.default_rng(3).standard_normal((2, 512)).astype(np.float32)
    x[1, 256:] = 0.0
    d, q = q6.quantize_row_q8_K(x)
    for m in range(2):
        out = np.zeros(2 * 292, np.uint8)
        py_oracle.lib().ref_quantize_row_q8_K(x[m].ctypes.data, out.ctypes.data, 512)
        blk = out.reshape(2, 292)
        assert np.array_equal(blk[:, :4].copy().view(np.float32).reshape(-1), d[m])
        assert np.array_equal(blk[:, 4:260].view(np.int8), q[m])


def _rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))


def test_round_trip_beats_q4_K():
    x = (np.random.default_rng(0).standard_normal((16, 512)) * 0.02).astype(np.float32)
    e6 = _rms(q6.dequantize(q6.quantize_row_q6_K(x), 512, 16), x)
    e4 = _rms(py_oracle.dequant_q4_K(py_oracle.quantize(Q4K, x), 512, 16), x)
    assert 0 < e6 < e4, (e6, e4)
    assert e6 < 0.02 / 32  # about 6 bits over a sub-block's range of a few sigma


def test_round_trip_zero_and_outlier():
    z = np.zeros((1, 256), np.float32)
    assert not q6.quantize_row_q6_K(z).any()  # an all-zero block is written as zeros
    assert np.array_equal(q6.dequantize(q6.quantize_row_q6_K(z), 256, 1), z)
    o = (np.random.default_rng(1).standard_normal((1, 512)) * 0.01).astype(np.float32)
    o[0, 77] = 3.0e4
    o[0, 256:272] = 0.0  # a zero sub-block in a live block: its scale is 0 and it keeps the search's L
    y = q6.dequantize(q6.quantize_row_q6_K(o), 512, 1)
    assert np.isfinite(y).all() and abs(y[0, 77] / 3.0e4 - 1) < 0.02 and not y[0, 256:272].any()
    tiny = np.full((1, 256), 1e-20, np.float32)  # below GROUP_MAX_EPS everywhere: zeros
    assert not q6.quantize_row_q6_K(tiny).any()


CASES = [(K, N, M) for K, N in q6.GEMV_SHAPES for M in q6.GEMV_COLS if N * M >= 32] + \
        [(K, N, M) for K, N in q6.GEMM_SHAPES for M in q6.GEMM_COLS if N * M >= 32]


@pytest.mark.parametrize("K,N,M", CASES)
def test_reference_tells_orders_apart(K, N, M):
    """On the GPU module's inputs the contract's chain and a one-sum-per-block chain differ in bits on at least a
    quarter of the outputs, and |aux32| < 2^24, so the int-to-float step is exact.  Every GEMV and many-column case of
    tests/test_q6_k_gpu.py is taken except those of fewer than 32 outputs (N * M < 32), where a quarter of a handful
    of sums says nothing either way."""
    w, x = q6.case(K, N, M)
    aux, _, _ = q6.aux32(w, x, N)
    assert np.abs(aux).max() < 2 ** 24
    a, b = q6.vec_dot_q6_K_q8_K(w, x, N), q6.vec_dot_one_sum_per_block(w, x, N)
    assert np.mean(a.view(np.uint32) != b.view(np.uint32)) >= 0.25
    assert np.allclose(a, b, rtol=1e-4, atol=1e-6 * np.abs(a).max())  # and still the same product
    deq = q6.dequantize(w, K, N).astype(np.float64)
    assert np.allclose(a, x.astype(np.float64) @ deq.T, rtol=0, atol=0.02 * np.abs(a).max())


# ---- the rule ----
def test_existing_rule_answers_unchanged_with_mix_0():
    r = ttship.gguf_tensor_rule
    names = [("parler-tts", n) for n in ("decoder.layers.3.fc1.weight", "decoder.layers.3.self_attn.v_proj.weight", "decoder.layer_norm.weight",
                                           "decoder.lm_heads.0.weight.head", "decoder.embed_prompts", "decoder.layers.1.encoder_attn.v_proj.weight",
                                           "audio_encoder.initial.weight")] + \
            [("dia", "dia.decoder.layers.0.self_attn.q_proj"), ("dia", "dia.decoder.heads.0"), ("kokoro", "kokoro.albert.layers.0.attn.q"),
             ("orpheus", "orpheus.layers.0.mlp.down_proj"), ("orpheus", "orpheus.lm_head"), ("orpheus", "orpheus.layers.0.input_norm.weight")]
    for kw in ({}, dict(quantize_output_heads=1, quantize_text_embeddings=1, quantize_cross_attn_kv=1), dict(convert_dac_to_f16=1)):
        for arch, n in names:
            base = r(arch, n, ttship.quantize_params(Q4K, **kw))
            if arch in ("parler-tts", "orpheus"):
                assert r(arch, n, ttship.quantize_params(Q4K, mix=MIX, **kw)) == base, (arch, n)  # the rule itself never sees the mix
            t = ttship.gguf_tensor_out_type(arch, n, 8, ttship.quantize_params(Q4K, **kw))
            assert t == {0: F32, 1: Q4K, 2: F16}[base], (arch, n)
    assert r("unknown-arch", "x") == -1 and ttship.gguf_tensor_out_type("unknown-arch", "x", 8) == -1


def _parler_mix_names(heads, cross):
    want = set()
    for i in MORE_BITS_8:
        want |= {f"decoder.layers.{i}.self_attn.v_proj.weight", f"decoder.layers.{i}.fc2.weight"}
        if cross:
            want.add(f"decoder.layers.{i}.encoder_attn.v_proj.weight")
    if heads:
        want |= {f"decoder.lm_heads.{h}.weight.head" for h in range(9)}
    return want


def _orpheus_mix_names(heads):
    want = {f"orpheus.layers.{i}.{m}" for i in MORE_BITS_8 for m in ("self_attn.v_proj", "mlp.down_proj")}
    return want | ({"orpheus.lm_head"} if heads else set())


@pytest.mark.parametrize("heads,cross", [(0, 0), (1, 0), (1, 1)])
def test_mix_rule_exact_sets(tmp_path, heads, cross):
    p = ttship.quantize_params(Q4K, mix=MIX, quantize_output_heads=heads, quantize_cross_attn_kv=cross)
    src = tmp_path / "p.gguf"
    ttship.write_parler_synthetic_gguf(src, ttship.parler_config(weight_type=F32, head_type=F32, **TINY8))
    with ttship.Gguf(src) as g:
        names = [t[0] for t in g.tensors()]
    got = {n for n in names if ttship.gguf_tensor_out_type("parler-tts", n, 8, p) == Q6K}
    assert got == _parler_mix_names(heads, cross)
    for n in names:  # everything else: what the rule alone says
        if n not in got:
            assert ttship.gguf_tensor_out_type("parler-tts", n, 8, p) == (Q4K if ttship.gguf_tensor_rule("parler-tts", n, p) == 1 else F32), n
    onames = [f"orpheus.layers.{i}.{m}" for i in range(8) for m in
              ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
               "mlp.down_proj", "input_norm", "post_attention_norm")] + \
             ["orpheus.embed_tokens", "orpheus.lm_head", "orpheus.norm", "orpheus.rope_frequencies", "snac.decoder.x"]
    po = ttship.quantize_params(Q4K, mix=MIX, quantize_output_heads=heads)
    assert {n for n in onames if ttship.gguf_tensor_out_type("orpheus", n, 8, po) == Q6K} == _orpheus_mix_names(heads)
    # the predicate at another depth: n = 28 (Orpheus-3B) -> 0 1 2, 5 8 11 .. 23, 24 .. 27
    more = [i for i in range(28) if ttship.gguf_tensor_out_type("orpheus", f"orpheus.layers.{i}.mlp.down_proj", 28, po) == Q6K]
    assert more == [i for i in range(28) if i < 3 or i >= 24 or (i - 3) % 3 == 2]


def _numpy_rows(ttype, x):
    return q6.quantize_row_q6_K(x) if ttype == Q6K else py_oracle.quantize(ttype, x)


def test_refusals(tmp_path, capfd):
    t = ttship.gguf_tensor_out_type
    assert t("dia", "dia.decoder.layers.0.self_attn.q_proj", 8, ttship.quantize_params(Q4K, mix=MIX)) < 0
    assert t("kokoro", "kokoro.albert.layers.0.attn.q", 8, ttship.quantize_params(Q4K, mix=MIX)) < 0
    assert t("kokoro", "kokoro.albert.layers.0.attn.q", 8, ttship.quantize_params(Q6K)) < 0
    assert t("parler-tts", "decoder.layers.0.fc2.weight", 8, ttship.quantize_params(Q8, mix=MIX)) < 0
    assert t("parler-tts", "decoder.layers.0.fc2.weight", 8, ttship.quantize_params(Q4K, mix=7)) < 0
    # the tool itself
    dia, par, rag = tmp_path / "dia.gguf", tmp_path / "parler.gguf", tmp_path / "ragged.gguf"
    ttship.write_dia_synthetic_gguf(dia, ttship.dia_config(**dict(DIA, weight_type=F32, head_type=F32)), ttship.dac_config(**DAC))
    ttship.write_parler_synthetic_gguf(par, ttship.parler_config(weight_type=F32, head_type=F32, **TINY))
    out = tmp_path / "out.gguf"
    with pytest.raises(RuntimeError):
        ttship.quantize_gguf(dia, out, ttship.quantize_params(Q4K, mix=MIX), rows_fn=_numpy_rows)
    with pytest.raises(RuntimeError):
        ttship.quantize_gguf(par, out, ttship.quantize_params(Q8, mix=MIX), rows_fn=_numpy_rows)
    assert not out.exists()
    # a quantizable tensor whose rows are no multiple of 256 long fails the run with its name
    w = ttship.GgufWriter()
    w.set("general.architecture", "parler-tts")
    w.add_tensor("decoder.layers.0.fc2.weight", F32, [384, 4], np.zeros((4, 384), np.float32))
    w.write(rag)
    w.close()
    capfd.readouterr()
    for p in (ttship.quantize_params(Q6K), ttship.quantize_params(Q4K, mix=MIX)):
        with pytest.raises(RuntimeError):
            ttship.quantize_gguf(rag, out, p, rows_fn=_numpy_rows)
        assert "decoder.layers.0.fc2.weight" in capfd.readouterr().err


def test_kokoro_plain_q6_K_is_refused(tmp_path):
    from test_kokoro_quant_cpu import TINYQ
    src = tmp_path / "k.gguf"
    ttship.write_kokoro_synthetic_gguf(src, ttship.kokoro_config(**TINYQ))
    with pytest.raises(RuntimeError):
        ttship.quantize_gguf(src, tmp_path / "o.gguf", ttship.quantize_params(Q6K), rows_fn=_numpy_rows)


@pytest.fixture(scope="module")
def mix_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("q6k_cpu")
    src, mix, plain, plain0 = d / "parler8-f32.gguf", d / "parler8-mix.gguf", d / "parler8-q4k.gguf", d / "parler8-q4k-mix0.gguf"
    ttship.write_parler_synthetic_gguf(src, ttship.parler_config(weight_type=F32, head_type=F32, **TINY8), ttship.dac_config(**DAC_TINY))
    ttship.quantize_gguf(src, mix, ttship.quantize_params(Q4K, mix=MIX, quantize_output_heads=1), rows_fn=_numpy_rows)
    ttship.quantize_gguf(src, plain, ttship.quantize_params(Q4K, quantize_output_heads=1), rows_fn=_numpy_rows)
    ttship.quantize_gguf(src, plain0, ttship.quantize_params(Q4K, quantize_output_heads=1, mix=0), rows_fn=_numpy_rows)
    return src, mix, plain, plain0


def test_mix_file_layout(mix_files):
    """The mix file through the independent parser: types where the rule puts them, 210 * K / 256 bytes per Q6_K row,
    KV pairs copied; with mix = 0 the tool writes the same bytes as before the field existed."""
    src, mix, plain, plain0 = mix_files
    assert plain.read_bytes() == plain0.read_bytes()
    _, kv0, infos0, _, _ = parse_gguf(src)
    _, kv, infos, data0, raw = parse_gguf(mix)
    _, _, infos4, _, _ = parse_gguf(plain)
    for k, v in kv0.items():
        assert kv[k] == v, k
    assert kv["general.quantization_type"] == Q4K and kv["general.quantization_version"] == 2
    assert [i[0] for i in infos] == [i[0] for i in infos0]
    want6 = _parler_mix_names(1, 0)
    got6 = set()
    offs = sorted(i[3] for i in infos) + [len(raw) - data0]
    with ttship.Gguf(src) as g:
        for (name, ne, ty, off), (_, _, ty4, _) in zip(infos, infos4):
            size = offs[offs.index(off) + 1] - off
            if ty == Q6K:
                got6.add(name)
                assert ty4 == Q4K and ne[0] % 256 == 0, name
                rows = int(np.prod(ne[1:]))
                nbytes = rows * 210 * ne[0] // 256
                assert nbytes <= size < nbytes + 32, name
                x = g.tensor_bytes(name).view(np.float32).reshape(rows, ne[0])
                got = np.frombuffer(raw, np.uint8, nbytes, data0 + off)
                assert np.array_equal(got, q6.quantize_row_q6_K(x)), name
            else:
                assert ty == ty4, name
    assert got6 == want6
    with ttship.Gguf(mix) as g:
        cfg = ttship.parler_config_from_gguf(g, max_ctx=TINY["max_ctx"])
        assert cfg.weight_type == Q4K and cfg.head_type == Q6K and cfg.n_layers == 8


def test_synthetic_q6_K_file(tmp_path):
    cfg = ttship.parler_config(weight_type=Q6K, head_type=F32, **TINY)
    path = tmp_path / "parler-q6k-synth.gguf"
    ttship.write_parler_synthetic_gguf(path, cfg)
    with ttship.Gguf(path) as g:
        ts = {t[0]: t for t in g.tensors()}
        for name, std in (("decoder.layers.1.fc1.weight", 0.02), ("decoder.embed_tokens.3.weight", 0.25)):
            _, ty, ne, _, nbytes = ts[name]
            assert ty == Q6K and nbytes == ne[0] * ne[1] // 256 * 210
            w = q6.dequantize(g.tensor_bytes(name), ne[0], ne[1])
            assert abs(w.std() / std - 1) < 0.2 and abs(w.mean()) < 0.2 * std, (name, w.std(), w.mean())


def test_synthetic_orpheus_weight_mix():
    """tts_orpheus_config.weight_mix: the synthetic runner's tensors take the types the tool's mix gives a file's."""
    from runner_gguf import ORPHEUS, orpheus_name_map
    cfg = ttship.orpheus_config(**dict(ORPHEUS, n_layers=8, weight_type=Q4K, weight_mix=MIX))
    p = ttship.quantize_params(Q4K, mix=MIX, quantize_output_heads=1)
    o = ttship.Orpheus(py_oracle.iface(2), cfg)
    try:
        raw = o.weights_raw()
    finally:
        o.close()
    names = orpheus_name_map()  # (written for the 2-layer tiny model: the other layers' names follow layer 0's)
    for l in range(2, 8):
        names.update({k.replace("layers.0.", f"layers.{l}."): v.replace("layers.0.", f"layers.{l}.") for k, v in list(names.items()) if k.startswith("layers.0.")})
    n6 = 0
    for rn, (ty, _, _) in raw.items():
        fname = "orpheus." + names.get(rn, rn)
        if ty in (Q4K, Q6K):
            assert ty == ttship.gguf_tensor_out_type("orpheus", fname, 8, p), (rn, fname, ty)
            n6 += ty == Q6K
    assert n6 == 2 * len(MORE_BITS_8) + 1
    plain = ttship.Orpheus(py_oracle.iface(2), ttship.orpheus_config(**dict(ORPHEUS, n_layers=8, weight_type=Q4K)))
    try:
        assert not any(ty == Q6K for ty, _, _ in plain.weights_raw().values())
    finally:
        plain.close()
