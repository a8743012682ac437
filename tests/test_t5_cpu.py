"""T5 voice-description encoder runner (tts.cpp_amd/csrc/t5.cpp) on the CPU oracle: shapes, the node
order of build_t5_graph (/root/reference/src/models/parler/t5/model.cpp:216-298), the position buckets
of t5_runner::set_inputs, the planner's view of the graph (no device), the GGUF round trip, and the
voice description handed to the Parler runner at run time (tts_parler_set_conditional_prompt)."""
import math

import numpy as np
import pytest

import attn_bias_chain as abc
import nodes as nd
import py_oracle
import ttship

TINY = dict(n_layers=2, hidden_size=128, n_attn_heads=2, head_size=64, ffn_size=256, vocab_size=96, max_context_length=160,
            output_size=96, has_down_proj=1, weight_type=ttship.F32)
TINY_F16 = dict(TINY, n_attn_heads=4, has_down_proj=0, weight_type=ttship.F16)


def tokens(n, vocab=96, seed=0):
    t = np.random.default_rng(100 + n + seed).integers(2, vocab, n).astype(np.int32)
    t[-1] = 1  # EOS
    return t


def reference_bucket(key, query, buckets=32):
    """t5_runner::set_inputs' formula as written (t5/model.cpp:308-316): the logarithm takes an integer
    quotient, its denominator is a float, the maximum distance is the literal 128."""
    n_buckets = buckets // 2
    max_exact = n_buckets // 2
    den = float(np.float32(math.log(128.0 / max_exact)))
    ab, rpos = abs(key - query), key - query
    big = min(n_buckets - 1, max_exact + int(math.log(ab // max_exact) / den * max_exact)) if ab >= max_exact else ab
    return (n_buckets if rpos > 0 else 0) + big


def test_output_shapes_and_context_limit():
    t = ttship.T5(py_oracle.iface(4), ttship.t5_config(**TINY))
    u = ttship.T5(py_oracle.iface(4), ttship.t5_config(**TINY_F16))
    try:
        assert t.output_size == 96 and u.output_size == 128
        for n in (1, 7):
            a, b = t.encode(tokens(n)), u.encode(tokens(n))
            assert a.shape == (n, 96) and b.shape == (n, 128)
            assert np.isfinite(a).all() and np.isfinite(b).all()
        assert t.encode(tokens(160)).shape == (160, 96)
        with pytest.raises(RuntimeError):
            t.encode(tokens(161))  # n > max_context_length
        # one token's encoding depends on its neighbours (attention runs), and on nothing after a reset of inputs
        a = t.encode(tokens(7))
        assert np.array_equal(a, t.encode(tokens(7)))
        assert not np.array_equal(a[0], t.encode(tokens(7)[:1])[0])
    finally:
        t.close()
        u.close()


def test_node_order_is_the_builders():
    t = ttship.T5(py_oracle.iface(2), ttship.t5_config(**TINY))
    try:
        t.encode(tokens(6))
        ops = [t.node(i, cap=4)[0] for i in range(t.last_graph_nodes())]
    finally:
        t.close()
    head = ["GET_ROWS",                                           # embedding
            "VIEW", "GET_ROWS", "VIEW", "PERMUTE", "CONT"]        # build_t5_pos_bias
    attn = ["MUL_MAT"] * 3 + ["RESHAPE"] * 2 + ["PERMUTE", "PERMUTE", "CONT", "MUL_MAT", "ADD", "SOFT_MAX", "TRANSPOSE", "CONT",
                                                  "MUL_MAT", "PERMUTE", "CONT", "MUL_MAT", "ADD"]
    mlp = ["RMS_NORM", "MUL", "MUL_MAT", "MUL_MAT", "UNARY", "MUL", "MUL_MAT", "ADD"]
    layer = ["RMS_NORM", "MUL"] + attn + mlp
    want = head + layer
    assert ops[:len(want)] == want, ops[:len(want)]
    tail = ["RMS_NORM", "MUL", "MUL_MAT", "ADD"]                  # final norm, down_proj, its bias
    assert ops == head + layer * TINY["n_layers"] + tail


def test_pos_buckets_follow_the_reference_formula():
    import torch
    from transformers.models.t5.modeling_t5 import T5Attention
    n = 40
    t = ttship.T5(py_oracle.iface(2), ttship.t5_config(**TINY))
    try:
        t.encode(tokens(n))
        got = t.named("pos_bucket", "int32").reshape(n, n)  # [key][query]
    finally:
        t.close()
    want = np.array([[reference_bucket(i, ii) for ii in range(n)] for i in range(n)], dtype=np.int32)
    assert np.array_equal(got, want)
    rel = torch.arange(n)[:, None] - torch.arange(n)[None, :]  # key - query, [key][query]
    hf = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=32, max_distance=128).numpy()
    d = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    assert np.array_equal(got[d <= 11], hf[d <= 11])  # the two formulas agree up to distance 11
    differs = sorted(set(d[got != hf].tolist()))
    assert differs and differs[0] == 12, differs  # ... and part at 12-15, 23, ...


def test_planner_fuses_every_layers_attention():
    t = ttship.T5(py_oracle.iface(4), ttship.t5_config(**TINY))
    try:
        for n in (5, 130):
            t.encode(tokens(n))
            st = t.plan_stats()
            assert st["attn"] == TINY["n_layers"], (n, st)
            off = t.plan_stats(ttship.FUSE_ALL & ~ttship.FUSE["ATTN"])
            assert off["attn"] == 0, (n, off)
            # the fused item takes ADD, SOFT_MAX, both products and the K / V / output copies with it
            assert off["unfused"] - st["unfused"] == 7 * TINY["n_layers"], (n, st, off)
    finally:
        t.close()


@pytest.mark.parametrize("P,n,H,hd,want", [(65, 65, 2, 64, 1), (512, 3, 2, 64, 1), (513, 16, 2, 64, 0), (40, 16, 2, 128, 0)])
def test_planner_range_on_a_hand_built_chain(P, n, H, hd, want):
    g = nd.Graph()
    abc.build(g, *abc.inputs(P, n, H, hd))
    assert abc.plan(g)["attn"] == want
    assert abc.plan(g, ttship.FUSE_ALL & ~ttship.FUSE["ATTN"])["attn"] == 0


@pytest.mark.parametrize("out_on", ["q", "k", "v"])
def test_output_on_an_operands_memory_still_fuses(out_on):
    """A graph allocator hands an operand's memory to the attention output (the T5 runner's does): fused all the same
    (in place over q's rows, through the backend's staging buffer over k or v; tests/test_attn_bias_gpu.py runs it)."""
    g = nd.Graph()
    abc.build(g, *abc.inputs(20, 20, 2, 64), out_on=out_on)
    assert abc.plan(g)["attn"] == 1


def test_broadcast_bias_stays_unfused():
    q, k, v, bias, mask = abc.inputs(20, 6, 2, 64)
    g = nd.Graph()
    abc.build(g, q, k, v, bias[:1], mask)  # one head's bias for every head: ne [P, n, 1]
    assert abc.plan(g)["attn"] == 0


KEYS = ("gemv", "attn", "ln", "embed", "mcpy", "rint", "node", "copy", "gemv_products", "xattn", "unfused")
# recorded from the commit before the bias pattern existed (same configs, same calls)
PARENT = {
    "parler_prefill_b1": (19, 6, 10, 1, 0, 0, 0, 6, 33, 0, 10),
    "parler_decode_b1": (19, 6, 10, 1, 0, 0, 0, 0, 33, 3, 1),
    "parler_prefill_b3": (18, 5, 9, 0, 0, 0, 0, 6, 24, 0, 17),
    "parler_decode_b3": (19, 6, 10, 1, 0, 0, 0, 0, 33, 3, 0),
    "dia_prefill": (23, 4, 10, 1, 0, 4, 10, 14, 38, 0, 39),
    "dia_decode": (16, 4, 7, 1, 0, 4, 6, 10, 27, 0, 16),
    "orpheus_prefill": (11, 2, 5, 0, 2, 0, 4, 4, 15, 0, 10),
    "orpheus_decode": (11, 2, 5, 0, 2, 0, 2, 2, 15, 0, 5),
}


def test_existing_step_graphs_plan_as_before():
    got = {}

    def rec(tag, st):
        got[tag] = tuple(st[k] for k in KEYS)

    P = dict(n_layers=3, hidden_size=256, n_attn_heads=4, ffn_size=1024, output_vocab=1088, max_ctx=96, prompt_vocab=512, max_positions=128)
    for batch in (1, 3):
        c = ttship.Parler(py_oracle.iface(2), ttship.parler_config(batch=batch, **P))
        c.prefill((np.arange(6 * batch, dtype=np.int32).reshape(batch, 6) * 41) % 512)
        rec(f"parler_prefill_b{batch}", c.plan_stats())
        c.decode(np.full((batch, 9), 7, dtype=np.int32))
        rec(f"parler_decode_b{batch}", c.plan_stats())
        c.close()
    D = dict(n_encoder_layers=1, n_decoder_layers=2, encoder_hidden_size=64, decoder_hidden_size=128, encoder_attn_heads=4,
             decoder_attn_heads=4, decoder_query_heads=2, head_size=32, encoder_ffn_size=128, decoder_ffn_size=256,
             max_generation_size=64, max_encoder_context_length=32)
    d = ttship.Dia(py_oracle.iface(4), ttship.dia_config(**D))
    lg = d.prefill(np.frombuffer(b"\x01 hello there.", dtype=np.uint8).astype(np.int32), np.full(9, 1026, dtype=np.int32))
    rec("dia_prefill", d.plan_stats())
    d.decode(lg.argmax(axis=1).astype(np.int32))
    rec("dia_decode", d.plan_stats())
    d.close()
    O = dict(n_layers=2, hidden_size=256, n_attn_heads=4, n_kv_attn_heads=2, head_size=64, ffn_size=512, vocab_size=1000, max_ctx=48)
    o = ttship.Orpheus(py_oracle.iface(2), ttship.orpheus_config(**O))
    o.prefill(np.arange(4, dtype=np.int32)[None])
    rec("orpheus_prefill", o.plan_stats())
    o.decode(np.array([7], dtype=np.int32))
    rec("orpheus_decode", o.plan_stats())
    o.close()
    assert got == PARENT


@pytest.mark.parametrize("cfg", [TINY, TINY_F16], ids=["f32_down_proj", "f16"])
def test_gguf_round_trip_is_bit_identical(tmp_path, cfg):
    c = ttship.t5_config(**cfg)
    path = tmp_path / "t5.gguf"
    ttship.write_t5_synthetic_gguf(path, c)
    a = ttship.T5(py_oracle.iface(4), c)
    with ttship.Gguf(path) as g:
        fc = ttship.t5_config_from_gguf(g)
        for f in ("n_layers", "hidden_size", "n_attn_heads", "head_size", "ffn_size", "relative_attn_buckets", "vocab_size",
                  "max_context_length", "has_down_proj", "weight_type", "eos_token_id"):
            assert getattr(fc, f) == getattr(c, f), f
        b = ttship.T5.from_gguf(py_oracle.iface(4), g)
        try:
            assert b.output_size == a.output_size
            wa, wb = a.weights(), b.weights()
            assert list(wa) == list(wb) and len(wa) == 2 + 9 * cfg["n_layers"] + 1 + 2 * cfg["has_down_proj"]
            for k in wa:
                assert np.array_equal(wa[k], wb[k]), k
            assert np.array_equal(a.encode(tokens(9)), b.encode(tokens(9)))
        finally:
            a.close()
            b.close()


def test_gguf_without_vocab_size_is_refused(tmp_path):
    w = ttship.GgufWriter()
    w.set("general.architecture", "t5encoder")
    w.add_tensor("t5encoder.enc.blk.0.attn_q", ttship.F32, [4, 4], np.zeros((4, 4), np.float32))
    w.write(tmp_path / "bad.gguf")
    w.close()
    with ttship.Gguf(tmp_path / "bad.gguf") as g:
        with pytest.raises(RuntimeError):
            ttship.t5_config_from_gguf(g)


# ---- the voice description at run time ----
PARLER = dict(n_layers=2, hidden_size=128, n_attn_heads=2, ffn_size=256, max_ctx=48, prompt_vocab=300, max_positions=64,
              weight_type=ttship.F32, head_type=ttship.F32, batch=1)


def decode3(p, cfg):
    p.prefill((np.arange(5, dtype=np.int32)[None] * 13) % cfg.prompt_vocab)
    out, audio = [], np.full((1, cfg.n_output_heads), cfg.bos_token, dtype=np.int32)
    for _ in range(3):
        lg = p.decode(audio)
        out.append(lg)
        audio = lg.argmax(-1).astype(np.int32)
    return np.stack(out)


def test_set_conditional_prompt():
    cfg = ttship.parler_config(**PARLER)
    fresh = ttship.Parler(py_oracle.iface(4), cfg)
    p = ttship.Parler(py_oracle.iface(4), cfg)
    try:
        want = decode3(fresh, cfg)
        own = p.weights()["text_encoding"].reshape(cfg.n_encode, cfg.hidden_size)
        decode3(p, cfg)  # positions and cache in use: the call must reset them
        p.set_conditional_prompt(own)
        assert p.position == 0
        assert np.array_equal(decode3(p, cfg), want)  # the runner's own encoding: nothing changes
        other = np.random.default_rng(3).standard_normal(own.shape).astype(np.float32)
        p.set_conditional_prompt(other)
        changed = decode3(p, cfg)
        assert np.isfinite(changed).all() and not np.array_equal(changed, want)
        assert np.array_equal(p.weights()["text_encoding"].reshape(own.shape), other)
        # a wrong length is refused and changes nothing
        with pytest.raises(ValueError):
            p.set_conditional_prompt(np.zeros((cfg.n_encode + 1, cfg.hidden_size), np.float32))
        p.reset()
        assert np.array_equal(decode3(p, cfg), changed)
        p.set_conditional_prompt(own)
        assert np.array_equal(decode3(p, cfg), want)
    finally:
        fresh.close()
        p.close()


def test_set_conditional_prompt_needs_cross_attention():
    cfg = ttship.parler_config(**dict(PARLER, use_cross_attn=0))
    p = ttship.Parler(py_oracle.iface(2), cfg)
    try:
        with pytest.raises(ValueError):
            p.set_conditional_prompt(np.zeros((cfg.n_encode, cfg.hidden_size), np.float32))
    finally:
        p.close()


def test_t5_encoding_drives_parler_end_to_end():
    n = 6
    t = ttship.T5(py_oracle.iface(4), ttship.t5_config(**dict(TINY, output_size=PARLER["hidden_size"])))
    cfg = ttship.parler_config(**dict(PARLER, n_encode=n))
    p = ttship.Parler(py_oracle.iface(4), cfg)
    try:
        before = decode3(p, cfg)
        enc = t.encode(tokens(n))
        assert enc.shape == (n, cfg.hidden_size)
        p.set_conditional_prompt(enc)
        after = decode3(p, cfg)
        assert np.isfinite(after).all() and after.shape == before.shape
        assert not np.array_equal(after, before)
    finally:
        t.close()
        p.close()
