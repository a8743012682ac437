"""Dia, Orpheus and SNAC from GGUF files, on the host (the CPU oracle's interface): the written files carry the
reference's names and keys, an F32 file loads to the synthetic runner's weights and logits whatever the order of its
tensors, a file from the quantize tool has its types where the tool's rule puts them and runs to the logits of a
synthetic runner holding the same bytes, and a file the runner cannot take is refused without a crash."""
import numpy as np
import pytest

import py_oracle
import runner_gguf as rg
import ttship
from runner_gguf import F16, F32, Q4_0, Q4_K, Q5_0, Q8_0


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return rg.write_f32(tmp_path_factory.mktemp("runner_gguf"))


@pytest.fixture(scope="module")
def it():
    return py_oracle.iface(4)


# ---- names and keys: against the reference's scheme, spelled out in runner_gguf.py ----
def _listing(g, prefixes):
    return {name: tuple(ne) for name, _, ne, _, _ in g.tensors() if name.startswith(prefixes)}


def test_dia_file_names_and_keys(files, tmp_path):
    with ttship.Gguf(files[0]) as g:
        assert sorted(g.keys()) == sorted(rg.DIA_KEYS)
        assert g.get("general.architecture") == "dia"
        c = rg.DIA
        want = {"dia.attn_head_size": c["head_size"], "dia.eos_token_id": 1024, "dia.bos_token_id": 1026, "dia.pad_token_id": 1025,
                "dia.max_delay": 15, "dia.encoder.max_context_length": c["max_encoder_context_length"],
                "dia.encoder.attn_heads": c["encoder_attn_heads"], "dia.encoder.layers": c["n_encoder_layers"],
                "dia.decoder.hidden_size": c["decoder_hidden_size"], "dia.decoder.layers": c["n_decoder_layers"],
                "dia.decoder.output_heads": 9, "dia.decoder.attn_heads": c["decoder_attn_heads"],
                "dia.decoder.query_heads": c["decoder_query_heads"], "dia.decoder.output_vocab_size": 1028,
                "dia.decoder.audio_vocab_size": 1024, "dia.decoder.max_generation_size": c["max_generation_size"],
                "dac.up_scaling_factor": 16, "dac.dac_layer_stride_3": 2, "dac.dac_layer_padding_3": 1}
        for k, v in want.items():
            assert g.get(k) == v, k
        assert _listing(g, "dia.") == rg.dia_file_tensors()
        assert all(ty == F32 for _, ty, _, _, _ in g.tensors())
        dac = _listing(g, "audio_encoder.")
        rest = [n for n, *_ in g.tensors() if not n.startswith(("dia.", "audio_encoder."))]
    assert rest == []
    # the DAC half is the one the Parler writer has always written
    par = tmp_path / "parler.gguf"
    ttship.write_parler_synthetic_gguf(par, ttship.parler_config(n_layers=1, hidden_size=64, n_attn_heads=2, ffn_size=64, prompt_vocab=8,
                                                                 max_positions=8, max_ctx=8, weight_type=F32), ttship.dac_config(**rg.DAC))
    with ttship.Gguf(par) as p:
        assert dac == _listing(p, "audio_encoder.") and len(dac) > 0
    # cfg_scale is no key of the converter's: written only when it is not the reference's default
    other = tmp_path / "scale.gguf"
    ttship.write_dia_synthetic_gguf(other, rg.dia_cfg(weight_type=F32, cfg_scale=2.5))
    with ttship.Gguf(other) as g:
        assert g.get("dia.cfg_scale") == 2.5 and "dac.up_scaling_factor" not in g.keys()
        assert ttship.dia_config_from_gguf(g).cfg_scale == 2.5


def test_orpheus_file_names_and_keys(files, it):
    with ttship.Gguf(files[1]) as g:
        assert sorted(g.keys()) == sorted(rg.ORPHEUS_KEYS)
        c = rg.ORPHEUS
        want = {"general.architecture": "orpheus", "orpheus.stopping_token_id": 128258, "orpheus.hidden_size": c["hidden_size"],
                "orpheus.vocab_size": c["vocab_size"], "orpheus.attn_heads": c["n_attn_heads"], "orpheus.kv_attn_heads": c["n_kv_attn_heads"],
                "orpheus.head_dim": c["head_size"], "orpheus.layers": c["n_layers"],
                "orpheus.kv_hidden_size": c["hidden_size"] // (c["n_attn_heads"] // c["n_kv_attn_heads"]), "snac.audio_token_channels": 3}
        for l, s in enumerate(rg.SNAC["rates"]):
            want[f"snac.snac_layer_stride_{l}"] = s
            want[f"snac.snac_layer_padding_{l}"] = (s + 1) // 2
            want[f"snac.snac_layer_grouping_{l}"] = rg.SNAC["decoder_dim"] >> (l + 1)  # depthwise residual units
        for k, v in want.items():
            assert g.get(k) == v, k
        assert _listing(g, "orpheus.") == rg.orpheus_file_tensors()
        assert _listing(g, "snac.") == rg.snac_file_tensors()
        assert len(g.tensors()) == len(rg.orpheus_file_tensors()) + len(rg.snac_file_tensors())
        rope = g.tensor_bytes("orpheus.rope_frequencies").view(np.float32)
    o = ttship.Orpheus(it, rg.orpheus_cfg(weight_type=F32))
    try:
        held = o.weights_raw()["rope_frequencies"][2].view(np.float32)
    finally:
        o.close()
    assert np.array_equal(rope, held) and rope.min() >= 1.0 and rope.max() == 32.0  # the Llama-3 factors tts_orpheus_create computes


# ---- round trip ----
def test_config_round_trip(files):
    with ttship.Gguf(files[0]) as g:
        c = ttship.dia_config_from_gguf(g, seed=77, arena_bytes=rg.ARENA)
        w = rg.dia_cfg(weight_type=F32, head_type=F32)
        for k, _ in w._fields_:
            if k not in ("seed", "arena_bytes"):
                assert getattr(c, k) == getattr(w, k), k
        assert c.seed == 77 and c.arena_bytes == rg.ARENA
        d = ttship.dac_config_from_gguf(g, max_frames=16)
        assert d.n_codebooks == 9 and list(d.rates[:d.n_layers]) == rg.DAC["rates"]
    with ttship.Gguf(files[1]) as g:
        c = ttship.orpheus_config_from_gguf(g, batch=2, max_ctx=48, seed=5, arena_bytes=rg.ARENA, rope_theta=1.0)
        w = rg.orpheus_cfg(weight_type=F32)
        for k in ("n_layers", "hidden_size", "n_attn_heads", "n_kv_attn_heads", "head_size", "ffn_size", "vocab_size", "weight_type"):
            assert getattr(c, k) == getattr(w, k), k
        assert (c.batch, c.max_ctx, c.seed, c.arena_bytes, c.rope_theta) == (2, 48, 5, rg.ARENA, 1.0)
        s = ttship.snac_config_from_gguf(g, max_frames=24, seed=9)
        w = ttship.snac_config(**rg.SNAC)
        for k in ("n_heads", "codebook_size", "codebook_dim", "latent_dim", "decoder_dim", "n_layers"):
            assert getattr(s, k) == getattr(w, k), k
        assert list(s.rates) == list(w.rates) and list(s.repeats) == list(w.repeats) and (s.max_frames, s.seed) == (24, 9)
        with pytest.raises(RuntimeError):
            ttship.dia_config_from_gguf(g)  # an Orpheus file is no Dia file
    with ttship.Gguf(files[0]) as g:
        with pytest.raises(RuntimeError):
            ttship.orpheus_config_from_gguf(g)
        with pytest.raises(RuntimeError):
            ttship.snac_config_from_gguf(g)


def _same_weights(a, b):
    wa, wb = a.weights_raw(), b.weights_raw()
    assert list(wa) == list(wb)
    for name in wa:
        assert wa[name][:2] == wb[name][:2] and np.array_equal(wa[name][2], wb[name][2]), name


def _check_loaded_bytes(runner, g, prefix, name_map):
    """Every weight of the runner holds the bytes and the type of the file tensor the reference's names map it to."""
    raw = runner.weights_raw()
    assert sorted(raw) == sorted(name_map)
    for name, (ty, _, data) in raw.items():
        fname = prefix + name_map[name]
        assert ty == g.tensor_type(fname) and np.array_equal(data, g.tensor_bytes(fname)), fname


def test_dia_f32_file_equals_synthetic_runner(files, it):
    ref = ttship.Dia(it, rg.dia_cfg(weight_type=F32, head_type=F32))
    with ttship.Gguf(files[0]) as g:
        _check_loaded_bytes(ref, g, "dia.", rg.dia_name_map())  # the writer put each weight under the reference's name
        run = ttship.Dia.from_gguf(it, g, arena_bytes=rg.ARENA)
        dac = ttship.Dac(it, ttship.dac_config_from_gguf(g, max_frames=16), gguf=g)
    dac0 = ttship.Dac(it, ttship.dac_config(**rg.DAC))
    try:  # the mapping is closed: a runner holds its own copy of the weights
        _same_weights(run, ref)
        assert run.weight_bytes() == ref.weight_bytes()
        assert np.array_equal(rg.dia_logits(run), rg.dia_logits(ref))
        _same_weights(dac, dac0)
        assert np.array_equal(dac.decode(rg.dac_codes(4)), dac0.decode(rg.dac_codes(4)))
    finally:
        for r in (run, ref, dac, dac0):
            r.close()


def test_orpheus_f32_file_equals_synthetic_runner(files, it):
    ref = ttship.Orpheus(it, rg.orpheus_cfg(weight_type=F32))
    with ttship.Gguf(files[1]) as g:
        _check_loaded_bytes(ref, g, "orpheus.", rg.orpheus_name_map())
        run = ttship.Orpheus.from_gguf(it, g, max_ctx=rg.ORPHEUS["max_ctx"], arena_bytes=rg.ARENA)
    try:
        _same_weights(run, ref)
        assert np.array_equal(rg.orpheus_logits(run), rg.orpheus_logits(ref))
    finally:
        run.close()
        ref.close()


def test_snac_f32_file_equals_synthetic_runner(files, it):
    ref = ttship.Snac(it, ttship.snac_config(**rg.SNAC))
    with ttship.Gguf(files[1]) as g:
        run = ttship.Snac.from_gguf(it, g, max_frames=rg.SNAC["max_frames"])
    try:
        wa, wb = run.weights(), ref.weights()
        assert list(wa) == list(wb) and "one" in wa  # the constant 1.0 is the runner's own, not a file tensor
        assert sorted("snac." + n for n in wb if n != "one") == sorted(rg.snac_file_tensors())  # the runner's names are the file's
        with ttship.Gguf(files[1]) as g:
            for name in wa:
                assert np.array_equal(wa[name], wb[name]), name
                if name != "one":
                    assert np.array_equal(g.tensor_bytes("snac." + name).view(np.float32), wb[name].reshape(-1)), name
        heads, z = rg.snac_inputs(8, run.noise_per_frame)
        pcm = run.decode(heads, z)
        assert np.array_equal(pcm, ref.decode(heads, z)) and pcm.shape == (8 * run.hop,) and np.abs(pcm).max() > 0
    finally:
        run.close()
        ref.close()


# ---- order independence ----
def test_files_load_in_any_tensor_order(files, it, tmp_path):
    dia = rg.rebuilt(files[0], tmp_path / "dia-rev.gguf", reverse=True, extra=True)
    orph = rg.rebuilt(files[1], tmp_path / "orpheus-rev.gguf", reverse=True, extra=True)
    with ttship.Gguf(dia) as g, ttship.Gguf(files[0]) as g0:
        assert g.get("tokenizer.ggml.tokens") == ["<s>", "hello", "</s>"] and g.tensors()[0][0] == "unrelated.table"
        assert [t[0] for t in g.tensors()[1:]] == [t[0] for t in reversed(g0.tensors())]
        a, b = ttship.Dia.from_gguf(it, g, arena_bytes=rg.ARENA), ttship.Dia.from_gguf(it, g0, arena_bytes=rg.ARENA)
        da, db = (ttship.Dac(it, ttship.dac_config_from_gguf(x, max_frames=16), gguf=x) for x in (g, g0))
    try:
        assert np.array_equal(rg.dia_logits(a), rg.dia_logits(b))
        assert np.array_equal(da.decode(rg.dac_codes(4)), db.decode(rg.dac_codes(4)))
    finally:
        for r in (a, b, da, db):
            r.close()
    kw = dict(max_ctx=rg.ORPHEUS["max_ctx"], arena_bytes=rg.ARENA)
    with ttship.Gguf(orph) as g, ttship.Gguf(files[1]) as g0:
        a, b = ttship.Orpheus.from_gguf(it, g, **kw), ttship.Orpheus.from_gguf(it, g0, **kw)
        sa, sb = ttship.Snac.from_gguf(it, g, max_frames=32), ttship.Snac.from_gguf(it, g0, max_frames=32)
    try:
        assert np.array_equal(rg.orpheus_logits(a), rg.orpheus_logits(b))
        heads, z = rg.snac_inputs(8, sa.noise_per_frame)
        assert np.array_equal(sa.decode(heads, z), sb.decode(heads, z))
    finally:
        for r in (a, b, sa, sb):
            r.close()


# ---- files from the quantize tool ----
def _check_tool_output(src, out, arch, qtype, heads, quantized_names):
    """Types exactly where the rule puts them, quantized bytes those of the host quantizer, the rest untouched."""
    p = ttship.quantize_params(qtype, quantize_output_heads=int(heads))
    with ttship.Gguf(src) as a, ttship.Gguf(out) as b:
        assert b.get("general.quantization_type") == qtype and b.get("general.architecture") == arch
        assert [t[0] for t in a.tensors()] == [t[0] for t in b.tensors()]
        n = 0
        for (name, _, ne, _, _), (_, ty, ne2, _, _) in zip(a.tensors(), b.tensors()):
            assert ne == ne2, name
            assert ttship.gguf_tensor_rule(arch, name, p) == (1 if name in quantized_names else 0), name
            if name in quantized_names:
                n += 1
                assert ty == qtype, (name, ty)
                x = a.tensor_bytes(name).view(np.float32).reshape(-1, ne[0])
                want = x.astype(np.float16).view(np.uint8).reshape(-1) if qtype == F16 else rg.host_rows(qtype, x)
                assert np.array_equal(b.tensor_bytes(name), want), name
            else:  # norms, rope_frequencies, F32 heads, snac.* and audio_encoder.*
                assert ty == F32 and np.array_equal(b.tensor_bytes(name), a.tensor_bytes(name)), name
        assert n == len(quantized_names)


@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("qtype", [Q8_0, Q5_0, Q4_0, F16])
def test_dia_quantized_file(files, it, qtype, heads):
    out, _, twin = rg.quantized(files[0], qtype, heads)
    names = rg.dia_quantized_names(heads)
    assert len(names) == 10 + 9 * heads + 7 * rg.DIA["n_encoder_layers"] + 11 * rg.DIA["n_decoder_layers"]
    _check_tool_output(files[0], out, "dia", qtype, heads, names)
    ot = rg.oracle_type(qtype)
    with ttship.Gguf(out) as g:
        c = ttship.dia_config_from_gguf(g)
        assert (c.weight_type, c.head_type) == (qtype, qtype if heads else F32)
    with ttship.Gguf(twin) as t:
        assert {ty for n, ty, *_ in t.tensors() if n in names} == {ot}
        run = ttship.Dia.from_gguf(it, t, arena_bytes=rg.ARENA)
        ref = ttship.Dia(it, rg.dia_cfg(weight_type=ot, head_type=ot if heads else F32))
        try:
            _check_loaded_bytes(run, t, "dia.", rg.dia_name_map())
            rg.set_weights_from_file(ref, t, "dia.", rg.dia_name_map())
            got = rg.dia_logits(run)
            rg.bits_equal(rg.dia_logits(ref), got, "dia logits")
            assert got.std() > 0
            dac = ttship.Dac(it, ttship.dac_config_from_gguf(t, max_frames=16), gguf=t)  # the tool leaves audio_encoder.* alone
            dac.close()
        finally:
            run.close()
            ref.close()


@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("qtype", [Q4_K, Q4_0, Q8_0, Q5_0])
def test_orpheus_quantized_file(files, it, qtype, heads):
    out, _, twin = rg.quantized(files[1], qtype, heads)
    names = rg.orpheus_quantized_names(heads)
    assert len(names) == 1 + heads + 7 * rg.ORPHEUS["n_layers"]
    _check_tool_output(files[1], out, "orpheus", qtype, heads, names)
    ot = rg.oracle_type(qtype)
    kw = dict(max_ctx=rg.ORPHEUS["max_ctx"], arena_bytes=rg.ARENA)
    nm = rg.orpheus_name_map()
    with ttship.Gguf(twin) as t:
        assert ttship.orpheus_config_from_gguf(t, **kw).weight_type == ot
        assert t.tensor_type("orpheus.lm_head") == (ot if heads else F32) and t.tensor_type("orpheus.embed_tokens") == ot
        run = ttship.Orpheus.from_gguf(it, t, **kw)
        ref = ttship.Orpheus(it, rg.orpheus_cfg(weight_type=ot))  # every matrix, the embedding and the head of one type
        try:
            _check_loaded_bytes(run, t, "orpheus.", nm)
            # an F32 head fits no synthetic runner: ref keeps its own head and lends its final norm's output instead
            rg.set_weights_from_file(ref, t, "orpheus.", nm, skip=() if heads else ("output",))
            got, want = rg.orpheus_logits(run), rg.orpheus_logits(ref)
            if heads:
                rg.bits_equal(want, got, "orpheus logits")
            else:
                # the last decode step: the two runners' final norm outputs agree, and run's logits are the oracle's
                # MUL_MAT of the file's F32 head over them
                x = rg.last_hidden(ref)
                rg.bits_equal(x, rg.last_hidden(run), "final norm output")
                c = rg.ORPHEUS
                head = t.tensor_bytes("orpheus.lm_head")
                rg.bits_equal(rg.oracle_mul_mat(F32, head, c["hidden_size"], c["vocab_size"], x), got[-1], "F32 head logits")
                assert not np.array_equal(got[-1], want[-1])
            assert got.std() > 0
            snac = ttship.Snac.from_gguf(it, t, max_frames=32)  # the rule leaves snac.* alone: still F32, still loads
            snac.close()
        finally:
            run.close()
            ref.close()


def test_orpheus_rule_on_a_real_files_names():
    r = lambda name, **kw: ttship.gguf_tensor_rule("orpheus", name, ttship.quantize_params(Q4_K, **kw))  # noqa: E731
    assert r("orpheus.layers.3.self_attn.q_proj") == 1 and r("orpheus.layers.27.self_attn.o_proj") == 1
    assert r("orpheus.layers.3.mlp.gate_proj") == 1 and r("orpheus.layers.0.mlp.down_proj") == 1
    assert r("orpheus.embed_tokens") == 1
    assert r("orpheus.lm_head") == 0 and r("orpheus.lm_head", quantize_output_heads=1) == 1
    assert r("orpheus.norm") == 0 and r("orpheus.norm", quantize_output_heads=1) == 0
    assert r("orpheus.layers.3.input_layernorm") == 0 and r("orpheus.layers.3.post_attention_layernorm") == 0
    assert r("orpheus.rope_frequencies") == 0
    for name in ("snac.in.weight", "snac.layers.0.weight", "snac.quantizers.0.codebook.weight", "snac.layers.1.residual_unit.2.out_weight",
                 "snac.quantizers.1.out_proj.weight", "snac.alpha_out"):
        assert r(name) == 0 and r(name, quantize_output_heads=1) == 0, name
    # the ".weight" spellings keep their answers
    assert r("orpheus.layers.0.mlp.down_proj.weight") == 1 and r("orpheus.layers.0.input_norm.weight") == 0
    assert r("orpheus.lm_head.weight") == 0 and r("orpheus.lm_head.weight", quantize_output_heads=1) == 1


# ---- refusals: NULL (a RuntimeError in the binding), never an abort ----
def _refused(cls, it, path, capfd, needle, **kw):
    with ttship.Gguf(path) as g:
        with pytest.raises(RuntimeError):
            cls(it, kw.pop("cfg"), gguf=g)
    err = capfd.readouterr().err
    assert needle in err, err


def test_refusals(files, it, tmp_path, capfd):
    with ttship.Gguf(files[0]) as g:
        dcfg = ttship.dia_config_from_gguf(g, arena_bytes=rg.ARENA)
    with ttship.Gguf(files[1]) as g:
        ocfg = ttship.orpheus_config_from_gguf(g, max_ctx=48, arena_bytes=rg.ARENA)
        scfg = ttship.snac_config_from_gguf(g, max_frames=32)
    # one tensor removed
    p = rg.rebuilt(files[0], tmp_path / "d-missing.gguf", drop="dia.decoder.layers.1.cross_v_proj")
    _refused(ttship.Dia, it, p, capfd, "'dia.decoder.layers.1.cross_v_proj' is missing", cfg=dcfg)
    p = rg.rebuilt(files[1], tmp_path / "o-missing.gguf", drop="orpheus.rope_frequencies")
    _refused(ttship.Orpheus, it, p, capfd, "'orpheus.rope_frequencies' is missing", cfg=ocfg)
    _refused(ttship.Snac, it, rg.rebuilt(files[1], tmp_path / "s-missing.gguf", drop="snac.layers.2.noise_weight"), capfd,
             "'snac.layers.2.noise_weight' is missing", cfg=scfg)
    # a wrong dimension: the same bytes under a transposed shape
    E, D = rg.DIA["encoder_hidden_size"], rg.DIA["decoder_hidden_size"]
    p = rg.rebuilt(files[0], tmp_path / "d-shape.gguf", reshape={"dia.decoder.layers.0.cross_k_proj": (D, E)})
    _refused(ttship.Dia, it, p, capfd, "'dia.decoder.layers.0.cross_k_proj' has type 0 [128 64 1 1]", cfg=dcfg)
    H, F = rg.ORPHEUS["hidden_size"], rg.ORPHEUS["ffn_size"]
    p = rg.rebuilt(files[1], tmp_path / "o-shape.gguf", reshape={"orpheus.layers.1.mlp.down_proj": (H, F)})
    _refused(ttship.Orpheus, it, p, capfd, "'orpheus.layers.1.mlp.down_proj' has type 0 [256 512 1 1]", cfg=ocfg)
    p = rg.rebuilt(files[1], tmp_path / "s-shape.gguf", reshape={"snac.up.weight": (1, 64, 32)})
    _refused(ttship.Snac, it, p, capfd, "'snac.up.weight' has type 0 [1 64 32 1]", cfg=scfg)
    # a quantized norm, which the tool's Dia rule never writes; an F16 norm in an Orpheus file
    norm = py_oracle.quantize(Q8_0, np.ones((1, E), np.float32))
    p = rg.rebuilt(files[0], tmp_path / "d-norm.gguf", retype={"dia.encoder.layers.0.pre_sa_norm": (Q8_0, norm)})
    _refused(ttship.Dia, it, p, capfd, "'dia.encoder.layers.0.pre_sa_norm' has type 8", cfg=dcfg)
    p = rg.rebuilt(files[1], tmp_path / "o-norm.gguf", retype={"orpheus.norm": (F16, np.ones(H, np.float16))})
    _refused(ttship.Orpheus, it, p, capfd, "'orpheus.norm' has type 1", cfg=ocfg)
    # storage types the runners do not take: Q4_K in a Dia file, F16 matrices in an Orpheus file, F16 in SNAC
    k = py_oracle.quantize(Q4_K, np.zeros((rg.DIA["decoder_hidden_size"], 256), np.float32))
    p = rg.rebuilt(files[0], tmp_path / "d-q4k.gguf", retype={"dia.decoder.layers.0.wo": (Q4_K, k)})
    _refused(ttship.Dia, it, p, capfd, "'dia.decoder.layers.0.wo' has type 12", cfg=dcfg)
    p = rg.rebuilt(files[1], tmp_path / "o-f16.gguf", retype={"orpheus.layers.0.self_attn.q_proj": (F16, np.zeros(H * H, np.float16))})
    _refused(ttship.Orpheus, it, p, capfd, "'orpheus.layers.0.self_attn.q_proj' has type 1", cfg=ocfg)
    p = rg.rebuilt(files[1], tmp_path / "s-f16.gguf", retype={"snac.in.bias": (F16, np.zeros(32, np.float16))})
    _refused(ttship.Snac, it, p, capfd, "'snac.in.bias' has type 1", cfg=scfg)
    # another model's file
    par = tmp_path / "parler.gguf"
    ttship.write_parler_synthetic_gguf(par, ttship.parler_config(n_layers=1, hidden_size=64, n_attn_heads=2, ffn_size=64, prompt_vocab=8,
                                                                 max_positions=8, max_ctx=8, weight_type=F32))
    with ttship.Gguf(par) as g:
        with pytest.raises(RuntimeError):
            ttship.dia_config_from_gguf(g)
    _refused(ttship.Dia, it, par, capfd, "not a dia file", cfg=dcfg)
    _refused(ttship.Orpheus, it, files[0], capfd, "not an orpheus file", cfg=ocfg)
    _refused(ttship.Snac, it, files[0], capfd, "'snac.quantizers.0.codebook.weight' is missing", cfg=scfg)
    # and the files themselves still load after all that
    with ttship.Gguf(files[0]) as g:
        ttship.Dia(it, dcfg, gguf=g).close()


def test_writers_refuse_a_config_that_is_no_model(tmp_path):
    with pytest.raises(RuntimeError):
        ttship.write_orpheus_synthetic_gguf(tmp_path / "a.gguf", rg.orpheus_cfg(weight_type=F32, n_attn_heads=3))  # 3 * 64 != 256
    with pytest.raises(RuntimeError):
        ttship.write_orpheus_synthetic_gguf(tmp_path / "b.gguf", rg.orpheus_cfg(weight_type=F32), ttship.snac_config(n_heads=9, **rg.SNAC))
    assert not (tmp_path / "a.gguf").exists() and not (tmp_path / "b.gguf").exists()


def test_set_weight_refuses_a_wrong_size(it):
    o = ttship.Orpheus(it, rg.orpheus_cfg(weight_type=F32))
    try:
        n = len(o.weights_raw())
        with pytest.raises(RuntimeError):
            o.set_weight(2, np.zeros(rg.ORPHEUS["hidden_size"] - 1, np.float32))  # output_norm holds hidden_size values
        with pytest.raises(RuntimeError):
            o.set_weight(n, np.zeros(4, np.float32))
        o.set_weight(2, np.full(rg.ORPHEUS["hidden_size"], 2.0, np.float32))
        assert np.all(o.weights()["output_norm"] == 2.0)
    finally:
        o.close()
