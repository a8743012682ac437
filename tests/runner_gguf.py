"""What tests/test_runner_gguf_cpu.py and tests/test_runner_gguf_gpu.py share: the tiny Dia + DAC and Orpheus + SNAC
files, the reference's tensor names and keys spelled out from its source (src/models/dia/model.cpp:3-251,
src/models/orpheus/model.cpp:11-120, src/decoder/snac_model.cpp:3-84, general_neural_audio_codec.cpp:36-127 and the
converters under py-gguf/tts_encoders), the quantize tool's host rows, and the files the CPU oracle can hold.

The oracle computes F32, F16, Q4_K and Q8_0.  A Q5_0 file equals its Q8_0 twin under it bit for bit, a Q4_0 file
does once the low two mantissa bits of every block's d are cleared (tests/q5_0_ref.py, tests/q4_0_ref.py): so the
oracle runs the twin of the (trimmed) file, and the HIP backend the (trimmed) file itself.
"""
import ctypes

import numpy as np

import py_oracle
import q4_0_ref as q4
import q5_0_ref as q5
import ttship
import weights_pin as wp

F32, F16, Q4_K, Q8_0, Q5_0, Q4_0 = ttship.F32, ttship.F16, ttship.Q4_K, ttship.Q8_0, ttship.Q5_0, ttship.Q4_0
TYPE_NAME = {F32: "f32", F16: "f16", Q4_K: "q4_k", Q8_0: "q8_0", Q5_0: "q5_0", Q4_0: "q4_0"}
ARENA = 64 << 20

DIA = dict(wp.DIA_TINY, arena_bytes=ARENA)
ORPHEUS = dict(wp.ORPHEUS_TINY, arena_bytes=ARENA)
SNAC = dict(wp.SNAC_TINY)
DAC = dict(wp.DAC_TINY)
DIA_HEADS, DIA_VOCAB, DIA_TEXT_VOCAB = 9, 1028, 256  # Dia-1.6B's own, which DIA_TINY keeps


def dia_cfg(**kw):
    return ttship.dia_config(**dict(DIA, **kw))


def orpheus_cfg(**kw):
    return ttship.orpheus_config(**dict(ORPHEUS, **kw))


# ---- the reference's names: runner name -> file name after the prefix, and the file's shapes ----
def dia_name_map():
    """{runner's tensor name: the file's name after "dia."} (assign_to_encoder_layer / assign_to_decoder_layer)."""
    m = {"encoder.embedding": "encoder.embedding", "encoder.norm": "encoder.norm", "decoder.norm": "decoder.norm"}
    for l in range(DIA["n_encoder_layers"]):
        for a, b in (("q", "q_proj"), ("k", "k_proj"), ("v", "v_proj"), ("o", "o_proj"), ("self_attn_norm", "pre_sa_norm"),
                     ("mlp_norm", "post_sa_norm"), ("gate", "gate"), ("up", "up"), ("out", "wo")):
            m[f"encoder.layers.{l}.{a}"] = f"encoder.layers.{l}.{b}"
    for l in range(DIA["n_decoder_layers"]):
        for a, b in (("self_attn_q", "self_q_proj"), ("self_attn_k", "self_k_proj"), ("self_attn_v", "self_v_proj"),
                     ("self_attn_o", "self_o_proj"), ("cross_attn_q", "cross_q_proj"), ("cross_attn_k", "cross_k_proj"),
                     ("cross_attn_v", "cross_v_proj"), ("cross_attn_o", "cross_o_proj"), ("self_attn_norm", "pre_sa_norm"),
                     ("cross_attn_norm", "pre_ca_norm"), ("mlp_norm", "pre_mlp_norm"), ("gate", "gate"), ("up", "up"), ("out", "wo")):
            m[f"decoder.layers.{l}.{a}"] = f"decoder.layers.{l}.{b}"
    for i in range(DIA_HEADS):
        m[f"decoder.embds.{i}"] = f"decoder.embeddings.{i}"
        m[f"decoder.heads.{i}"] = f"decoder.heads.{i}"
    return m


def dia_file_tensors():
    """{file tensor name: ggml ne} of the Dia half of a DIA_TINY file, as dia_gguf_encoder.py lays the tensors out."""
    c = DIA
    E, D, hd = c["encoder_hidden_size"], c["decoder_hidden_size"], c["head_size"]
    EA, DA = c["encoder_attn_heads"] * hd, c["decoder_attn_heads"] * hd
    DKV = DA // c["decoder_query_heads"]
    t = {"dia.encoder.embedding": (E, DIA_TEXT_VOCAB), "dia.encoder.norm": (E,), "dia.decoder.norm": (D,)}
    for l in range(c["n_encoder_layers"]):
        p = f"dia.encoder.layers.{l}."
        t.update({p + "pre_sa_norm": (E,), p + "post_sa_norm": (E,), p + "q_proj": (E, EA), p + "k_proj": (E, EA), p + "v_proj": (E, EA),
                  p + "o_proj": (EA, E), p + "gate": (E, c["encoder_ffn_size"]), p + "up": (E, c["encoder_ffn_size"]),
                  p + "wo": (c["encoder_ffn_size"], E)})
    for l in range(c["n_decoder_layers"]):
        p = f"dia.decoder.layers.{l}."
        t.update({p + "pre_sa_norm": (D,), p + "pre_ca_norm": (D,), p + "pre_mlp_norm": (D,), p + "self_q_proj": (D, DA),
                  p + "self_k_proj": (D, DKV), p + "self_v_proj": (D, DKV), p + "self_o_proj": (DA, D), p + "cross_q_proj": (D, DA),
                  p + "cross_k_proj": (E, DA), p + "cross_v_proj": (E, DA), p + "cross_o_proj": (DA, D),
                  p + "gate": (D, c["decoder_ffn_size"]), p + "up": (D, c["decoder_ffn_size"]), p + "wo": (c["decoder_ffn_size"], D)})
    for i in range(DIA_HEADS):
        t[f"dia.decoder.embeddings.{i}"] = (D, DIA_VOCAB)
        t[f"dia.decoder.heads.{i}"] = (D, DIA_VOCAB)
    return t


DIA_KEYS = ["general.architecture", "dia.attn_head_size", "dia.eos_token_id", "dia.bos_token_id", "dia.pad_token_id", "dia.max_delay",
            "dia.encoder.max_context_length", "dia.encoder.attn_heads", "dia.encoder.layers", "dia.decoder.hidden_size",
            "dia.decoder.layers", "dia.decoder.output_heads", "dia.decoder.attn_heads", "dia.decoder.query_heads",
            "dia.decoder.output_vocab_size", "dia.decoder.audio_vocab_size", "dia.decoder.max_generation_size",
            "audio.bos_token_id", "audio.eos_token_id", "dac.up_scaling_factor"] + \
           [f"dac.dac_layer_{k}_{i}" for i in range(4) for k in ("stride", "padding")]


def orpheus_name_map():
    """{runner's tensor name: the file's name after "orpheus."} (orpheus_model::assign_weight / assign_to_layer)."""
    m = {"token_embd": "embed_tokens", "output": "lm_head", "output_norm": "norm", "rope_frequencies": "rope_frequencies"}
    for l in range(ORPHEUS["n_layers"]):
        for a, b in (("q", "self_attn.q_proj"), ("k", "self_attn.k_proj"), ("v", "self_attn.v_proj"), ("o", "self_attn.o_proj"),
                     ("gate", "mlp.gate_proj"), ("up", "mlp.up_proj"), ("down", "mlp.down_proj"), ("input_norm", "input_layernorm"),
                     ("post_attention_norm", "post_attention_layernorm")):
            m[f"layers.{l}.{a}"] = f"layers.{l}.{b}"
    return m


def orpheus_file_tensors():
    c = ORPHEUS
    H, KV = c["hidden_size"], c["n_kv_attn_heads"] * c["head_size"]
    t = {"orpheus.embed_tokens": (H, c["vocab_size"]), "orpheus.lm_head": (H, c["vocab_size"]), "orpheus.norm": (H,),
         "orpheus.rope_frequencies": (c["head_size"] // 2,)}
    for l in range(c["n_layers"]):
        p = f"orpheus.layers.{l}."
        t.update({p + "input_layernorm": (H,), p + "post_attention_layernorm": (H,), p + "self_attn.q_proj": (H, H),
                  p + "self_attn.k_proj": (H, KV), p + "self_attn.v_proj": (H, KV), p + "self_attn.o_proj": (H, H),
                  p + "mlp.gate_proj": (H, c["ffn_size"]), p + "mlp.up_proj": (H, c["ffn_size"]), p + "mlp.down_proj": (c["ffn_size"], H)})
    return t


def snac_file_tensors():
    """The SNAC half: snac_model::assign_weight's names (in / up / final / alpha_out, layers.N.{alpha, weight, bias,
    noise_weight}, layers.N.residual_unit.R.{in,out}_{alpha,weight,bias}, quantizers.N.{codebook.weight, out_proj.*}).
    Shapes as the runner holds them: a bias or an alpha [1, C] (the converter writes [C]; the loader takes either)."""
    c = dict(n_heads=3, codebook_dim=8, n_layers=4, **SNAC)
    lat, ch = c["latent_dim"], c["decoder_dim"]
    t = {}
    for i in range(c["n_heads"]):
        p = f"snac.quantizers.{i}."
        t.update({p + "codebook.weight": (c["codebook_dim"], c["codebook_size"]), p + "out_proj.weight": (1, c["codebook_dim"], lat),
                  p + "out_proj.bias": (1, lat)})
    t.update({"snac.in.weight": (7, 1, lat), "snac.in.bias": (1, lat), "snac.up.weight": (1, lat, ch), "snac.up.bias": (1, ch)})
    for l in range(c["n_layers"]):
        s, oc = c["rates"][l], ch // 2
        p = f"snac.layers.{l}."
        t.update({p + "alpha": (1, ch), p + "weight": (2 * s, oc, ch), p + "bias": (1, oc), p + "noise_weight": (1, oc, oc)})
        for r in range(3):
            q = p + f"residual_unit.{r}."
            t.update({q + "in_alpha": (1, oc), q + "in_weight": (7, 1, oc), q + "in_bias": (1, oc), q + "out_alpha": (1, oc),
                      q + "out_weight": (1, oc, oc), q + "out_bias": (1, oc)})
        ch = oc
    t.update({"snac.alpha_out": (1, ch), "snac.final.weight": (7, ch), "snac.final.bias": (1,)})
    return t


ORPHEUS_KEYS = ["general.architecture", "orpheus.stopping_token_id", "orpheus.hidden_size", "orpheus.vocab_size", "orpheus.attn_heads",
                "orpheus.kv_attn_heads", "orpheus.head_dim", "orpheus.layers", "orpheus.kv_hidden_size", "snac.audio_token_channels"] + \
               [f"snac.snac_layer_{k}_{i}" for i in range(4) for k in ("stride", "padding", "grouping")]


def dia_quantized_names(heads):
    """The tensors the tool's Dia rule quantizes (quantize_impl.cpp:42-49): everything under dia.* whose name does not
    end in "norm", the nine heads only with quantize_output_heads."""
    return {n for n in dia_file_tensors() if not n.endswith("norm") and (heads or not n.startswith("dia.decoder.heads"))}


def orpheus_quantized_names(heads):
    return {n for n in orpheus_file_tensors() if n.endswith("_proj") or n == "orpheus.embed_tokens" or (heads and n == "orpheus.lm_head")}


# ---- files ----
def host_rows(ty, x):
    """The quantize tool's rows on the host: the oracle's quantizers, numpy's for the types it has none for."""
    if ty in (Q4_K, Q8_0):
        return py_oracle.quantize(ty, x)
    return {Q5_0: q5.quantize_row_q5_0, Q4_0: q4.quantize_row_q4_0}[ty](x)


def write_f32(directory):
    """(dia + dac file, orpheus + snac file), F32, and the configs they were written from."""
    dia, orph = directory / "dia-f32.gguf", directory / "orpheus-f32.gguf"
    ttship.write_dia_synthetic_gguf(dia, dia_cfg(weight_type=F32, head_type=F32), ttship.dac_config(**DAC))
    ttship.write_orpheus_synthetic_gguf(orph, orpheus_cfg(weight_type=F32), ttship.snac_config(**SNAC))
    return dia, orph


def quantized(src, qtype, heads, backend=None):
    """src through the quantize tool -> (the file, the file the HIP backend runs, the file the oracle runs)."""
    stem = f"{src.name[:-len('-f32.gguf')]}-{TYPE_NAME[qtype]}{'-heads' if heads else ''}{'-dev' if backend else ''}"
    out = src.with_name(stem + ".gguf")
    if not out.exists():
        p = ttship.quantize_params(qtype, quantize_output_heads=int(heads))
        ttship.quantize_gguf(src, out, p, **(dict(backend=backend) if backend else dict(rows_fn=host_rows)))
    if qtype == Q5_0:
        run, twin = out, src.with_name(stem + "-twin.gguf")
        if not twin.exists():
            q5.twin_gguf(run, twin)
    elif qtype == Q4_0:
        run, twin = src.with_name(stem + "-trim.gguf"), src.with_name(stem + "-trim-twin.gguf")
        if not twin.exists():
            q4.trim_gguf(out, run)
            q4.twin_gguf(run, twin)
    else:
        run = twin = out
    return out, run, twin


def oracle_type(qtype):
    return Q8_0 if qtype in (Q5_0, Q4_0) else qtype


def rebuilt(src, dst, *, reverse=False, drop=None, retype=None, reshape=None, extra=False):
    """src rewritten with GgufWriter: tensors reversed, one dropped, one given another type ({name: (type, bytes)}) or
    shape ({name: ne}), an unrelated tensor and a string-array key added."""
    w = ttship.GgufWriter()
    keep = []
    with ttship.Gguf(src) as g:
        w.copy_kv(g)
        if extra:
            w.set("tokenizer.ggml.tokens", ["<s>", "hello", "</s>"])
            keep.append(np.arange(24, dtype=np.float32))
            w.add_tensor("unrelated.table", F32, (6, 4), keep[-1])
        ts = g.tensors()
        for name, ty, ne, _, _ in (reversed(ts) if reverse else ts):
            if name == drop:
                continue
            data = g.tensor_bytes(name)
            if retype and name in retype:
                ty, data = retype[name]
            if reshape and name in reshape:
                ne = reshape[name]
            keep.append(np.ascontiguousarray(data))
            w.add_tensor(name, ty, ne, keep[-1])
        w.write(dst)
    w.close()
    return dst


# ---- running ----
DIA_TEXT = np.frombuffer(b"\x01 hi.", dtype=np.uint8).astype(np.int32)  # 5 real tokens in the 32-token context


def dia_audio(step):
    return ((np.arange(DIA_HEADS, dtype=np.int32) * 97 + 131 * step + 5) % DIA_VOCAB).astype(np.int32)


def dia_logits(r, steps=3):
    """Prefill with 5 real tokens, then `steps` decode steps: [1 + steps][heads][vocab]."""
    out = [r.prefill(DIA_TEXT, dia_audio(0))]
    for s in range(steps):
        out.append(r.decode(dia_audio(s + 1)))
    return np.stack(out)


def orpheus_tokens(batch, n, step=0):
    v = ORPHEUS["vocab_size"]
    return ((np.arange(batch * n, dtype=np.int32).reshape(batch, n) * 37 + 211 * step + 3) % v).astype(np.int32)


def orpheus_logits(r, batch=1, steps=3):
    """Prefill of 5 tokens, then `steps` decode steps: [1 + steps][batch][vocab]."""
    out = [r.prefill(orpheus_tokens(batch, 5))]
    for s in range(steps):
        out.append(r.decode(orpheus_tokens(batch, 1, s + 1).reshape(batch)))
    return np.stack(out)


def snac_inputs(T, noise_per_frame, codebook=64):
    rng = np.random.default_rng(T)
    heads = [rng.integers(0, codebook, T // r).astype(np.int32) for r in (4, 2, 1)]
    return heads, rng.standard_normal(noise_per_frame * T).astype(np.float32)


def dac_codes(T):
    return np.random.default_rng(T).integers(0, 1024, size=(T, DIA_HEADS))


def bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.all(np.isfinite(b)), what
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


def set_weights_from_file(runner, g, prefix, name_map, skip=()):
    """The file's bytes into a synthetic runner, weight by weight through the name map; every weight must have the type
    and size the runner declared (tts_<runner>_set_weight refuses another size)."""
    for i, (name, (ty, _, _)) in enumerate(runner.weights_raw().items()):
        if name in skip:
            continue
        fname = prefix + name_map[name]
        assert g.tensor_type(fname) == ty, (fname, g.tensor_type(fname), ty)
        runner.set_weight(i, g.tensor_bytes(fname))


def last_hidden(runner):
    """The final norm's output of an Orpheus decode step on the oracle (host memory): the activation the head
    multiplies, read from the step graph's second-last node."""
    n = ctypes.c_int32()
    nodes = ctypes.cast(runner.L.tts_orpheus_graph(runner.ptr, ctypes.byref(n)), ctypes.POINTER(ctypes.POINTER(ttship.TtsTensor)))
    head, x = nodes[n.value - 1].contents, nodes[n.value - 2].contents
    assert ttship.OPS[head.op] == "MUL_MAT" and ttship.OPS[x.op] == "MUL" and x.type == F32, (ttship.OPS[head.op], ttship.OPS[x.op])
    cnt = x.ne[0] * x.ne[1] * x.ne[2] * x.ne[3]
    return np.ctypeslib.as_array(ctypes.cast(x.data, ctypes.POINTER(ctypes.c_float)), shape=(cnt,)).copy().reshape(-1, x.ne[0])


def oracle_mul_mat(wtype, w_bytes, K, N, x):
    """The oracle's MUL_MAT node over a weight's bytes and activations x [M][K] -> [M][N]."""
    import nodes
    g = nodes.Graph()
    w = g.leaf(raw=w_bytes, typ=wtype, ne=[K, N])
    a = g.leaf(x)
    y = g.node("MUL_MAT", F32, [N, x.shape[0]], (w, a))
    g.run_oracle(4)
    return g.node_array(y, shape=(x.shape[0], N))
