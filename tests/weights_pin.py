"""The weight-bytes pin shared by tests/golden/gen_weights_pin.py and tests/test_weights_pin_*.py.

Every runner configuration below is created on a backend and each of its weights is read back through
the exported tts_<runner>_weight (ctypes, not ttship.runner_weights, which skips quantized tensors):
name, ggml type, ne[4] and the sha256 of the bytes.  tests/golden/weights_pin.json.gz holds those entries
as the runners produced them before the shared weight store existed; it is never regenerated.
"""
import ctypes
import gzip
import hashlib
import json
import pathlib

import ttship

FIXTURE = pathlib.Path(__file__).resolve().parent / "golden" / "weights_pin.json.gz"  # 3595 digests: gzip keeps it small

PARLER_Q4K = dict(n_layers=2, hidden_size=256, n_attn_heads=4, ffn_size=512, max_ctx=64, prompt_vocab=512, max_positions=96)
T5_TINY = dict(n_layers=2, hidden_size=128, n_attn_heads=2, head_size=64, ffn_size=256, vocab_size=96, max_context_length=160,
               output_size=96, has_down_proj=1, weight_type=ttship.F32)
T5_TINY_F16 = dict(T5_TINY, n_attn_heads=4, has_down_proj=0, weight_type=ttship.F16)
ORPHEUS_TINY = dict(n_layers=2, hidden_size=256, n_attn_heads=4, n_kv_attn_heads=2, head_size=64, ffn_size=512, vocab_size=1000, max_ctx=48)
DIA_TINY = dict(n_encoder_layers=1, n_decoder_layers=2, encoder_hidden_size=64, decoder_hidden_size=128, encoder_attn_heads=4,
                decoder_attn_heads=4, decoder_query_heads=2, head_size=32, encoder_ffn_size=128, decoder_ffn_size=256,
                max_generation_size=64, max_encoder_context_length=32)
DAC_TINY = dict(latent_dim=64, decoder_dim=64, rates=[2, 2, 2, 2], n_layers=4, max_frames=16)
SNAC_TINY = dict(latent_dim=32, decoder_dim=64, codebook_size=64, rates=[2, 2, 4, 2], max_frames=32)
KOKORO_GEN_TINY = dict(in_channels=32, style_dim=16, max_frames=16)
KOKORO_TINY = dict(gen=dict(in_channels=32, style_dim=16), hidden=64, n_heads=4, ffn=128, embd=32, d_model=32, dec_dim=64, asr_res_dim=8,
                   max_tokens=16, max_total=96, n_recurrence=3, n_voice_rows=20)
SMALL_ARENA = 16 << 20  # no graph runs here

# runner -> (class, config maker, exported prefix, whether tts_<prefix>_weight reports the type)
RUNNERS = {
    "parler": (ttship.Parler, ttship.parler_config, "tts_parler", True),
    "t5": (ttship.T5, ttship.t5_config, "tts_t5", True),
    "orpheus": (ttship.Orpheus, ttship.orpheus_config, "tts_orpheus", True),
    "dia": (ttship.Dia, ttship.dia_config, "tts_dia", True),
    "dac": (ttship.Dac, ttship.dac_config, "tts_dac", True),
    "snac": (ttship.Snac, ttship.snac_config, "tts_snac", False),
    "kokoro_gen": (ttship.KokoroGenerator, ttship.kokoro_gen_config, "tts_kokoro_gen", False),
    "kokoro": (ttship.Kokoro, ttship.kokoro_config, "tts_kokoro", False),
}

# configuration id -> (runner, config keywords); every one is sized like the tiny ones of tests/test_*_cpu.py
CONFIGS = {
    "parler_q4k": ("parler", dict(PARLER_Q4K, weight_type=ttship.Q4_K, head_type=ttship.F32)),
    "parler_f32": ("parler", dict(PARLER_Q4K, weight_type=ttship.F32, head_type=ttship.F32)),
    "parler_q4k_seed": ("parler", dict(PARLER_Q4K, weight_type=ttship.Q4_K, head_type=ttship.F32, seed=0xC0FFEE123)),
    "t5_f32": ("t5", T5_TINY),
    "t5_f16": ("t5", T5_TINY_F16),
    "orpheus_default": ("orpheus", ORPHEUS_TINY),
    "orpheus_f32": ("orpheus", dict(ORPHEUS_TINY, weight_type=ttship.F32)),
    "dia_default": ("dia", DIA_TINY),
    "dia_f32": ("dia", dict(DIA_TINY, weight_type=ttship.F32)),
    "dac": ("dac", DAC_TINY),
    "snac": ("snac", SNAC_TINY),
    "kokoro_gen_f32": ("kokoro_gen", dict(KOKORO_GEN_TINY, weight_type=ttship.F32)),
    "kokoro_gen_f16": ("kokoro_gen", dict(KOKORO_GEN_TINY, weight_type=ttship.F16)),
    "kokoro_f32": ("kokoro", dict(KOKORO_TINY, weight_type=ttship.F32)),
    "kokoro_f16": ("kokoro", dict(KOKORO_TINY, weight_type=ttship.F16)),
    "kokoro_f32_seed": ("kokoro", dict(KOKORO_TINY, weight_type=ttship.F32, seed=0xABCDEF0123)),
}
# every tensor F32 or F16: the HIP backend stores those as ggml does, so they read back byte for byte
GPU_CONFIGS = ["t5_f32", "t5_f16", "dac", "snac", "kokoro_gen_f32"]

# synthetic file id -> (writer, runner configs it is written from)
FILES = {
    "parler_q4k_dac.gguf": lambda path: ttship.write_parler_synthetic_gguf(path, make_config("parler_q4k"), make_config("dac")),
    "t5_f32.gguf": lambda path: ttship.write_t5_synthetic_gguf(path, make_config("t5_f32")),
}


def make_config(cid):
    runner, kw = CONFIGS[cid]
    kw = dict(kw)
    if "arena_bytes" in dict(RUNNERS[runner][1]()._fields_):
        kw.setdefault("arena_bytes", SMALL_ARENA)
    return RUNNERS[runner][1](**kw)


def weight_digests(runner, obj):
    """[[name, type, [ne0..ne3], sha256 of the bytes tts_<runner>_weight returns]] in declaration order."""
    _, _, prefix, typed = RUNNERS[runner]
    n_fn, w_fn = getattr(obj.L, prefix + "_n_weights"), getattr(obj.L, prefix + "_weight")
    out = []
    for i in range(n_fn(obj.ptr)):
        name = ctypes.create_string_buffer(128)
        ne = (ctypes.c_int64 * 4)()
        ty = ctypes.c_int32(ttship.F32)  # the untyped getters return f32 values
        head = (obj.ptr, i, name, 128, ne) + ((ctypes.byref(ty),) if typed else ())
        n = w_fn(*head, None, 0)
        assert n > 0, (runner, i)
        buf = ctypes.create_string_buffer(n)
        assert w_fn(*head, ctypes.cast(buf, ctypes.c_void_p), n) == n, (runner, i)
        out.append([name.value.decode(), int(ty.value), [int(v) for v in ne], hashlib.sha256(buf.raw).hexdigest()])
    return out


def config_digests(cid, iface):
    runner = CONFIGS[cid][0]
    obj = RUNNERS[runner][0](iface, make_config(cid))
    try:
        return weight_digests(runner, obj)
    finally:
        obj.close()


def file_digest(fid, directory):
    path = pathlib.Path(directory) / fid
    FILES[fid](path)
    return hashlib.sha256(path.read_bytes()).hexdigest()


def load_fixture():
    return json.loads(gzip.decompress(FIXTURE.read_bytes()))


def save_fixture(obj):
    """Same bytes for the same content: no file name or time in the gzip header."""
    FIXTURE.write_bytes(gzip.compress((json.dumps(obj, separators=(",", ":")) + "\n").encode(), 9, mtime=0))


def first_difference(cid, got, want):
    """None, or a message naming the first weight of configuration cid that differs from the fixture."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"{cid}: weight {i} '{w[0]}' differs: got {g}, pinned {w}"
    if len(got) != len(want):
        return f"{cid}: {len(got)} weights, the fixture pins {len(want)}"
    return None
