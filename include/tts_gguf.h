/* GGUF model files: reader (mmap), writer, the quantize tool and the runners' loader path.
 *
 * The reference loads every model through ggml's gguf API: runner_from_file mmaps the file and points
 * each tensor's data into the mapping (src/models/loaders.cpp:34-95), reads the architecture and the
 * model constants from the KV section (e.g. parler_tts_model::prep_constants,
 * src/models/parler/model.cpp:51-108) and hands every named tensor to the runner's assign_weight
 * (parler/model.cpp:263-307, dac_model.cpp:58-98, general_neural_audio_codec.cpp:36-127).  The
 * quantize example rewrites an F32 file per-architecture (examples/quantize/quantize_impl.cpp:14-292).
 * These entry points are that path for this backend: the runners take their weights from a GGUF file
 * instead of the synthetic generator, uploaded whole-tensor so the HIP backend keeps its own layouts.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "tts_hip.h"
#include "tts_runners.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gguf_type (value types of the KV section) */
enum tts_gguf_type {
    TTS_GGUF_UINT8 = 0,
    TTS_GGUF_INT8 = 1,
    TTS_GGUF_UINT16 = 2,
    TTS_GGUF_INT16 = 3,
    TTS_GGUF_UINT32 = 4,
    TTS_GGUF_INT32 = 5,
    TTS_GGUF_FLOAT32 = 6,
    TTS_GGUF_BOOL = 7,
    TTS_GGUF_STRING = 8,
    TTS_GGUF_ARRAY = 9,
    TTS_GGUF_UINT64 = 10,
    TTS_GGUF_INT64 = 11,
    TTS_GGUF_FLOAT64 = 12,
};

/* ---- reader (gguf_init_from_file with no_alloc + llama_mmap) ---- */
typedef struct tts_gguf tts_gguf;

/* NULL on a missing / malformed file (the reason goes to stderr). */
tts_gguf * tts_gguf_open(const char * path);
void tts_gguf_close(tts_gguf * g);
uint32_t tts_gguf_version(const tts_gguf * g);
uint64_t tts_gguf_alignment(const tts_gguf * g);
uint64_t tts_gguf_data_offset(const tts_gguf * g); /* gguf_get_data_offset */

int64_t tts_gguf_n_kv(const tts_gguf * g);
int64_t tts_gguf_find_key(const tts_gguf * g, const char * key); /* -1 if absent */
const char * tts_gguf_key(const tts_gguf * g, int64_t i);
int32_t tts_gguf_kv_type(const tts_gguf * g, int64_t i);
/* scalar value of any numeric / bool type converted to the requested C type; 0 on a type mismatch */
int tts_gguf_get_u32(const tts_gguf * g, int64_t i, uint32_t * out);
int tts_gguf_get_i64(const tts_gguf * g, int64_t i, int64_t * out);
int tts_gguf_get_f64(const tts_gguf * g, int64_t i, double * out);
const char * tts_gguf_get_str(const tts_gguf * g, int64_t i); /* NULL unless a string */
int32_t tts_gguf_arr_type(const tts_gguf * g, int64_t i);      /* -1 unless an array */
int64_t tts_gguf_arr_n(const tts_gguf * g, int64_t i);
const void * tts_gguf_arr_data(const tts_gguf * g, int64_t i); /* numeric arrays: packed elements */
const char * tts_gguf_arr_str(const tts_gguf * g, int64_t i, int64_t j);

int64_t tts_gguf_n_tensors(const tts_gguf * g);
int64_t tts_gguf_find_tensor(const tts_gguf * g, const char * name); /* -1 if absent */
const char * tts_gguf_tensor_name(const tts_gguf * g, int64_t i);
int32_t tts_gguf_tensor_type(const tts_gguf * g, int64_t i); /* ggml_type numbering (= TTS_TYPE_*) */
int32_t tts_gguf_tensor_ndims(const tts_gguf * g, int64_t i, int64_t * ne4);
uint64_t tts_gguf_tensor_offset(const tts_gguf * g, int64_t i); /* relative to the data section */
uint64_t tts_gguf_tensor_size(const tts_gguf * g, int64_t i);
const void * tts_gguf_tensor_data(const tts_gguf * g, int64_t i); /* into the mapping */
/* bytes of one block / elements per block of a ggml_type (0 if unknown) */
size_t tts_gguf_type_size(int32_t type);
int64_t tts_gguf_blck_size(int32_t type);

/* ---- writer (gguf_init_empty / gguf_set_* / gguf_add_tensor / gguf_write_to_file) ---- */
typedef struct tts_gguf_writer tts_gguf_writer;

tts_gguf_writer * tts_gguf_writer_new(void);
void tts_gguf_writer_free(tts_gguf_writer * w);
/* setting an existing key replaces its value (gguf_set_val_*) */
void tts_gguf_set_u32(tts_gguf_writer * w, const char * key, uint32_t v);
void tts_gguf_set_i32(tts_gguf_writer * w, const char * key, int32_t v);
void tts_gguf_set_f32(tts_gguf_writer * w, const char * key, float v);
void tts_gguf_set_u64(tts_gguf_writer * w, const char * key, uint64_t v);
void tts_gguf_set_bool(tts_gguf_writer * w, const char * key, int v);
void tts_gguf_set_str(tts_gguf_writer * w, const char * key, const char * v);
void tts_gguf_set_arr(tts_gguf_writer * w, const char * key, int32_t elem_type, const void * data, int64_t n);
void tts_gguf_set_arr_str(tts_gguf_writer * w, const char * key, const char * const * v, int64_t n);
/* gguf_set_kv: every KV pair of a file */
void tts_gguf_copy_kv(tts_gguf_writer * w, const tts_gguf * src);
/* The data is copied; nbytes must equal the type's row size x rows.  0 on success. */
int tts_gguf_add_tensor(tts_gguf_writer * w, const char * name, int32_t type, int32_t n_dims, const int64_t * ne,
                        const void * data, uint64_t nbytes);
int tts_gguf_writer_write(const tts_gguf_writer * w, const char * path); /* 0 on success */

/* ---- quantize tool (examples/quantize/quantize_impl.cpp) ---- */
typedef struct tts_quantize_params {
    int32_t quantize_type;                  /* TTS_TYPE_Q4_K, TTS_TYPE_Q6_K, TTS_TYPE_Q8_0, TTS_TYPE_Q5_0, TTS_TYPE_Q4_0 or TTS_TYPE_F16 */
    int32_t quantize_output_heads;          /* quantization_params fields, same meaning */
    int32_t quantize_text_embeddings;
    int32_t quantize_cross_attn_kv;
    int32_t convert_dac_to_f16;
    int32_t convert_non_quantizable_to_f16;
    int32_t mix;                            /* 0 = every quantized tensor in quantize_type; TTS_QUANT_MIX_* */
} tts_quantize_params;

/* llama.cpp's Q4_K_M recipe: quantize_type must be TTS_TYPE_Q4_K (Parler and Orpheus files only).  Of the tensors the
 * rule quantizes these take Q6_K instead, where more_bits(N, n) = N < n/8 || N >= 7*n/8 || (N - n/8) % 3 == 2 over the
 * n layers of the file (integer division):
 *   Orpheus: orpheus.layers.N.self_attn.v_proj and .mlp.down_proj when more_bits(N, n); orpheus.lm_head;
 *   Parler : ...layers.N.self_attn.v_proj.weight, ...layers.N.fc2.weight and ...layers.N.encoder_attn.v_proj.weight
 *            when more_bits(N, n); the *.weight.head tensors. */
#define TTS_QUANT_MIX_Q4_K_M 1

/* Rows of x [rows][K] f32 (host memory) -> type's blocks in dst (host memory); 0 on success. */
typedef int (*tts_quantize_rows_fn)(void * ctx, int32_t type, const float * x, void * dst, int64_t rows, int64_t K);

/* quantize_impl.cpp:14-80 (parler / dia / kokoro; orpheus, where the reference aborts: the projections
 * orpheus.layers.N.{self_attn,mlp}.*_proj and orpheus.embed_tokens, orpheus.lm_head with quantize_output_heads,
 * never a norm, orpheus.rope_frequencies or a snac.* tensor): 1 = quantize, 2 = convert to F16, 0 = copy unchanged. */
int tts_gguf_tensor_rule(const char * arch, const char * name, const tts_quantize_params * params);
/* The storage type the tool gives tensor `name` of an F32 file of n_layers layers: quantize_type (or TTS_TYPE_Q6_K
 * where params->mix moves it) for rule 1, TTS_TYPE_F16 for rule 2 and for rule 1 under quantize_type F16,
 * TTS_TYPE_F32 for a tensor copied unchanged.  Negative: an unknown architecture, or parameters the tool refuses
 * (TTS_STATUS_BAD_ARG: a mix with another quantize_type than Q4_K, a mix for a Dia or Kokoro file, Q6_K for Kokoro). */
int32_t tts_gguf_tensor_out_type(const char * arch, const char * name, int32_t n_layers, const tts_quantize_params * params);
/* quantize_gguf: KV pairs copied + general.quantization_version / general.quantization_type, every
 * tensor in file order, quantized rows from `fn`, F16 by round-to-nearest-even.  0 on success. */
int tts_gguf_quantize(const char * in_path, const char * out_path, const tts_quantize_params * params,
                      tts_quantize_rows_fn fn, void * fn_ctx);
/* The same with the device quantizers (tts_hip_quantize, k_quant.hip). */
int tts_hip_gguf_quantize(tts_hip_backend_t be, const char * in_path, const char * out_path, const tts_quantize_params * params);

/* ---- loader path (runner_from_file -> assign_weight) ---- */
/* parler_tts_model::prep_constants + tensor types: fills the model fields of cfg from the file
 * (n_layers, hidden_size, heads, vocabularies, n_encode, weight / head types); batch, max_ctx, seed
 * and arena stay as given.  0 on success. */
int tts_parler_config_from_gguf(const tts_gguf * g, tts_parler_config * cfg);
/* A Parler runner whose weights are the file's "decoder.*" tensors (parler/model.cpp:501-505);
 * NULL (with the reason on stderr) on a missing tensor or a shape / type the runner cannot take. */
tts_parler * tts_parler_create_from_gguf(const tts_backend_iface * be, const tts_parler_config * cfg, const tts_gguf * g);
/* Writes the runner's synthetic weights (the ones tts_parler_create uploads for cfg) as a GGUF file
 * with the reference's tensor names and keys, plus a DAC-44k decoder ("audio_encoder.*", dac.* keys)
 * for dac_cfg when not NULL -- the F32 input of the quantize tool in the tests. */
int tts_parler_write_synthetic_gguf(const tts_parler_config * cfg, const tts_dac_config * dac_cfg, const char * path);

/* t5_encoder::prep_constants (t5encoder.* keys; t5encoder.vocab_size is required) + what the tensors carry:
 * ffn_size from enc.blk.0.ffn_up, head_size from attn_q, has_down_proj from t5encoder.down_proj's presence,
 * weight_type from attn_q (F32 / F16).  seed and arena stay as given.  0 on success. */
int tts_t5_config_from_gguf(const tts_gguf * g, tts_t5_config * cfg);
/* A T5 encoder runner whose weights are the file's "t5encoder.*" tensors. */
tts_t5 * tts_t5_create_from_gguf(const tts_backend_iface * be, const tts_t5_config * cfg, const tts_gguf * g);
/* Writes the synthetic weights tts_t5_create uploads for cfg with the reference's tensor names and keys. */
int tts_t5_write_synthetic_gguf(const tts_t5_config * cfg, const char * path);

/* dac_model::prep_constants / prep_layers: codebooks, strides from the dac.* keys.  0 on success. */
int tts_dac_config_from_gguf(const tts_gguf * g, tts_dac_config * cfg);
/* A DAC decoder whose weights are the file's "audio_encoder.*" tensors (F32). */
tts_dac * tts_dac_create_from_gguf(const tts_backend_iface * be, const tts_dac_config * cfg, const tts_gguf * g);

/* ---- Dia (dia_model::prep_constants / assign_weight, src/models/dia/model.cpp:3-251) ---- */
/* general.architecture must be "dia".  The dia.* keys prep_constants reads (layers, heads, head size, vocabulary,
 * context and generation lengths, dia.cfg_scale when present); the widths no key carries from the tensors: encoder
 * hidden size and vocabulary from dia.encoder.embedding, FFN sizes from the gate tensors, decoder hidden size from
 * dia.decoder.embeddings.0; weight_type from dia.decoder.layers.0.self_q_proj, head_type from dia.decoder.heads.0.
 * seed and arena stay as given.  0 on success. */
int tts_dia_config_from_gguf(const tts_gguf * g, tts_dia_config * cfg);
/* A Dia runner whose weights are the file's "dia.*" tensors, each in the type the file gives it: F32, F16, Q8_0,
 * Q5_0 or Q4_0 for the matrices, embeddings and heads (what the quantize tool's Dia rule can produce), F32 for the
 * norms.  NULL (the tensor's name and the reason on stderr) on a missing tensor, a shape that disagrees with cfg,
 * another type, or a quantized norm. */
tts_dia * tts_dia_create_from_gguf(const tts_backend_iface * be, const tts_dia_config * cfg, const tts_gguf * g);
/* Writes the runner's synthetic weights (the ones tts_dia_create uploads for cfg) under the reference's tensor
 * names and keys, plus the DAC decoder ("audio_encoder.*", dac.* keys) for dac_cfg when not NULL: the file
 * tts_dac_create_from_gguf loads its other half from. */
int tts_dia_write_synthetic_gguf(const tts_dia_config * cfg, const tts_dac_config * dac_cfg, const char * path);

/* ---- Orpheus (orpheus_model::prep_constants / assign_weight, src/models/orpheus/model.cpp:11-120) ---- */
/* general.architecture must be "orpheus".  orpheus.{vocab_size,attn_heads,kv_attn_heads,head_dim,hidden_size,layers};
 * ffn_size from orpheus.layers.0.mlp.gate_proj, weight_type from orpheus.layers.0.self_attn.q_proj.  batch, max_ctx,
 * seed, the arena and the rope fields stay as given (the loader does not use the rope fields).  0 on success. */
int tts_orpheus_config_from_gguf(const tts_gguf * g, tts_orpheus_config * cfg);
/* An Orpheus runner whose weights are the file's "orpheus.*" tensors (names as the converter writes them, without
 * ".weight").  The embedding, the head and every matrix take the type the file gives that tensor: F32, Q4_K, Q8_0,
 * Q5_0 or Q4_0 (a file quantized without quantize_output_heads has an F32 lm_head beside quantized matrices); norms
 * and orpheus.rope_frequencies, which is read from the file and not recomputed, are F32.  NULL on failure, as above. */
tts_orpheus * tts_orpheus_create_from_gguf(const tts_backend_iface * be, const tts_orpheus_config * cfg, const tts_gguf * g);
/* Writes the synthetic model under those names and keys, plus the SNAC decoder ("snac.*") for snac_cfg when not NULL. */
int tts_orpheus_write_synthetic_gguf(const tts_orpheus_config * cfg, const tts_snac_config * snac_cfg, const char * path);

/* ---- SNAC (snac_model::prep_constants / prep_layers / assign_weight, src/decoder/snac_model.cpp:3-84) ---- */
/* snac.audio_token_channels, snac.snac_layer_stride_{i} (padding and grouping, when present, must be what the
 * decoder assumes); codebook size and dimension, latent and decoder widths from the tensor shapes.  repeats,
 * max_frames, seed and the arena stay as given.  0 on success. */
int tts_snac_config_from_gguf(const tts_gguf * g, tts_snac_config * cfg);
/* A SNAC decoder whose weights are the file's "snac.*" tensors (F32 only). */
tts_snac * tts_snac_create_from_gguf(const tts_backend_iface * be, const tts_snac_config * cfg, const tts_gguf * g);

/* ---- Kokoro (kokoro_model::prep_constants / assign_weight, src/models/kokoro/model.cpp:413-930) ---- */
/* Writes the F32 synthetic model (what tts_kokoro_create fills for cfg with weight_type F32), the input of the
 * quantize tool: general.architecture = "kokoro", the kokoro.* keys prep_constants and the generator's
 * *_from_file builders read, the reference's tensor names under "kokoro.", one voice pack
 * "kokoro.voice_tensors.synthetic".  Constants post_load_assign builds (LSTM initial hidden / state, sqrt_tensor,
 * the window and sampling constants) are not in the file.  0 on success. */
int tts_kokoro_write_synthetic_gguf(const tts_kokoro_config * cfg, const char * path);
/* The model fields of cfg from the keys, the widths from the tensor shapes; max_tokens, max_total, seed and the
 * arena stay as given.  0 on success. */
int tts_kokoro_config_from_gguf(const tts_gguf * g, tts_kokoro_config * cfg);
/* A Kokoro runner over the file's tensors, each in the type the file gives it: F32 anywhere, F16 where the
 * quantize tool converts to F16, Q8_0 / Q5_0 / Q4_0 where its Kokoro rule quantizes; any other type, or a quantized
 * tensor the rule would not quantize, fails with the tensor's name on stderr.  voice names the
 * "kokoro.voice_tensors.<voice>" pack (NULL: the file's first); a missing voice fails.  NULL on failure. */
tts_kokoro * tts_kokoro_create_from_gguf(const tts_backend_iface * be, const tts_kokoro_config * cfg, const tts_gguf * g, const char * voice);

#ifdef __cplusplus
}
#endif
