// T5 voice-description encoder runner (Parler-TTS' conditional prompt): builds the node list of
// t5_runner::build_t5_graph (/root/reference/src/models/parler/t5/model.cpp:216-298) in its order and feeds
// it as t5_runner::set_inputs does (:300-320), over any tts_backend_iface.  On the HIP backend every
// layer's mul_mat(k, q) -> add(pos_bias) -> soft_max_ext -> mul_mat(kq, v) -> permute -> cont chain
// runs as one k_attn_bias launch (graph_exec.hip try_attn).  Token ids come from the caller (EOS
// included): tokenizers are out of scope.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tts_gguf.h"
#include "../../include/tts_runners.h"
#include "graph.h"
#include "weights.h"

using namespace tts;

struct t5_layer {
    tts_tensor *attn_norm, *q, *k, *v, *o, *mlp_norm, *wi_0, *wi_1, *wo;
};

struct tts_t5 {
    tts_t5_config cfg;
    tts_backend_iface be;
    weight_store w;  // the weights, declaration order
    tts_tensor *embd = nullptr, *rel_bias = nullptr, *out_norm = nullptr, *down_proj = nullptr, *down_proj_bias = nullptr;
    std::vector<t5_layer> layers;
    char * arena = nullptr;
    size_t arena_size = 0;
    tg::context gctx;
    tts_tensor * res = nullptr;
    tts_tensor *in_tokens = nullptr, *in_pos_bucket = nullptr, *in_mask = nullptr;
    int32_t last_nodes = 0;
};

extern "C" void tts_t5_default_config(tts_t5_config * c) {
    // t5_encoder defaults (t5/model.h:42-51: flan-t5-xl with Parler's down projection)
    c->n_layers = 24;
    c->hidden_size = 2048;
    c->n_attn_heads = 32;
    c->head_size = 64;
    c->ffn_size = 5120;
    c->relative_attn_buckets = 32;
    c->vocab_size = 32128;
    c->max_context_length = 512;
    c->output_size = 1536;
    c->has_down_proj = 1;
    c->weight_type = TTS_TYPE_F32;
    c->eos_token_id = 1;
    c->seed = 0x5EED;
    c->arena_bytes = 0;
    c->debug_no_reuse = 0;
    c->pad_ = 0;
}

// kind: 0 = matrix, 1 = norm weight (~1), 2 = bias (~0), 3 = embedding, 4 = relative attention bias (values
// that move the softmax); 1..3 only as F32, any other storage type is a matrix.  With a file attached it
// decides the storage type.
static tts_tensor * wnew(tts_t5 * p, int type, int64_t ne0, int64_t ne1, int kind, const std::string & name) {
    type = p->w.file_type(name, type);
    const weight_fill fill = kind == 4                         ? weight_fill::uniform(2.0f, 0.0f)
                             : type != TTS_TYPE_F32 || kind == 0 ? weight_fill::matrix(kind == 3 ? 0.25f : 0.05f)
                             : kind == 1                       ? weight_fill::uniform(0.1f, 1.0f)
                             : kind == 2                       ? weight_fill::uniform(0.02f, 0.0f)
                                                               : weight_fill::uniform(0.5f, 0.0f);
    return p->w.add(type, ne0, ne1, 1, name, fill, p->cfg.seed ^ p->w.index());
}

static void declare_weights(tts_t5 * p) {
    const auto & cf = p->cfg;
    p->w.prefix = "t5encoder.";  // t5/model.cpp:6-25
    const int64_t E = cf.hidden_size, A = (int64_t)cf.n_attn_heads * cf.head_size, F = cf.ffn_size;
    const int wt = cf.weight_type;
    p->embd = wnew(p, wt, E, cf.vocab_size, 3, "token_embd");
    p->rel_bias = wnew(p, TTS_TYPE_F32, cf.n_attn_heads, cf.relative_attn_buckets, 4, "enc.blk.0.attn_rel_b");
    p->layers.resize(cf.n_layers);
    for (int l = 0; l < cf.n_layers; ++l) {
        t5_layer & L = p->layers[l];
        const std::string pre = "enc.blk." + std::to_string(l);
        L.attn_norm = wnew(p, TTS_TYPE_F32, E, 1, 1, pre + ".attn_norm");
        L.q = wnew(p, wt, E, A, 0, pre + ".attn_q");
        L.k = wnew(p, wt, E, A, 0, pre + ".attn_k");
        L.v = wnew(p, wt, E, A, 0, pre + ".attn_v");
        L.o = wnew(p, wt, A, E, 0, pre + ".attn_o");
        L.mlp_norm = wnew(p, TTS_TYPE_F32, E, 1, 1, pre + ".ffn_norm");
        L.wi_0 = wnew(p, wt, E, F, 0, pre + ".ffn_up");    // the GELU branch
        L.wi_1 = wnew(p, wt, E, F, 0, pre + ".ffn_gate");
        L.wo = wnew(p, wt, F, E, 0, pre + ".ffn_down");
    }
    p->out_norm = wnew(p, TTS_TYPE_F32, E, 1, 1, "enc.final_layer_norm");
    if (cf.has_down_proj) {
        p->down_proj = wnew(p, wt, E, cf.output_size, 0, "down_proj");
        p->down_proj_bias = wnew(p, TTS_TYPE_F32, cf.output_size, 1, 2, "down_proj_bias");
    }
}

static tts_t5 * t5_create(const tts_backend_iface * be, const tts_t5_config * cfg, const tts_gguf * g) {
    if (!be || !cfg) return nullptr;
    const auto & cf = *cfg;
    if (cf.n_layers < 1 || cf.hidden_size < 1 || cf.n_attn_heads < 1 || cf.head_size < 1 || cf.ffn_size < 1 || cf.vocab_size < 1 ||
        cf.relative_attn_buckets < 4 || cf.max_context_length < 1 || (cf.has_down_proj && cf.output_size < 1) ||
        (cf.weight_type != TTS_TYPE_F32 && cf.weight_type != TTS_TYPE_F16)) {
        fprintf(stderr, "t5: unusable config\n");
        return nullptr;
    }
    auto * p = new tts_t5();
    p->cfg = cf;
    if (!cf.has_down_proj) p->cfg.output_size = cf.hidden_size;
    p->be = *be;
    p->w.attach(g);
    declare_weights(p);
    if (!p->w.upload(p->be)) {
        fprintf(stderr, "t5: weight allocation/upload failed\n");
        tts_t5_free(p);
        return nullptr;
    }
    // the worst-case graph (t5_runner::prepare_post_load): a few [width, ctx] activations and the
    // [ctx, ctx, heads] bias and score tensors
    const size_t T = (size_t)p->cfg.max_context_length;
    const size_t wide = (size_t)std::max(std::max(p->cfg.hidden_size, p->cfg.ffn_size), p->cfg.n_attn_heads * p->cfg.head_size);
    p->arena_size = cf.arena_bytes ? cf.arena_bytes : 4 * (12 * wide * T + 5 * T * T * (size_t)p->cfg.n_attn_heads) + (1u << 20);
    p->arena = (char *)p->be.alloc(p->be.ctx, p->arena_size);
    if (!p->arena) {
        tts_t5_free(p);
        return nullptr;
    }
    return p;
}

extern "C" tts_t5 * tts_t5_create(const tts_backend_iface * be, const tts_t5_config * cfg) { return t5_create(be, cfg, nullptr); }

extern "C" void tts_t5_free(tts_t5 * p) {
    if (!p) return;
    if (p->arena) p->be.free(p->be.ctx, p->arena);
    p->w.release(p->be);
    delete p;
}

// build_t5_graph for n tokens.  Every op joins the node list as the builder creates it, so the list is
// build_t5_graph's own sequence of calls (embedding, position bias, then the layers).
static tts_tensor * build_graph(tts_t5 * p, int64_t n) {
    const auto & cf = p->cfg;
    const int64_t hd = cf.head_size, H = cf.n_attn_heads;
    tg::context & c = p->gctx;
    c.reset();
    const auto E = [&c](tts_tensor * t) {
        tg::build_forward_expand(c, t);
        return t;
    };
    p->in_pos_bucket = tg::new_tensor_2d(c, TTS_TYPE_I32, n, n);
    tg::set_name(p->in_pos_bucket, "pos_bucket");
    tg::set_input(p->in_pos_bucket);
    p->in_tokens = tg::new_tensor_1d(c, TTS_TYPE_I32, n);
    tg::set_input(p->in_tokens);
    tts_tensor * inpL = E(tg::get_rows(c, p->embd, p->in_tokens));
    p->in_mask = tg::new_tensor_2d(c, TTS_TYPE_F32, n, n);  // build_t5_attn_mask
    tg::set_input(p->in_mask);
    // build_t5_pos_bias: [key, query, head]
    tts_tensor * pos_bias = E(tg::get_rows(c, p->rel_bias, E(tg::view_1d(c, p->in_pos_bucket, n * n, 0))));
    pos_bias = E(tg::view_3d(c, pos_bias, pos_bias->ne[0], n, n, 4 * (size_t)pos_bias->ne[0], 4 * (size_t)pos_bias->ne[0] * (size_t)n, 0));
    pos_bias = E(tg::cont(c, E(tg::permute(c, pos_bias, 2, 1, 0, 3))));
    tg::set_name(pos_bias, "pos_bias");
    tts_tensor * cur = inpL;
    const auto norm = [&](tts_tensor * x, tts_tensor * w) {  // build_t5_norm (t5/model.cpp:179-185)
        return E(tg::mul(c, E(tg::rms_norm(c, x, 0.000001f)), w));
    };
    for (auto & L : p->layers) {
        tts_tensor * residual = inpL;
        cur = norm(inpL, L.attn_norm);
        tts_tensor * Qcur = E(tg::mul_mat(c, L.q, cur));
        tts_tensor * Kcur = E(tg::mul_mat(c, L.k, cur));
        tts_tensor * Vcur = E(tg::mul_mat(c, L.v, cur));
        Qcur = E(tg::reshape_3d(c, Qcur, hd, H, n));
        Kcur = E(tg::reshape_3d(c, Kcur, hd, H, n));
        tts_tensor * q = E(tg::permute(c, Qcur, 0, 2, 1, 3));
        tts_tensor * k = E(tg::cont(c, E(tg::permute(c, Kcur, 0, 2, 1, 3))));
        tts_tensor * kq = E(tg::mul_mat(c, k, q));
        kq = E(tg::add(c, kq, pos_bias));
        kq = E(tg::soft_max_ext(c, kq, p->in_mask, 1.0f, 0.0f));
        tts_tensor * v = E(tg::cont_3d(c, E(tg::transpose(c, Vcur)), n, hd, H));
        tts_tensor * kqv = E(tg::mul_mat(c, kq, v));
        tts_tensor * attn_out = E(tg::cont_2d(c, E(tg::permute(c, kqv, 2, 0, 1, 3)), H * hd, n));
        attn_out = E(tg::mul_mat(c, L.o, attn_out));
        cur = E(tg::add(c, attn_out, residual));
        tts_tensor * residual_mlp = cur;
        cur = norm(cur, L.mlp_norm);
        tts_tensor * gate = E(tg::mul_mat(c, L.wi_1, cur));
        cur = E(tg::mul(c, E(tg::gelu(c, E(tg::mul_mat(c, L.wi_0, cur)))), gate));
        cur = E(tg::mul_mat(c, L.wo, cur));
        cur = E(tg::add(c, cur, residual_mlp));
        inpL = cur;
    }
    cur = norm(cur, p->out_norm);
    if (p->down_proj) cur = E(tg::mul_mat(c, p->down_proj, cur));
    if (p->down_proj_bias) cur = E(tg::add(c, cur, p->down_proj_bias));
    tg::set_name(cur, "t5_output");
    tg::set_output(cur);
    return cur;
}

// t5_runner::set_inputs' bucket of (key i, query ii), exactly as written there (t5/model.cpp:308-316): the
// logarithm's argument is an integer quotient and the maximum distance is the literal 128.
static int32_t t5_bucket(int i, int ii, int relative_attn_buckets) {
    const int n_buckets = relative_attn_buckets / 2;
    const int max_exact = n_buckets / 2;
    const float logarithmic_denominator = log(128.0 / max_exact);
    const int ab_rpos = abs(i - ii);
    const int rpos = i - ii;
    return (int32_t)((uint32_t)(rpos > 0 ? n_buckets : 0) +
                     (ab_rpos < max_exact ? ab_rpos
                                          : std::min((n_buckets - 1), (max_exact + (int)((log((ab_rpos / max_exact)) / logarithmic_denominator) * max_exact)))));
}

extern "C" int tts_t5_encode(tts_t5 * p, const int32_t * tokens, int32_t n, float * out) {
    if (!p || !tokens || n < 1 || n > p->cfg.max_context_length) return TTS_STATUS_BAD_ARG;
    for (int32_t i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= p->cfg.vocab_size) return TTS_STATUS_BAD_ARG;
    p->res = build_graph(p, n);
    if (!tg::alloc_graph(p->gctx, p->arena, p->arena_size, !p->cfg.debug_no_reuse)) {
        fprintf(stderr, "t5: compute arena too small (%zu needed)\n", p->gctx.arena_used);
        return TTS_STATUS_ALLOC_FAILED;
    }
    p->last_nodes = (int32_t)p->gctx.nodes.size();
    std::vector<int32_t> bucket((size_t)n * n);
    std::vector<float> mask((size_t)n * n, 0.0f);
    for (int i = 0; i < n; ++i)
        for (int ii = 0; ii < n; ++ii) bucket[(size_t)i * n + ii] = t5_bucket(i, ii, p->cfg.relative_attn_buckets);
    auto & be = p->be;
    int st = be.set(be.ctx, p->in_tokens->data, tokens, sizeof(int32_t) * (size_t)n);
    st |= be.set(be.ctx, p->in_pos_bucket->data, bucket.data(), bucket.size() * sizeof(int32_t));
    st |= be.set(be.ctx, p->in_mask->data, mask.data(), mask.size() * sizeof(float));
    if (st != 0) return TTS_STATUS_FAILED;
    st = be.compute(be.ctx, p->gctx.nodes.data(), (int)p->gctx.nodes.size());
    if (st == 0 && out) st = be.get(be.ctx, out, p->res->data, sizeof(float) * (size_t)n * (size_t)p->cfg.output_size);
    if (st == 0) st = be.synchronize(be.ctx);
    return st;
}

extern "C" int32_t tts_t5_output_size(const tts_t5 * p) { return p ? p->cfg.output_size : 0; }
extern "C" int32_t tts_t5_last_graph_nodes(const tts_t5 * p) { return p ? p->last_nodes : 0; }
extern "C" uint64_t tts_t5_weight_bytes(const tts_t5 * p) { return p ? p->w.wbytes : 0; }
extern "C" int32_t tts_t5_n_weights(const tts_t5 * p) { return p ? p->w.size() : 0; }
extern "C" uint64_t tts_t5_weight(tts_t5 * p, int32_t i, char * name, uint64_t name_cap, int64_t * ne, int32_t * type, void * dst, uint64_t cap) {
    const tts_tensor * t = p ? p->w.tensor(i) : nullptr;
    return t ? tg::weight_out(p->be, t, name, name_cap, ne, type, dst, cap) : 0;
}
extern "C" tts_tensor * const * tts_t5_graph(const tts_t5 * p, int32_t * n_nodes) { return tg::graph_out(p ? &p->gctx : nullptr, n_nodes); }

// Debug: a named node ("pos_bias", "t5_output": the last one of that name) or input ("pos_bucket") of the last graph.
extern "C" uint64_t tts_t5_get_node(tts_t5 * p, const char * name, void * dst, uint64_t cap) {
    if (!p || !name) return 0;
    const tts_tensor * hit = nullptr;
    for (auto * t : p->gctx.nodes)
        if (strcmp(t->name, name) == 0) hit = t;
    if (!hit && p->in_pos_bucket && strcmp(p->in_pos_bucket->name, name) == 0 && p->last_nodes) hit = p->in_pos_bucket;
    return hit ? tg::tensor_out(p->be, hit, dst, cap) : 0;
}

// Debug: node i of the last graph: op / type / ne; copies its bytes when contiguous (returns size).
extern "C" uint64_t tts_t5_node(tts_t5 * p, int32_t i, int32_t * op, int32_t * type, int64_t * ne, void * dst, uint64_t cap) {
    return p ? tg::node_out(p->be, p->gctx.nodes, i, op, type, ne, dst, cap) : 0;
}

// ---- GGUF (t5_encoder::prep_constants / assign_weight, t5/model.cpp:27-110) ----
extern "C" int tts_t5_config_from_gguf(const tts_gguf * g, tts_t5_config * c) {
    if (!g || !c) return TTS_STATUS_BAD_ARG;
    if (tts_gguf_find_key(g, "t5encoder.vocab_size") < 0) {
        fprintf(stderr, "gguf: key 't5encoder.vocab_size' must be specified\n");
        return TTS_STATUS_BAD_ARG;
    }
    gguf_first_u32(g, {"t5encoder.vocab_size"}, &c->vocab_size);
    gguf_first_u32(g, {"t5encoder.block_count"}, &c->n_layers);
    gguf_first_u32(g, {"t5encoder.embedding_length"}, &c->hidden_size);
    gguf_first_u32(g, {"t5encoder.attention.head_count"}, &c->n_attn_heads);
    gguf_first_u32(g, {"t5encoder.context_length"}, &c->max_context_length);
    gguf_first_u32(g, {"t5encoder.output_size"}, &c->output_size);
    gguf_first_u32(g, {"tokenizer.ggml.eos_token_id"}, &c->eos_token_id);
    // sizes and types the tensors themselves carry
    const int64_t ffn = gguf_tensor_dim(g, "t5encoder.enc.blk.0.ffn_up", 1);
    const int64_t attn = gguf_tensor_dim(g, "t5encoder.enc.blk.0.attn_q", 1);
    const int64_t buckets = gguf_tensor_dim(g, "t5encoder.enc.blk.0.attn_rel_b", 1);
    if (ffn < 0 || attn < 0 || buckets < 0) {
        fprintf(stderr, "gguf: t5encoder tensors missing\n");
        return TTS_STATUS_BAD_ARG;
    }
    c->ffn_size = (int32_t)ffn;
    if (c->n_attn_heads < 1 || attn % c->n_attn_heads) return TTS_STATUS_BAD_ARG;
    c->head_size = (int32_t)(attn / c->n_attn_heads);
    c->relative_attn_buckets = (int32_t)buckets;
    c->weight_type = tts_gguf_tensor_type(g, tts_gguf_find_tensor(g, "t5encoder.enc.blk.0.attn_q"));
    c->has_down_proj = tts_gguf_find_tensor(g, "t5encoder.down_proj") >= 0 ? 1 : 0;
    if (c->weight_type != TTS_TYPE_F32 && c->weight_type != TTS_TYPE_F16) {
        fprintf(stderr, "gguf: quantized t5encoder weights are not supported\n");
        return TTS_STATUS_UNSUPPORTED;
    }
    return TTS_STATUS_SUCCESS;
}

extern "C" tts_t5 * tts_t5_create_from_gguf(const tts_backend_iface * be, const tts_t5_config * cfg, const tts_gguf * g) {
    if (!be || !cfg || !g) return nullptr;
    return t5_create(be, cfg, g);
}

extern "C" int tts_t5_write_synthetic_gguf(const tts_t5_config * cfg, const char * path) {
    if (!cfg || !path) return TTS_STATUS_BAD_ARG;
    tts_t5 p;  // declarations only: no backend, no buffers
    p.cfg = *cfg;
    declare_weights(&p);
    tts_gguf_writer * w = tts_gguf_writer_new();
    const auto & c = *cfg;
    tts_gguf_set_str(w, "general.architecture", "t5encoder");
    tts_gguf_set_u32(w, "t5encoder.block_count", (uint32_t)c.n_layers);
    tts_gguf_set_u32(w, "t5encoder.embedding_length", (uint32_t)c.hidden_size);
    tts_gguf_set_u32(w, "t5encoder.attention.head_count", (uint32_t)c.n_attn_heads);
    tts_gguf_set_u32(w, "t5encoder.context_length", (uint32_t)c.max_context_length);
    tts_gguf_set_u32(w, "t5encoder.vocab_size", (uint32_t)c.vocab_size);
    if (c.has_down_proj) tts_gguf_set_u32(w, "t5encoder.output_size", (uint32_t)c.output_size);
    tts_gguf_set_u32(w, "tokenizer.ggml.eos_token_id", (uint32_t)c.eos_token_id);
    int st = p.w.write(w);
    if (st == TTS_STATUS_SUCCESS) st = tts_gguf_writer_write(w, path);
    tts_gguf_writer_free(w);
    return st;
}
