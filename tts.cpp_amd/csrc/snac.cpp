// SNAC (Scale Neural Audio Codec, 24 kHz) decoder runner -- Orpheus' vocoder: three codebook
// streams at 1/4, 1/2 and 1x the latent frame rate -> PCM.  The node list of
// snac_runner::build_snac_graph (/root/reference/src/decoder/snac_model.cpp:130-159) with
// snac_build_audio_inputs (:86-109: per-head codebook lookup + 1x1 projection, repeat_interleave
// of the coarse heads through ggml_repeat), the depthwise input conv (ggml_conv_1d_dw, :141) and
// general_neural_audio_codec::build_layer / build_residual_unit / build_quantize_layer
// (general_neural_audio_codec.cpp:133-172) with the noise branch (conv_1d k = 1, MUL by the noise
// row, ADD) and grouped (depthwise) residual units.  The reference draws the noise on the host
// (random_normal_gen in snac_runner::set_inputs, :178); here the caller passes it in.
// Weights are deterministic synthetic tensors in SNAC-24kHz shapes (hubertsiuzdak/snac_24khz as
// Orpheus uses it: codebook 4096 x 8, latent 768, decoder 1024, rates 8,8,4,2, vq strides 4,2,1).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "graph.h"
#include "weights.h"
#include "tts_hip.h"
#include "tts_runners.h"

using namespace tts;

namespace {

struct snac_ru {  // residual unit (general_neural_audio_codec.h:29-41), grouped: depthwise conv
    tts_tensor *in_alpha, *in_kernel, *in_bias, *out_alpha, *out_kernel, *out_bias;
    int padding, dilation;
};

struct snac_layer {  // decoder block (general_neural_audio_codec.h:43-58) with its noise kernel
    tts_tensor *in_alpha, *kernel, *bias, *noise_kernel;
    int stride, padding;
    snac_ru ru[3];
};

struct snac_quant {  // residual_vector_quantize_layer
    tts_tensor *codebook, *out_kernel, *out_bias;
};

}  // namespace

struct tts_snac {
    tts_snac_config cfg;
    tts_backend_iface be;
    weight_store w;  // the weights, declaration order
    std::vector<snac_quant> quant;
    tts_tensor *in_kernel = nullptr, *in_bias = nullptr, *up_kernel = nullptr, *up_bias = nullptr;
    tts_tensor *out_alpha = nullptr, *out_kernel = nullptr, *out_bias = nullptr;
    tts_tensor * one = nullptr;  // the scalar 1.0 of reciprocal() (a device tensor, not a host static)
    std::vector<snac_layer> layers;
    char * arena = nullptr;
    size_t arena_size = 0;
    tg::context gctx;
    tts_tensor *in_codes = nullptr, *in_noise = nullptr;
};

extern "C" void tts_snac_default_config(tts_snac_config * c) {
    memset(c, 0, sizeof(*c));
    c->n_heads = 3;
    c->codebook_size = 4096;
    c->codebook_dim = 8;
    c->latent_dim = 768;
    c->decoder_dim = 1024;
    c->n_layers = 4;
    const int rates[4] = {8, 8, 4, 2};
    for (int i = 0; i < 4; ++i) c->rates[i] = rates[i];
    const int reps[3] = {4, 2, 1};
    for (int i = 0; i < 3; ++i) c->repeats[i] = reps[i];
    c->max_frames = 2048;
    c->seed = 0x5AAC5EEDull;
    c->arena_bytes = 0;
}

// in_file = false: a constant the runner builds itself, never in a GGUF file
static tts_tensor * wnew(tts_snac * d, float scale, float offset, int64_t ne0, int64_t ne1, int64_t ne2, const std::string & name,
                         bool in_file = true) {
    return d->w.add(TTS_TYPE_F32, ne0, ne1, ne2, name, weight_fill::uniform(scale, offset), d->cfg.seed ^ d->w.index(), in_file);
}

// conv kernel [K, IC, OC], uniform +-gain*sqrt(3/fan_in)
static tts_tensor * conv_w(tts_snac * d, int K, int IC, int OC, const std::string & name, float gain = 1.0f) {
    return wnew(d, gain * std::sqrt(3.0f / (float)(K * IC)), 0.f, K, IC, OC, name);
}

static int64_t snac_hop(const tts_snac_config & c) {
    int64_t hop = 1;
    for (int l = 0; l < c.n_layers; ++l) hop *= c.rates[l];
    return hop;
}

// Declares every weight tensor under the reference's names (snac_model::assign_weight, snac_model.cpp:51-84;
// general_neural_audio_codec.cpp:36-127); the synthetic seeds follow this order.  No backend needed.
static void declare_weights(tts_snac * d) {
    const auto & c = d->cfg;
    d->w.prefix = "snac.";
    for (int i = 0; i < c.n_heads; ++i) {
        snac_quant q;
        const std::string pre = "quantizers." + std::to_string(i);
        q.codebook = wnew(d, 1.0f, 0.f, c.codebook_dim, c.codebook_size, 1, pre + ".codebook.weight");
        q.out_kernel = conv_w(d, 1, c.codebook_dim, c.latent_dim, pre + ".out_proj.weight");
        q.out_bias = wnew(d, 0.01f, 0.f, 1, c.latent_dim, 1, pre + ".out_proj.bias");
        d->quant.push_back(q);
    }
    // depthwise input conv (kernel [7, 1, latent]) and the 1x1 up projection (snac_model.cpp:141-144)
    d->in_kernel = wnew(d, std::sqrt(3.0f / 7.0f), 0.f, 7, 1, c.latent_dim, "in.weight");
    d->in_bias = wnew(d, 0.01f, 0.f, 1, c.latent_dim, 1, "in.bias");
    d->up_kernel = conv_w(d, 1, c.latent_dim, c.decoder_dim, "up.weight");
    d->up_bias = wnew(d, 0.01f, 0.f, 1, c.decoder_dim, 1, "up.bias");
    int ch = c.decoder_dim;
    for (int l = 0; l < c.n_layers; ++l) {
        const int s = c.rates[l], oc = ch / 2;
        snac_layer L;
        const std::string pre = "layers." + std::to_string(l);
        L.stride = s;
        L.padding = (s + 1) / 2;  // SNAC DecoderBlock: ceil(stride / 2), output_padding stride % 2 = 0
        L.in_alpha = wnew(d, 0.5f, 1.0f, 1, ch, 1, pre + ".alpha");
        L.kernel = wnew(d, std::sqrt(3.0f / (float)(2 * ch)), 0.f, 2 * s, oc, ch, pre + ".weight");
        L.bias = wnew(d, 0.01f, 0.f, 1, oc, 1, pre + ".bias");
        L.noise_kernel = conv_w(d, 1, oc, oc, pre + ".noise_weight", 0.3f);
        for (int r = 0; r < 3; ++r) {
            snac_ru & u = L.ru[r];
            const std::string rp = pre + ".residual_unit." + std::to_string(r);
            u.dilation = (int)std::pow(3, r);
            u.padding = 3 * u.dilation;  // pow(3, r + 1) (general_neural_audio_codec.h:46)
            u.in_alpha = wnew(d, 0.5f, 1.0f, 1, oc, 1, rp + ".in_alpha");
            u.in_kernel = wnew(d, 0.5f * std::sqrt(3.0f / 7.0f), 0.f, 7, 1, oc, rp + ".in_weight");  // groups = channels
            u.in_bias = wnew(d, 0.01f, 0.f, 1, oc, 1, rp + ".in_bias");
            u.out_alpha = wnew(d, 0.5f, 1.0f, 1, oc, 1, rp + ".out_alpha");
            u.out_kernel = conv_w(d, 1, oc, oc, rp + ".out_weight", 0.5f);
            u.out_bias = wnew(d, 0.01f, 0.f, 1, oc, 1, rp + ".out_bias");
        }
        d->layers.push_back(L);
        ch = oc;
    }
    d->out_alpha = wnew(d, 0.5f, 1.0f, 1, ch, 1, "alpha_out");
    d->out_kernel = conv_w(d, 7, ch, 1, "final.weight", 0.1f);
    d->out_bias = wnew(d, 0.01f, 0.f, 1, 1, 1, "final.bias");
    d->one = wnew(d, 0.f, 1.0f, 1, 1, 1, "one", false);
}

static bool config_ok(const tts_snac_config * cfg) {
    return cfg && cfg->n_heads >= 1 && cfg->n_heads <= 4 && cfg->n_layers >= 1 && cfg->n_layers <= 8;
}

static tts_snac * snac_create(const tts_backend_iface * be, const tts_snac_config * cfg, const tts_gguf * g) {
    if (!be || !config_ok(cfg)) return nullptr;
    auto * d = new tts_snac();
    d->cfg = *cfg;
    d->be = *be;
    d->w.attach(g);
    const auto & c = d->cfg;
    declare_weights(d);
    if (!d->w.upload(d->be)) {
        tts_snac_free(d);
        return nullptr;
    }
    // arena: the widest activations are the last blocks' [T*hop, C] tensors plus their F16 im2cols
    const int64_t hop = snac_hop(c);
    const size_t last = (size_t)c.max_frames * (size_t)hop * (size_t)(c.decoder_dim >> c.n_layers) * 4;
    d->arena_size = c.arena_bytes ? c.arena_bytes : last * 24 + ((size_t)64 << 20);
    d->arena = (char *)d->be.alloc(d->be.ctx, d->arena_size);
    if (!d->arena) {
        tts_snac_free(d);
        return nullptr;
    }
    return d;
}

extern "C" tts_snac * tts_snac_create(const tts_backend_iface * be, const tts_snac_config * cfg) { return snac_create(be, cfg, nullptr); }

extern "C" void tts_snac_free(tts_snac * d) {
    if (!d) return;
    if (d->arena) d->be.free(d->be.ctx, d->arena);
    d->w.release(d->be);
    delete d;
}

extern "C" int64_t tts_snac_hop(const tts_snac * d) { return snac_hop(d->cfg); }

extern "C" int64_t tts_snac_noise_per_frame(const tts_snac * d) {
    // noise_steps (snac_model.h:19): the cumulative upsampling after each block, 8 + 64 + 256 + 512
    int64_t n = 0, up = 1;
    for (int l = 0; l < d->cfg.n_layers; ++l) n += (up *= d->cfg.rates[l]);
    return n;
}

// snake_1d (util.cpp:98-101): x + sin(alpha*x)^2 * (1/alpha), reciprocal() as DIV of a broadcast 1.0
static tts_tensor * snake(tts_snac * d, tg::context & c, tts_tensor * alpha, tts_tensor * x) {
    tts_tensor * one = tg::view_2d(c, d->one, 1, alpha->ne[1], 0, 0);
    tts_tensor * recip = tg::div(c, one, alpha);
    return tg::add(c, x, tg::mul(c, tg::sqr(c, tg::sin(c, tg::mul(c, x, alpha))), recip));
}

static tts_tensor * build_graph(tts_snac * d, int64_t T) {
    const auto & cf = d->cfg;
    tg::context & c = d->gctx;
    c.reset();
    // snac_build_audio_inputs (snac_model.cpp:86-109): head i holds T / repeats[i] codes, stored
    // back to back in one I32 input
    int64_t ncodes = 0;
    for (int i = 0; i < cf.n_heads; ++i) ncodes += T / cf.repeats[i];
    d->in_codes = tg::new_tensor_1d(c, TTS_TYPE_I32, ncodes);
    tg::set_input(d->in_codes);
    tts_tensor * embd = nullptr;
    size_t stride = 0;
    for (int i = 0; i < cf.n_heads; ++i) {
        const int64_t Ti = T / cf.repeats[i];
        tts_tensor * head = tg::cont(c, tg::view_1d(c, d->in_codes, Ti, stride));
        stride += (size_t)Ti * 4;
        // build_quantize_layer (general_neural_audio_codec.cpp:166-172)
        tts_tensor * code = tg::get_rows(c, d->quant[i].codebook, head);
        code = tg::cont(c, tg::transpose(c, code));
        code = tg::conv_1d(c, d->quant[i].out_kernel, code, 1, 0, 1);
        code = tg::add(c, code, d->quant[i].out_bias);
        if (cf.repeats[i] > 1) {
            // repeat_interleave along time through ggml_repeat (snac_model.cpp:97-101)
            tts_tensor * shape = tg::new_tensor_3d(c, TTS_TYPE_F32, cf.repeats[i], code->ne[0], cf.latent_dim);
            code = tg::repeat(c, tg::cont_3d(c, code, 1, code->ne[0], code->ne[1]), shape);
            code = tg::cont_2d(c, code, T, code->ne[2]);
        }
        embd = i == 0 ? code : tg::add(c, embd, code);
    }
    d->in_noise = tg::new_tensor_1d(c, TTS_TYPE_F32, tts_snac_noise_per_frame(d) * T);
    tg::set_input(d->in_noise);
    tg::set_name(embd, "embd");
    tts_tensor * cur = tg::conv_1d_dw(c, d->in_kernel, embd, 1, 3, 1);
    cur = tg::add(c, cur, d->in_bias);
    tg::set_name(cur, "in_conv");
    cur = tg::conv_1d(c, d->up_kernel, cur, 1, 0, 1);
    cur = tg::add(c, cur, d->up_bias);
    tg::set_name(cur, "up");
    int li = 0;
    size_t noise_off = 0;
    int64_t up = 1;
    for (auto & L : d->layers) {
        up *= L.stride;
        tts_tensor * noise = tg::cont(c, tg::view_1d(c, d->in_noise, up * T, noise_off));
        noise_off += (size_t)(up * T) * 4;
        // general_neural_audio_codec::build_layer (general_neural_audio_codec.cpp:151-164)
        cur = snake(d, c, L.in_alpha, cur);
        cur = tg::conv_transpose_1d(c, L.kernel, cur, L.stride, L.padding, 1, 0, 1);
        cur = tg::add(c, cur, L.bias);
        tg::set_name(cur, "convt." + std::to_string(li));
        tts_tensor * x = tg::conv_1d(c, L.noise_kernel, cur, 1, 0, 1);
        x = tg::mul(c, x, noise);
        cur = tg::add(c, cur, x);
        tg::set_name(cur, "noise." + std::to_string(li));
        int ri = 0;
        for (auto & u : L.ru) {
            // build_residual_unit (general_neural_audio_codec.cpp:133-149), groups > 1
            tts_tensor * residual = cur;
            cur = snake(d, c, u.in_alpha, cur);
            cur = tg::conv_1d_dw(c, u.in_kernel, cur, 1, u.padding, u.dilation);
            cur = tg::add(c, cur, u.in_bias);
            cur = snake(d, c, u.out_alpha, cur);
            cur = tg::conv_1d(c, u.out_kernel, cur, 1, 0, 1);
            cur = tg::add(c, cur, u.out_bias);
            cur = tg::add(c, cur, residual);
            tg::set_name(cur, "ru." + std::to_string(li) + "." + std::to_string(ri++));
        }
        ++li;
    }
    cur = snake(d, c, d->out_alpha, cur);
    cur = tg::conv_1d(c, d->out_kernel, cur, 1, 3, 1);
    cur = tg::add(c, cur, d->out_bias);
    cur = tg::tanh(c, cur);
    tg::set_name(cur, "pcm");
    tg::set_output(cur);
    tg::build_forward_expand(c, cur);
    return cur;
}

extern "C" int tts_snac_decode(tts_snac * d, const int32_t * codes, int32_t T, const float * noise, float * pcm) {
    if (!d || !codes || !noise || T <= 0 || T > d->cfg.max_frames) return TTS_STATUS_BAD_ARG;
    for (int i = 0; i < d->cfg.n_heads; ++i)
        if (T % d->cfg.repeats[i]) return TTS_STATUS_BAD_ARG;  // every head covers whole frames
    tts_tensor * out = build_graph(d, T);
    if (!tg::alloc_graph(d->gctx, d->arena, d->arena_size, !d->cfg.debug_no_reuse)) {
        fprintf(stderr, "snac: compute arena too small (%zu needed)\n", d->gctx.arena_used);
        return TTS_STATUS_ALLOC_FAILED;
    }
    int st = d->be.set(d->be.ctx, d->in_codes->data, codes, tg::nbytes(d->in_codes));
    if (st == 0) st = d->be.set(d->be.ctx, d->in_noise->data, noise, tg::nbytes(d->in_noise));
    if (st == 0) st = d->be.compute(d->be.ctx, d->gctx.nodes.data(), (int)d->gctx.nodes.size());
    if (st == 0 && pcm) st = d->be.get(d->be.ctx, pcm, out->data, sizeof(float) * (size_t)tg::nelements(out));
    return st;
}

extern "C" int32_t tts_snac_last_graph_nodes(const tts_snac * d) { return (int32_t)d->gctx.nodes.size(); }

extern "C" int32_t tts_snac_n_weights(const tts_snac * d) { return d ? d->w.size() : 0; }

extern "C" uint64_t tts_snac_weight(tts_snac * d, int32_t i, char * name, uint64_t name_cap, int64_t * ne, float * dst, uint64_t cap) {
    const tts_tensor * t = d ? d->w.tensor(i) : nullptr;
    return t ? tg::weight_out(d->be, t, name, name_cap, ne, nullptr, dst, cap) : 0;
}

// Debug: copy the named node of the last graph to host (contiguous nodes only); returns bytes.
extern "C" uint64_t tts_snac_get_node(tts_snac * d, const char * name, void * dst, uint64_t cap) {
    return d && name ? tg::named_node_out(d->be, d->gctx.nodes, name, dst, cap) : 0;
}

// ---- GGUF loader path (snac_model::prep_constants / prep_layers / assign_weight, snac_model.cpp:3-84) ----
extern "C" int tts_snac_config_from_gguf(const tts_gguf * g, tts_snac_config * c) {
    if (!g || !c) return TTS_STATUS_BAD_ARG;
    gguf_first_u32(g, {"snac.audio_token_channels"}, &c->n_heads);
    int n_layers = 0;
    for (int l = 0; l < 8; ++l) {  // prep_layers: stride, padding and grouping per block
        const std::string n = std::to_string(l);
        int32_t s = 0, pd = 0, gr = 0;
        if (!gguf_first_u32(g, {("snac.snac_layer_stride_" + n).c_str()}, &s)) break;
        // the reference requires the other two keys; when present they must be what the runner computes
        if (gguf_first_u32(g, {("snac.snac_layer_padding_" + n).c_str()}, &pd) && (uint32_t)pd != ((uint32_t)s + 1) / 2) {
            fprintf(stderr, "gguf: SNAC block %d padding %u, the decoder assumes ceil(stride / 2)\n", l, (uint32_t)pd);
            return TTS_STATUS_UNSUPPORTED;
        }
        const int64_t oc = gguf_tensor_dim(g, "snac.layers." + n + ".residual_unit.0.in_weight", 2);
        if (gguf_first_u32(g, {("snac.snac_layer_grouping_" + n).c_str()}, &gr) && oc >= 0 && gr != oc) {
            fprintf(stderr, "gguf: SNAC block %d grouping %u, the decoder's residual units are depthwise (%lld)\n", l, (uint32_t)gr, (long long)oc);
            return TTS_STATUS_UNSUPPORTED;
        }
        c->rates[l] = s;
        n_layers = l + 1;
    }
    if (n_layers == 0) {
        fprintf(stderr, "gguf: key snac.snac_layer_stride_0 must be specified for the SNAC decoder\n");
        return TTS_STATUS_BAD_ARG;
    }
    c->n_layers = n_layers;
    const char * cbw = "snac.quantizers.0.codebook.weight";
    const int64_t cd = gguf_tensor_dim(g, cbw, 0), cs = gguf_tensor_dim(g, cbw, 1);
    const int64_t lat = gguf_tensor_dim(g, "snac.up.weight", 1), dd = gguf_tensor_dim(g, "snac.up.weight", 2);
    if (cd < 0 || cs < 0 || lat < 0 || dd < 0) {
        fprintf(stderr, "gguf: SNAC tensors missing\n");
        return TTS_STATUS_BAD_ARG;
    }
    c->codebook_dim = (int32_t)cd;
    c->codebook_size = (int32_t)cs;
    c->latent_dim = (int32_t)lat;
    c->decoder_dim = (int32_t)dd;
    return config_ok(c) ? TTS_STATUS_SUCCESS : TTS_STATUS_BAD_ARG;
}

extern "C" tts_snac * tts_snac_create_from_gguf(const tts_backend_iface * be, const tts_snac_config * cfg, const tts_gguf * g) {
    if (!g) return nullptr;
    return snac_create(be, cfg, g);
}

namespace tts {
// The synthetic SNAC decoder as "snac.*" tensors + snac.* keys (orpheus_gguf_encoder.py:213-221).
int snac_write_synthetic(const tts_snac_config * cfg, tts_gguf_writer * w) {
    if (!config_ok(cfg)) return TTS_STATUS_BAD_ARG;
    tts_snac d;  // declarations only
    d.cfg = *cfg;
    declare_weights(&d);
    tts_gguf_set_u32(w, "snac.audio_token_channels", (uint32_t)cfg->n_heads);
    int ch = cfg->decoder_dim;
    for (int l = 0; l < cfg->n_layers; ++l) {
        ch /= 2;
        const std::string n = std::to_string(l);
        tts_gguf_set_u32(w, ("snac.snac_layer_stride_" + n).c_str(), (uint32_t)cfg->rates[l]);
        tts_gguf_set_u32(w, ("snac.snac_layer_padding_" + n).c_str(), (uint32_t)((cfg->rates[l] + 1) / 2));
        tts_gguf_set_u32(w, ("snac.snac_layer_grouping_" + n).c_str(), (uint32_t)ch);
    }
    return d.w.write(w);
}
}  // namespace tts
