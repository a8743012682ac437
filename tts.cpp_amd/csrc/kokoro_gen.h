// Internal: the Kokoro generator builder shared by the standalone generator runner (kokoro.cpp)
// and the full Kokoro runner (kokoro_model.cpp), which builds it into its own graph the way
// kokoro_runner::build_kokoro_graph calls build_generator (src/models/kokoro/model.cpp:1237).
#pragma once

#include <cstring>
#include <string>

#include "graph.h"
#include "weights.h"
#include "tts_gguf.h"
#include "tts_runners.h"

struct tts_kokoro_gen;

namespace tts {

// build_sin_gen + build_generator into c: x [C, T] (channel fastest), f0 [T] or [T, 1], style
// [style_dim]; returns the PCM node [300 T] and registers the generator's host inputs on k.
// device_draws: the uv_noise map draws its uniforms on the device (counter hash) instead of
// reading host draws; kokoro_gen_set_inputs must then be given rand = NULL.
tts_tensor * kokoro_gen_build(tts_kokoro_gen * k, tg::context & c, tts_tensor * x, tts_tensor * f0, tts_tensor * style, int64_t T,
                              bool device_draws);
// After tg::alloc_graph: fill and upload those inputs (uv_noise data block, window envelope);
// rand = [harmonic_num + 1][300 T] uniform draws, or NULL for a graph built with device_draws.
int kokoro_gen_set_inputs(tts_kokoro_gen * k, int64_t T, const float * rand);

// Which GGUF tensors an F16 Kokoro file holds as F16: kokoro_is_f16_compatible
// (/root/reference/examples/quantize/quantize_impl.cpp:14-18; `quantize -qt F16 -nqf` converts every
// such tensor, the quantizable ALBERT / LSTM / duration ones included).  Only matrices and conv
// kernels (>= 2-D) are converted here: the 1-D f16-compatible tensors of the real file (LSTM initial
// states) are zeros either way, and constants built by post_load_assign are not in the file.
inline bool kokoro_f16_tensor(const std::string & name, int64_t ne1) {
    auto has = [&](const char * w) { return name.find(w) != std::string::npos; };
    auto ends = [&](const char * w) {
        const size_t n = strlen(w);
        return name.size() >= n && name.compare(name.size() - n, n, w) == 0;
    };
    return ne1 > 0 && !has("voice_tensors") && !has("bias") && !has("gamma") && !has("beta") && !has("alpha") && !ends("embd") &&
           !ends("norm");
}

// The storage type of tensor `name` ([ne0, ne1, ..]; ne1 = 0: 1-D) under a runner's weight_type / f16_rest:
//  * weight_type Q8_0 / Q5_0 / Q4_0: that type exactly where the quantize tool's Kokoro rule quantizes
//    (tts_gguf_tensor_rule("kokoro", "kokoro." + name) == 1, quantize_impl.cpp:20-40) and the tensor is a
//    matrix; *bad_row is set when such a row is no whole number of 32-element blocks;
//  * weight_type F16, or f16_rest (`quantize -nqf`): F16 for the kokoro_f16_tensor tensors not quantized;
//  * F32 otherwise.
inline int kokoro_tensor_type(int weight_type, int f16_rest, const std::string & name, int64_t ne0, int64_t ne1, bool * bad_row) {
    if (wtype_q80_act(weight_type) && ne1 > 0) {
        tts_quantize_params qp;
        memset(&qp, 0, sizeof(qp));
        qp.quantize_type = weight_type;
        if (tts_gguf_tensor_rule("kokoro", ("kokoro." + name).c_str(), &qp) == 1) {
            if (ne0 % 32 && bad_row) *bad_row = true;
            return weight_type;
        }
    }
    return (weight_type == TTS_TYPE_F16 || f16_rest) && kokoro_f16_tensor(name, ne1) ? TTS_TYPE_F16 : TTS_TYPE_F32;
}

// With a file attached to the store the tensor takes the type the file gives it (missing: F32, and upload()
// reports it): F32 anywhere, F16 where kokoro_f16_tensor allows, Q8_0 / Q5_0 / Q4_0 where the rule quantizes.  Any other
// type, or a quantized tensor the rule would not quantize (a bias, say), sets *err to the reason with the file's
// tensor name.
inline int kokoro_store_type(const weight_store & w, int synth_type, const std::string & name, int64_t ne0, int64_t ne1, std::string * err) {
    if (!w.gguf) return synth_type;
    const int ft = w.file_type(name, TTS_TYPE_F32);
    bool ok = ft == TTS_TYPE_F32 || (ft == TTS_TYPE_F16 && kokoro_f16_tensor(name, ne1));
    if (wtype_q80_act(ft)) {
        bool bad = false;
        ok = kokoro_tensor_type(ft, 0, name, ne0, ne1, &bad) == ft && !bad;
    }
    if (!ok && err && err->empty())
        *err = "gguf: tensor '" + w.gguf_name(name) + "' has type " + std::to_string(ft) + ", which a Kokoro file cannot hold there";
    return ok ? ft : TTS_TYPE_F32;
}

// The generator over the file's "kokoro.decoder.generator.*" tensors (g NULL: synthetic weights).
tts_kokoro_gen * kokoro_gen_create(const tts_backend_iface * be, const tts_kokoro_gen_config * cfg, const tts_gguf * g);
// The generator's keys (build_*_from_file, prep_constants) and synthetic tensors into w.
int kokoro_gen_write(const tts_kokoro_gen_config * cfg, tts_gguf_writer * w);
// The generator's fields of cfg from the file's keys and tensor shapes; false (reason on stderr) when one is missing.
bool kokoro_gen_config_from_gguf(const tts_gguf * g, tts_kokoro_gen_config * cfg);

// f32 values of a weight (F16 widened, Q8_0 / Q5_0 / Q4_0 by ggml's dequantize_row_*) into dst; returns nelements * 4 (0 on a failed read)
uint64_t kokoro_read_weight(const tts_backend_iface & be, const tts_tensor * t, float * dst, uint64_t cap);

}  // namespace tts
