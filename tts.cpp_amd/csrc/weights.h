// The weight store every runner declares its persistent tensors in: one place that fills them with
// deterministic synthetic values (synth.h), uploads them whole to a backend, takes them from a GGUF
// file instead, or writes the synthetic values out as such a file.  A runner keeps only its
// declaration order (which defines the seeds), its own seed formula and its map from a tensor's role
// to a fill rule.
#pragma once

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/tts_gguf.h"
#include "graph.h"

namespace tts {

// How a tensor's synthetic values are made.
struct weight_fill {
    enum { UNIFORM, MATRIX, BYTES } rule;
    float a, b;               // UNIFORM: scale, offset; MATRIX: std, unused
    std::vector<char> bytes;  // BYTES: the tensor's bytes as the runner computed them

    // uniform in [-scale, scale) + offset (synth_f32); an F16 tensor gets the values rounded to nearest even
    static weight_fill uniform(float scale, float offset) { return {UNIFORM, scale, offset, {}}; }
    // roughly zero-mean values of standard deviation std in the tensor's own storage type (synth_fill)
    static weight_fill matrix(float std) { return {MATRIX, std, 0.f, {}}; }
    static weight_fill host(const void * data, size_t n) { return {BYTES, 0.f, 0.f, {(const char *)data, (const char *)data + n}}; }
};

struct weight_spec {
    tts_tensor * t;
    uint64_t seed;
    weight_fill fill;
    bool in_file;  // false: a constant the runner builds itself, never read from or written to a file
};

struct weight_store {
    tg::context wctx;  // the weights, and whatever other persistent tensors the runner keeps beside them
    void * wbuf = nullptr;
    size_t wbytes = 0;
    std::vector<weight_spec> specs;  // declaration order
    std::string prefix;              // GGUF name of a weight = prefix + its name
    const tts_gguf * gguf = nullptr;  // the file upload() reads (attach), else synthetic values
    // a runner whose tensor names differ from the file's: its name -> the file's (after the prefix); null = the same
    std::string (*file_name)(const std::string &) = nullptr;
    std::string gguf_name(const std::string & name) const { return prefix + (file_name ? file_name(name) : name); }

    void attach(const tts_gguf * g) { gguf = g; }
    // Storage type of `name` in the attached file; `type` without a file or without that tensor.
    int file_type(const std::string & name, int type) const;
    // A persistent tensor [ne0, ne1, ne2] (a 0 counts as 1), declared after index() others.
    tts_tensor * add(int type, int64_t ne0, int64_t ne1, int64_t ne2, const std::string & name, weight_fill fill, uint64_t seed,
                     bool in_file = true);
    uint64_t index() const { return specs.size(); }
    int32_t size() const { return (int32_t)specs.size(); }
    const tts_tensor * tensor(int32_t i) const { return i >= 0 && i < size() ? specs[(size_t)i].t : nullptr; }

    // The synthetic bytes of one spec.
    static void host_bytes(const weight_spec & s, std::vector<char> & host);
    // One buffer for every tensor (256-byte slots, declaration order), each uploaded whole through
    // set_tensor (the backend may keep its own layout): the attached file's bytes for the tensors it can
    // hold -- a missing tensor, another type or another element layout fails with the reason on stderr --
    // and the synthetic bytes otherwise.  Detaches the file.
    bool upload(const tts_backend_iface & be);
    // Replaces tensor i's bytes after upload (the type and shape it was declared with, nbytes of ggml's layout).
    bool set(const tts_backend_iface & be, int32_t i, const void * src, size_t nbytes);
    // Every file-backed tensor's synthetic bytes into w, trailing 1-sized dimensions dropped.
    int write(tts_gguf_writer * w) const;
    void release(const tts_backend_iface & be);
};

// search_for_gguf_keys: the first of `keys` that is present as a u32 -> *out (untouched when none is).
bool gguf_first_u32(const tts_gguf * g, std::initializer_list<const char *> keys, int32_t * out);
// Dimension d of tensor `name`, or -1 when the file has no such tensor.
int64_t gguf_tensor_dim(const tts_gguf * g, const std::string & name, int d);

}  // namespace tts
