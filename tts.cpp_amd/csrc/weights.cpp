#include "weights.h"

#include <cstdio>
#include <cstring>

#include "synth.h"

namespace tts {

static size_t slot(size_t nbytes) { return (nbytes + 255) & ~(size_t)255; }

int weight_store::file_type(const std::string & name, int type) const {
    const int64_t i = gguf ? tts_gguf_find_tensor(gguf, gguf_name(name).c_str()) : -1;
    return i >= 0 ? tts_gguf_tensor_type(gguf, i) : type;
}

tts_tensor * weight_store::add(int type, int64_t ne0, int64_t ne1, int64_t ne2, const std::string & name, weight_fill fill,
                               uint64_t seed, bool in_file) {
    tts_tensor * t = tg::new_tensor_3d(wctx, type, ne0, ne1 ? ne1 : 1, ne2 ? ne2 : 1);
    tg::set_name(t, name);
    t->flags |= tg::TG_FLAG_PERSIST;
    specs.push_back({t, seed, std::move(fill), in_file});
    return t;
}

void weight_store::host_bytes(const weight_spec & s, std::vector<char> & host) {
    const tts_tensor * t = s.t;
    host.resize(tg::nbytes(t));
    const size_t n = (size_t)tg::nelements(t);
    switch (s.fill.rule) {
        case weight_fill::UNIFORM:
            if (t->type == TTS_TYPE_F16) {
                std::vector<float> f(n);
                synth_f32(f.data(), n, s.seed, s.fill.a, s.fill.b);
                for (size_t i = 0; i < n; ++i) ((uint16_t *)host.data())[i] = fp32_to_fp16_host(f[i]);
            } else {
                host.resize(n * sizeof(float));
                synth_f32((float *)host.data(), n, s.seed, s.fill.a, s.fill.b);
            }
            break;
        case weight_fill::MATRIX: synth_fill(t->type, host.data(), (int64_t)n / t->ne[0], t->ne[0], s.seed, s.fill.a); break;
        case weight_fill::BYTES: memcpy(host.data(), s.fill.bytes.data(), std::min(host.size(), s.fill.bytes.size())); break;
    }
}

// Same elements in the same order: equal after dropping the 1-sized dimensions (a GGUF bias [C]
// against a [1, C] tensor, assign_to_layer's transposed dup).
static bool same_squeezed_shape(const int64_t * a, const int64_t * b) {
    int64_t x[4], y[4];
    int nx = 0, ny = 0;
    for (int d = 0; d < 4; ++d) {
        if (a[d] != 1) x[nx++] = a[d];
        if (b[d] != 1) y[ny++] = b[d];
    }
    if (nx != ny) return false;
    for (int d = 0; d < nx; ++d)
        if (x[d] != y[d]) return false;
    return true;
}

// File tensor for t (assign_weight: the mapped bytes): present, same type, byte size and element
// layout; NULL (reason on stderr) otherwise.
static const void * gguf_source(const tts_gguf * g, const std::string & fname, const tts_tensor * t) {
    const int64_t i = tts_gguf_find_tensor(g, fname.c_str());
    if (i < 0) {
        fprintf(stderr, "gguf: tensor '%s' is missing\n", fname.c_str());
        return nullptr;
    }
    int64_t ne[4];
    tts_gguf_tensor_ndims(g, i, ne);
    if (tts_gguf_tensor_type(g, i) != t->type || !same_squeezed_shape(ne, t->ne) || tts_gguf_tensor_size(g, i) != tg::nbytes(t)) {
        fprintf(stderr, "gguf: tensor '%s' has type %d [%lld %lld %lld %lld], the runner needs type %d [%lld %lld %lld %lld]\n", fname.c_str(),
                tts_gguf_tensor_type(g, i), (long long)ne[0], (long long)ne[1], (long long)ne[2], (long long)ne[3], t->type, (long long)t->ne[0],
                (long long)t->ne[1], (long long)t->ne[2], (long long)t->ne[3]);
        return nullptr;
    }
    return tts_gguf_tensor_data(g, i);
}

bool weight_store::upload(const tts_backend_iface & be) {
    const tts_gguf * g = gguf;
    gguf = nullptr;
    size_t total = 0;
    for (auto & s : specs) total += slot(tg::nbytes(s.t));
    wbuf = be.alloc(be.ctx, total);
    if (!wbuf) return false;
    wbytes = total;
    size_t off = 0;
    std::vector<char> host;
    for (auto & s : specs) {
        s.t->data = (char *)wbuf + off;
        off += slot(tg::nbytes(s.t));
        const void * src;
        if (g && s.in_file) {
            src = gguf_source(g, gguf_name(s.t->name), s.t);
            if (!src) return false;
        } else {
            host_bytes(s, host);
            src = host.data();
        }
        if (be.set_tensor(be.ctx, s.t, src) != 0) return false;
    }
    return true;
}

bool weight_store::set(const tts_backend_iface & be, int32_t i, const void * src, size_t nbytes) {
    tts_tensor * t = i >= 0 && i < size() ? specs[(size_t)i].t : nullptr;
    if (!t || !t->data || !src || nbytes != tg::nbytes(t)) return false;
    return be.set_tensor(be.ctx, t, src) == 0;
}

int weight_store::write(tts_gguf_writer * w) const {
    std::vector<char> host;
    for (auto & s : specs) {
        if (!s.in_file) continue;
        host_bytes(s, host);
        int nd = 4;
        while (nd > 1 && s.t->ne[nd - 1] == 1) --nd;
        const int st = tts_gguf_add_tensor(w, gguf_name(s.t->name).c_str(), s.t->type, nd, s.t->ne, host.data(), host.size());
        if (st != TTS_STATUS_SUCCESS) return st;
    }
    return TTS_STATUS_SUCCESS;
}

void weight_store::release(const tts_backend_iface & be) {
    if (wbuf) be.free(be.ctx, wbuf);
    wbuf = nullptr;
    wbytes = 0;
}

bool gguf_first_u32(const tts_gguf * g, std::initializer_list<const char *> keys, int32_t * out) {
    for (const char * k : keys) {
        const int64_t i = tts_gguf_find_key(g, k);
        uint32_t v;
        if (i >= 0 && tts_gguf_get_u32(g, i, &v)) {
            *out = (int32_t)v;
            return true;
        }
    }
    return false;
}

int64_t gguf_tensor_dim(const tts_gguf * g, const std::string & name, int d) {
    const int64_t i = tts_gguf_find_tensor(g, name.c_str());
    if (i < 0) return -1;
    int64_t ne[4];
    tts_gguf_tensor_ndims(g, i, ne);
    return ne[d];
}

}  // namespace tts
