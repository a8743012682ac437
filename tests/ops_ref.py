"""A numpy reference for the generic op kernels (k_ops.hip) that shares no code with them or with the oracle.

`run(g)` interprets a nodes.Graph on private copies of its buffers and returns them; `read(g, bufs, t)` gathers
one tensor out of such a set (or out of g's own buffers after a device / oracle run).  A tensor is
(ne, nb, type, bytes): it is gathered with as_strided on the backing bytes, so permuted, padded, offset and
in-place views are all just strides here.

How each op is evaluated, and why a kernel that is right lands on it:

  singly rounded   ADD SUB MUL DIV SQR SQRT SCALE ABS NEG RELU LEAKY_RELU CLAMP ROUND MOD: numpy float32
                   arithmetic (IEEE, correctly rounded), so the bar is bit equality.
  transcendental   SIN COS EXP TANH SIGMOID SILU and ROPE's angles: the float64 function, rounded once to
                   float32; everything around it in the op's own f32 order (1 / (1 + e), theta *= theta_scale).
  GELU             ggml's f16 table rule: x <= -10 -> 0, x >= 10 -> x, else table[f16(x)], the table being
                   f16(0.5 x (1 + tanh(sqrt(2/pi) x (1 + 0.044715 x^2)))) evaluated in f32 at every f16 value.
  reductions       SUM_ROWS, NORM, RMS_NORM, SOFT_MAX's denominator: math.fsum (exact), then rounded as the op
                   rounds (the kernels sum in f64, off by < 2^-44 relative over <= 257 terms).
  moves            DUP CONT CPY CONCAT REPEAT GET_ROWS: index arithmetic; I32 stays integer throughout.

F16 loads and stores go through numpy.float16 (round to nearest even).
"""
import ctypes
import math

import numpy as np
from numpy.lib.stride_tricks import as_strided

import ttship

F32, F16, I32 = ttship.F32, ttship.F16, ttship.I32
NP = {F32: np.float32, F16: np.float16, I32: np.int32}
OPN = {v: k for k, v in ttship.OP.items()}
UNN = {v: k for k, v in ttship.UNARY.items()}
VIEW_OPS = ("NONE", "VIEW", "RESHAPE", "PERMUTE", "TRANSPOSE")
f32 = np.float32


def ne_of(t):
    return [int(t.ne[i]) for i in range(4)]


def nb_of(t):
    return [int(t.nb[i]) for i in range(4)]


def shape_of(t):
    return tuple(ne_of(t)[::-1])


def view(g, bufs, t):
    """Tensor t as a writable (ne3, ne2, ne1, ne0) array over its bytes in bufs."""
    owner, at = g.buffer_of(t)
    b = bufs[id(owner)]
    dt = np.dtype(NP[t.type])
    ne, nb = ne_of(t), nb_of(t)
    end = at + sum((ne[d] - 1) * nb[d] for d in range(4)) + dt.itemsize
    assert at >= 0 and end <= b.nbytes and min(nb) >= 0, (at, end, b.nbytes)
    return as_strided(b[at:at + dt.itemsize].view(dt), shape=ne[::-1], strides=nb[::-1])


def read(g, bufs, t):
    return view(g, bufs, t).copy()


def elem_mask(g, t):
    """Boolean mask over t's owner buffer: the bytes that t's elements occupy."""
    owner, at = g.buffer_of(t)
    m = {id(owner): np.zeros(g.arrays[id(owner)].nbytes, np.uint8)}
    es = np.dtype(NP[t.type]).itemsize
    ne, nb = ne_of(t), nb_of(t)
    for k in range(es):
        as_strided(m[id(owner)][at + k:at + k + 1], shape=ne[::-1], strides=nb[::-1])[...] = 1
    return id(owner), m[id(owner)].astype(bool)


def fparam(t, i):
    return np.array([t.op_params[i]], np.int32).view(np.float32)[0]


def _src(g, t, k):
    if not t.src[k]:
        return None
    addr = ctypes.addressof(t.src[k].contents)
    for s in g.tensors:
        if ctypes.addressof(s) == addr:
            return s
    raise KeyError("source is not a tensor of this graph")


def _load(g, bufs, t):
    """Values as the op sees them: float32 for F32 / F16, int32 for I32."""
    a = read(g, bufs, t)
    return a.astype(np.float32) if t.type == F16 else a


def _to_type(vals, typ):
    if vals.dtype == np.dtype(NP[typ]):
        return vals
    if typ == I32:                       # C's float -> int conversion truncates
        return np.trunc(vals).astype(np.int32)
    with np.errstate(over="ignore"):
        return vals.astype(NP[typ])      # float32 -> float16 rounds to nearest even; int32 -> float rounds likewise


def _store(g, bufs, t, vals):
    view(g, bufs, t)[...] = _to_type(np.asarray(vals), t.type).reshape(shape_of(t))


# ---- GELU's f16 table ----------------------------------------------------------------------------------------
_GELU = None


def gelu_table():
    """table[h] = f16(gelu(f32(h))) over all 65536 f16 patterns, the f32 expression evaluated left to right as C
    does: 0.5f * x * (1.0f + tanhf(SQRT_2_OVER_PI * x * (1.0f + GELU_COEF_A * x * x)))."""
    global _GELU
    if _GELU is None:
        x = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
        a, s = f32(0.044715), f32(0.79788456080286535587989211986876)
        with np.errstate(all="ignore"):
            inner = (s * x) * (f32(1) + (a * x) * x)
            th = np.tanh(inner.astype(np.float64)).astype(np.float32)
            _GELU = ((f32(0.5) * x) * (f32(1) + th)).astype(np.float16)
    return _GELU


def _gelu(x):
    with np.errstate(all="ignore"):
        h = x.astype(np.float16).view(np.uint16)
    y = gelu_table()[h].astype(np.float32)
    y = np.where(x <= f32(-10), f32(0), y)
    return np.where(x >= f32(10), x, y).astype(np.float32)


def _t64(fn, x):
    with np.errstate(all="ignore"):
        return fn(x.astype(np.float64)).astype(np.float32)


def _round_half_away(x):
    """C's roundf: x - trunc(x) is exact in f32, so the tie test is exact."""
    r = np.trunc(x)
    with np.errstate(invalid="ignore"):
        up = np.abs(x - r) >= f32(0.5)
    return np.where(up, r + np.copysign(f32(1), x), r).astype(np.float32)


def _unary(t, x):
    op = OPN[t.op]
    p0, p1 = fparam(t, 0), fparam(t, 1)
    one, zero = f32(1), f32(0)
    with np.errstate(all="ignore"):
        if op == "SQR":
            return x * x
        if op == "SQRT":
            return np.sqrt(x)
        if op == "SIN":
            return _t64(np.sin, x)
        if op == "COS":
            return _t64(np.cos, x)
        if op == "SCALE":
            return x * p0
        if op == "CLAMP":                # ggml: MAX(MIN(x, max), min), the macros' (a < b ? a : b): NaN -> max
            v = np.where(x < p1, x, p1)
            return np.where(v > p0, v, p0).astype(np.float32)
        if op == "LEAKY_RELU":           # ggml_vec_leaky_relu_f32
            return np.where(x > 0, x, zero) + p0 * np.where(x < 0, x, zero)
        if op == "ROUND":
            return _round_half_away(x)
        if op == "MOD":
            return np.fmod(x, p0)
        u = UNN[t.op_params[0]]
        if u == "ABS":
            return np.abs(x)
        if u == "NEG":
            return -x
        if u == "RELU":
            return np.where(x > 0, x, zero).astype(np.float32)
        if u == "TANH":
            return _t64(np.tanh, x)
        if u == "EXP":
            return _t64(np.exp, x)
        if u == "SIGMOID":
            return one / (one + _t64(np.exp, -x))
        if u == "SILU":
            return x / (one + _t64(np.exp, -x))
        if u == "GELU":
            return _gelu(x)
    raise KeyError(op)


def _rows(a):
    return a.reshape(-1, a.shape[-1])


def _fsum_rows(a):
    return np.array([math.fsum(r.tolist()) for r in _rows(a)], np.float64).reshape(a.shape[:-1])


def _norm(t, x):
    n = x.shape[-1]
    eps = fparam(t, 0)
    with np.errstate(all="ignore"):
        if OPN[t.op] == "NORM":
            mean = (_fsum_rows(x) / n).astype(np.float32)[..., None]
            v = x - mean
            var = (_fsum_rows(v * v) / n).astype(np.float32)[..., None]
            return v * (f32(1) / np.sqrt(var + eps))
        mean = (_fsum_rows(x * x) / n).astype(np.float32)[..., None]
        return x * (f32(1) / np.sqrt(mean + eps))


def _soft_max(t, x, mask):
    scale = fparam(t, 0)
    with np.errstate(all="ignore"):
        w = x * scale
        if mask is not None:             # row i01 of slice (i02 % ne12, i03 % ne13), slope 1
            n3, n2, n1, _ = x.shape
            i3 = np.arange(n3) % mask.shape[0]
            i2 = np.arange(n2) % mask.shape[1]
            w = w + f32(1) * mask[i3][:, i2][:, :, :n1, :]
        mx = w.max(axis=-1, keepdims=True)
        e = _t64(np.exp, w - mx)
        inv = (1.0 / _fsum_rows(e)).astype(np.float32)[..., None]
        return e * inv


def _rope(t, x, pos, ff):
    n_dims, mode = int(t.op_params[1]), int(t.op_params[2])
    freq_base, freq_scale, attn = fparam(t, 5), fparam(t, 6), fparam(t, 8)
    neox = bool(mode & 2)
    h = n_dims // 2
    theta_scale = f32(np.power(np.float64(freq_base), np.float64(f32(-2.0) / f32(n_dims))))   # powf
    y = x.copy()
    n3, n2, n1, n0 = x.shape
    for i2 in range(n2):
        th = np.empty(h, np.float32)
        theta = f32(int(pos[i2]))
        for k in range(h):
            th[k] = theta
            theta = f32(theta * theta_scale)
        with np.errstate(all="ignore"):
            ang = freq_scale * (th / (ff[:h] if ff is not None else f32(1)))
            c = _t64(np.cos, ang) * attn
            s = _t64(np.sin, ang) * attn
            j0 = np.arange(h) if neox else 2 * np.arange(h)
            j1 = j0 + h if neox else j0 + 1
            x0, x1 = x[:, i2, :, j0], x[:, i2, :, j1]      # advanced index first: (h, n3, n1)
            c3, s3 = c[:, None, None], s[:, None, None]
            y[:, i2, :, j0] = x0 * c3 - x1 * s3
            y[:, i2, :, j1] = x0 * s3 + x1 * c3
    return y


def _tile_to(b, shape):
    return np.tile(b, [shape[i] // b.shape[i] for i in range(4)])


def eval_node(g, bufs, t):
    op = OPN[t.op]
    s0, s1, s2 = _src(g, t, 0), _src(g, t, 1), _src(g, t, 2)
    if op in VIEW_OPS:
        return
    if op in ("DUP", "CONT", "CPY"):
        _store(g, bufs, t, _to_type(_load(g, bufs, s0), t.type).reshape(-1))
    elif op in ("ADD", "SUB", "MUL", "DIV"):
        a = _load(g, bufs, s0)
        b = _tile_to(_load(g, bufs, s1), a.shape)
        with np.errstate(all="ignore"):
            _store(g, bufs, t, {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "DIV": np.divide}[op](a, b))
    elif op in ("SQR", "SQRT", "SIN", "COS", "SCALE", "CLAMP", "LEAKY_RELU", "ROUND", "MOD", "UNARY"):
        _store(g, bufs, t, _unary(t, _load(g, bufs, s0)))
    elif op in ("NORM", "RMS_NORM"):
        _store(g, bufs, t, _norm(t, _load(g, bufs, s0)))
    elif op == "SOFT_MAX":
        _store(g, bufs, t, _soft_max(t, _load(g, bufs, s0), _load(g, bufs, s1) if s1 is not None else None))
    elif op == "SUM_ROWS":
        _store(g, bufs, t, _fsum_rows(_load(g, bufs, s0)).astype(np.float32)[..., None])
    elif op == "GET_ROWS":
        tab, idx = _load(g, bufs, s0), read(g, bufs, s1)
        out = np.empty(shape_of(t), np.float32)
        for i12 in range(idx.shape[1]):
            for i11 in range(idx.shape[2]):
                out[i12, i11] = tab[i12, i11, idx[0, i12, i11, :], :]
        _store(g, bufs, t, out)
    elif op == "CONCAT":
        a, b = _load(g, bufs, s0), _load(g, bufs, s1)
        _store(g, bufs, t, np.concatenate([_to_type(a, t.type), _to_type(b, t.type)], axis=3 - int(t.op_params[0])))
    elif op == "REPEAT":
        _store(g, bufs, t, _tile_to(_to_type(_load(g, bufs, s0), t.type), shape_of(t)))
    elif op == "ROPE":
        pos = read(g, bufs, s1).reshape(-1)
        ff = read(g, bufs, s2).reshape(-1) if s2 is not None else None
        _store(g, bufs, t, _rope(t, _load(g, bufs, s0), pos, ff))
    else:
        raise KeyError(f"ops_ref has no {op}")


def run(g):
    """Interpret g's nodes in order on copies of its buffers; -> {id(owner tensor): bytes}."""
    bufs = {k: v.copy() for k, v in g.arrays.items()}
    for t in g.nodes:
        eval_node(g, bufs, t)
    return bufs
