"""Q5_0 in numpy, for the tests: random blocks, the unpack, the Q8_0 twin, ggml's quantize_row_q5_0_ref and
ggml_vec_dot_q5_0_q8_0 (generic C) restated with every float operation rounded to f32.

A Q5_0 block {f16 d; u8 qh[4]; u8 qs[16]} holds weights d * (q - 16), q - 16 in [-16, 15]: weight j
(j < 16) takes qs[j]'s low nibble and bit j of qh, weight j + 16 the high nibble and bit j + 16.  Its
"Q8_0 twin" is the Q8_0 block {d; int8 q - 16}: the same weights, and ggml's Q8_0 x Q8_0 dot rounds
sumi * (d_w * d_x) exactly as the Q5_0 x Q8_0 dot rounds (d_w * d_x) * sumi, so the CPU oracle run on the
twin is a bit-exact reference for Q5_0.
"""
import numpy as np

QK = 32
BLOCK = 22


def rand_q5_0(rng, N, K):
    """Random Q5_0 rows [N][K] as bytes, d around 0.01 (normal fp16)."""
    nb = N * (K // QK)
    b = np.zeros((nb, BLOCK), dtype=np.uint8)
    d = (0.01 * (0.5 + rng.random(nb))).astype(np.float16)
    b[:, 0:2] = d.view(np.uint8).reshape(nb, 2)
    b[:, 2:] = rng.integers(0, 256, size=(nb, 20), dtype=np.uint8)
    return b.reshape(-1)


def unpack(q):
    """bytes -> (d [nb] float16, q - 16 [nb][32] int8)."""
    b = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1, BLOCK)
    d = b[:, 0:2].copy().view(np.float16).reshape(-1)
    qh = b[:, 2:6].copy().view(np.uint32).reshape(-1)
    qs = b[:, 6:]
    j = np.arange(16, dtype=np.uint32)
    lo = (qs & 0x0F).astype(np.int32) | (((qh[:, None] >> j) & 1) << 4).astype(np.int32)
    hi = (qs >> 4).astype(np.int32) | (((qh[:, None] >> (j + 16)) & 1) << 4).astype(np.int32)
    return d, (np.concatenate([lo, hi], axis=1) - 16).astype(np.int8)


def twin_q8_0(q):
    """The Q8_0 bytes holding the same weights: block {d, int8 q - 16} (34 B)."""
    d, w = unpack(q)
    out = np.empty((d.size, 34), dtype=np.uint8)
    out[:, 0:2] = d.view(np.uint8).reshape(-1, 2)
    out[:, 2:] = w.view(np.uint8)
    return out.reshape(-1)


def quantize_row_q5_0(x):
    """quantize_row_q5_0_ref over the rows of x [N][K] float32 -> Q5_0 bytes (f32 operations in source order)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    xb = x.reshape(-1, QK)
    nb = xb.shape[0]
    # max: the signed value of largest magnitude, the first of equals (`if (amax < fabsf(v))`)
    idx = np.argmax(np.abs(xb), axis=1)
    vmax = xb[np.arange(nb), idx]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (vmax / np.float32(-16.0)).astype(np.float32)
        idv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    t = ((xb * idv[:, None]).astype(np.float32) + np.float32(16.5)).astype(np.float32)
    xi = np.minimum(31, np.trunc(t).astype(np.int32).astype(np.int8).astype(np.int32)).astype(np.uint8)  # (int8_t) cast, MIN(31, .)
    out = np.zeros((nb, BLOCK), dtype=np.uint8)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(nb, 2)
    x0, x1 = xi[:, :16], xi[:, 16:]
    out[:, 6:] = (x0 & 0x0F) | ((x1 & 0x0F) << 4)
    j = np.arange(16, dtype=np.uint32)
    qh = ((((x0 >> 4) & 1).astype(np.uint32) << j) | (((x1 >> 4) & 1).astype(np.uint32) << (j + 16))).sum(axis=1, dtype=np.uint32)
    out[:, 2:6] = qh.view(np.uint8).reshape(nb, 4)
    return out.reshape(-1)


def quantize_row_q8_0(x):
    """quantize_row_q8_0_ref of activation rows x [M][K] -> (d [M][K/32] float16, qs [M][K] int8)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    M, K = x.shape
    xb = x.reshape(-1, QK)
    amax = np.abs(xb).max(axis=1)
    d = (amax / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    v = (xb * idv[:, None]).astype(np.float32)
    qs = (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int8)  # roundf: half away from zero
    return d.astype(np.float16).reshape(M, K // QK), qs.reshape(M, K)


def vec_dot_q5_0_q8_0(q, x, N):
    """y[M][N] by ggml_vec_dot_q5_0_q8_0's generic loop: per (row, column), blocks ascending,
    sumf += (fp16_to_fp32(d_w) * fp16_to_fp32(d_x)) * sumi, each operation rounded to f32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    M, K = x.shape
    nb = K // QK
    dw, w = unpack(q)
    dw = dw.astype(np.float32).reshape(N, nb)
    w = w.astype(np.int32).reshape(N, nb, QK)
    dx, xq = quantize_row_q8_0(x)
    dx = dx.astype(np.float32)
    xq = xq.astype(np.int32).reshape(M, nb, QK)
    y = np.zeros((M, N), dtype=np.float32)
    for b in range(nb):
        sumi = np.einsum("mk,nk->mn", xq[:, b], w[:, b]).astype(np.float32)  # exact: |sumi| <= 32 * 16 * 127 < 2^24
        dd = (dw[None, :, b] * dx[:, b, None]).astype(np.float32)
        y = (y + (dd * sumi).astype(np.float32)).astype(np.float32)
    return y


def twin_gguf(src, dst):
    """Copy the GGUF file src to dst with every Q5_0 tensor re-encoded as its Q8_0 twin (keys as in the source)."""
    import ttship
    w = ttship.GgufWriter()
    keep = []
    with ttship.Gguf(src) as g:
        w.copy_kv(g)
        for name, ty, ne, _, _ in g.tensors():
            data = g.tensor_bytes(name)
            if ty == ttship.Q5_0:
                ty, data = ttship.Q8_0, twin_q8_0(data)
            keep.append(np.ascontiguousarray(data))
            w.add_tensor(name, ty, ne, keep[-1])
        w.write(dst)
    w.close()
