"""Q4_0 in numpy, for the tests: two references that need nothing from the CPU oracle beyond what it has.

A Q4_0 block {f16 d; u8 qs[16]} holds weights d * (q - 8), q - 8 in [-8, 7]: weight j (j < 16) takes qs[j]'s
low nibble, weight j + 16 its high nibble.  ggml_vec_dot_q4_0_q8_0 (generic C) adds, per block,
((float)sumi * d_w) * d_x -- not Q8_0's sumi * (d_w * d_x) nor Q5_0's (d_w * d_x) * sumi -- so the Q8_0 twin
{d; int8 q - 8} does not pin its bits in general.

R1 (general d): `vec_dot_q4_0_q8_0`, ggml's loop restated with every float operation rounded to f32 in
ggml's order.  The only reference that sees the association order.

R2 (trimmed d): with the low two mantissa bits of every block's f16 d cleared (`trim_d`), d_w has at most 9
significant bits; |sumi| <= 32 * 8 * 127 < 2^15, so sumi * d_w (<= 24 bits) and d_w * d_x (<= 20 bits) are
both exact in f32, and either association is one rounding of the same real number.  A trimmed block therefore
equals its Q8_0 twin bit for bit under the oracle, which lets whole graphs and runners be compared with the
unchanged oracle.  R2 cannot tell the two orders apart, so no kernel route is checked by it alone.
"""
import numpy as np

from q5_0_ref import quantize_row_q8_0

QK = 32
BLOCK = 18


def rand_q4_0(rng, N, K):
    """Random Q4_0 rows [N][K] as bytes, d around 0.01 (normal fp16, all ten mantissa bits in use)."""
    nb = N * (K // QK)
    b = np.zeros((nb, BLOCK), dtype=np.uint8)
    d = (0.01 * (0.5 + rng.random(nb))).astype(np.float16)
    b[:, 0:2] = d.view(np.uint8).reshape(nb, 2)
    b[:, 2:] = rng.integers(0, 256, size=(nb, 16), dtype=np.uint8)
    return b.reshape(-1)


def unpack(q):
    """bytes -> (d [nb] float16, q - 8 [nb][32] int8)."""
    b = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1, BLOCK)
    d = b[:, 0:2].copy().view(np.float16).reshape(-1)
    qs = b[:, 2:]
    lo, hi = (qs & 0x0F).astype(np.int32), (qs >> 4).astype(np.int32)
    return d, (np.concatenate([lo, hi], axis=1) - 8).astype(np.int8)


def dequantize(q, K, N):
    """dequantize_row_q4_0: (float)(q - 8) * d, rows [N][K]."""
    d, w = unpack(q)
    return (w.astype(np.float32) * d.astype(np.float32)[:, None]).astype(np.float32).reshape(N, K)


def trim_d(q):
    """The same blocks with the low two mantissa bits of every d cleared (u16 & 0xFFFC)."""
    b = np.array(q, dtype=np.uint8).reshape(-1, BLOCK)
    b[:, 0] &= 0xFC  # little endian: byte 0 holds the low mantissa bits
    return b.reshape(-1)


def twin_q8_0(q):
    """The Q8_0 bytes holding the same weights: block {d, int8 q - 8} (34 B)."""
    d, w = unpack(q)
    out = np.empty((d.size, 34), dtype=np.uint8)
    out[:, 0:2] = d.view(np.uint8).reshape(-1, 2)
    out[:, 2:] = w.view(np.uint8)
    return out.reshape(-1)


def quantize_row_q4_0(x):
    """quantize_row_q4_0_ref over the rows of x [N][K] float32 -> Q4_0 bytes (f32 operations in source order)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    xb = x.reshape(-1, QK)
    nb = xb.shape[0]
    # max: the signed value of largest magnitude, the first of equals (`if (amax < fabsf(v))`)
    idx = np.argmax(np.abs(xb), axis=1)
    vmax = xb[np.arange(nb), idx]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (vmax / np.float32(-8.0)).astype(np.float32)
        idv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    t = ((xb * idv[:, None]).astype(np.float32) + np.float32(8.5)).astype(np.float32)
    xi = np.minimum(15, np.trunc(t).astype(np.int32).astype(np.int8).astype(np.int32)).astype(np.uint8)  # (int8_t) cast, MIN(15, .)
    out = np.zeros((nb, BLOCK), dtype=np.uint8)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(nb, 2)
    out[:, 2:] = xi[:, :16] | (xi[:, 16:] << 4)
    return out.reshape(-1)


def vec_dot_q4_0_q8_0(q, x, N):
    """R1.  y[M][N] by ggml_vec_dot_q4_0_q8_0's generic loop: per (row, column), blocks ascending from 0.0f,
    sumf += ((float)sumi * fp16_to_fp32(d_w)) * fp16_to_fp32(d_x), each operation rounded to f32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    M, K = x.shape
    nb = K // QK
    dw, w = unpack(q)
    dw = dw.astype(np.float32).reshape(N, nb)
    w = w.astype(np.float32).reshape(N, nb, QK)  # small integers: f32 matrix products of them are exact (< 2^24)
    dx, xq = quantize_row_q8_0(x)
    dx = dx.astype(np.float32)
    xq = xq.astype(np.float32).reshape(M, nb, QK)
    y = np.zeros((M, N), dtype=np.float32)
    for b in range(nb):
        sumi = xq[:, b] @ w[:, b].T  # exact: |sumi| <= 32 * 8 * 127 < 2^15
        t = (sumi * dw[None, :, b]).astype(np.float32)
        t = (t * dx[:, b, None]).astype(np.float32)
        y = (y + t).astype(np.float32)
    return y


def _regguf(src, dst, fn):
    import ttship
    w = ttship.GgufWriter()
    keep = []
    with ttship.Gguf(src) as g:
        w.copy_kv(g)
        for name, ty, ne, _, _ in g.tensors():
            data = g.tensor_bytes(name)
            if ty == ttship.Q4_0:
                ty, data = fn(data)
            keep.append(np.ascontiguousarray(data))
            w.add_tensor(name, ty, ne, keep[-1])
        w.write(dst)
    w.close()


def trim_gguf(src, dst):
    """Copy the GGUF file src to dst with every Q4_0 tensor's d trimmed (keys as in the source)."""
    import ttship
    _regguf(src, dst, lambda data: (ttship.Q4_0, trim_d(data)))


def twin_gguf(src, dst):
    """Copy the GGUF file src to dst with every Q4_0 tensor re-encoded as its Q8_0 twin (keys as in the source)."""
    import ttship
    _regguf(src, dst, lambda data: (ttship.Q8_0, twin_q8_0(data)))


# ---- the kernel cases of tests/test_q4_0_gpu.py, shared with the CPU check that R1 tells the two orders apart on them ----
# K % 256 != 0 -> the general kernel only; N = 1, N % RW != 0; (4096, 1024) fills every CU with 4-row slabs
GEMV_SHAPES = [(96, 5), (160, 33), (256, 1), (256, 3), (1024, 33), (2048, 64), (4096, 1024)]
GEMV_COLS = [1, 2, 3, 5, 8]
# (96, 70): K % 256 != 0 and rows / columns that fill no 64 x 64 tile; N = 1000: a ragged last row tile
GEMM_SHAPES = [(256, 16), (1024, 1000), (4096, 1024), (96, 70)]
GEMM_COLS = [9, 17, 32, 100, 130]


def _case(seed, K, N, M):
    """Weights (general d) and activations on which the two association orders part.  Random data alone never
    tells them apart: |sumi| stays near 1000, and below 2^13 both sumi * d_w (<= 24 bits) and d_w * d_x are
    exact.  So block b has a random pattern p[b] in [-8, 7]: the even rows' quants are p[b] but for four random
    elements, the even columns' activations are +- p[b] times a random scale; their sumi is about 127 / 8 *
    sum p^2 = 10000, where fl(fl(sumi * d_w) * d_x) and fl(sumi * fl(d_w * d_x)) differ in many terms (test_q4_0_cpu.py
    checks that they do on every case).  Odd rows and odd columns are random throughout."""
    rng = np.random.default_rng(seed)
    w = rand_q4_0(rng, N, K).reshape(N, K // QK, BLOCK)
    x = rng.standard_normal((M, K)).astype(np.float32)
    nb = K // QK
    pat = rng.integers(0, 16, size=(nb, QK), dtype=np.uint8)  # nibbles q
    ne = (N + 1) // 2
    qe = np.broadcast_to(pat, (ne, nb, QK)).copy()
    for _ in range(4):
        j = rng.integers(0, QK, size=(ne, nb, 1))
        np.put_along_axis(qe, j, rng.integers(0, 16, size=(ne, nb, 1), dtype=np.uint8), axis=2)
    w[0::2, :, 2:] = qe[:, :, :16] | (qe[:, :, 16:] << 4)
    me = (M + 1) // 2
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=(me, nb, 1))
    scale = (0.05 + 0.2 * rng.random((me, nb, 1))).astype(np.float32)
    x.reshape(M, nb, QK)[0::2] = (pat.astype(np.float32) - 8.0)[None] * sign * scale
    return w.reshape(-1), x


# seeds kept because the orders part on them (test_r1_discriminates); the three small cases listed need another seed
GEMV_SEED_BUMP = {(96, 5, 8): 1, (160, 33, 1): 2, (1024, 33, 2): 1}


def gemv_case(K, N, M):
    return _case(K * 7 + N + M + 100000 * GEMV_SEED_BUMP.get((K, N, M), 0), K, N, M)


def gemm_case(K, N, M):
    return _case(K * 13 + N + M, K, N, M)


# MUL_MAT + residual ADD at the Q5_0 module's four shapes: the fused residual epilogue, GEMV and GEMM
RESIDUAL_SHAPES = [(256, 40, 1), (1024, 130, 3), (96, 33, 2), (512, 64, 20)]


def residual_case(K, N, M):
    return _case(K * 17 + N + M, K, N, M)
