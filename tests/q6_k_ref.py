"""Q6_K in numpy, for the tests: the format, dequantize_row_q6_K, ggml_vec_dot_q6_K_q8_K's generic C order and
quantize_row_q6_K_ref, restated from their description (DESIGN, "Q6_K").  ggml itself is not available to the tests
and the CPU oracle holds no Q6_K, so this module is the reference; that it equals ggml's own code is unverified.

block_q6_K (210 B per 256 weights): u8 ql[128], u8 qh[64], i8 scales[16], f16 d (byte 208).  Weight e is
d * scales[e / 16] * a[e] with a[e] in [-32, 31]; for half h = 0, 1 and l = 0 .. 31, q = ql + 64 h, g = qh + 32 h:
    a[128 h + l]      = ((q[l]      & 15) | (((g[l] >> 0) & 3) << 4)) - 32
    a[128 h + l + 32] = ((q[l + 32] & 15) | (((g[l] >> 2) & 3) << 4)) - 32
    a[128 h + l + 64] = ((q[l]      >> 4) | (((g[l] >> 4) & 3) << 4)) - 32
    a[128 h + l + 96] = ((q[l + 32] >> 4) | (((g[l] >> 6) & 3) << 4)) - 32
"""
import numpy as np

QK = 256
BLOCK = 210
f32 = np.float32


def unpack(q):
    """bytes -> (d [nb] float16, scales [nb][16] int8, a [nb][256] int8)."""
    b = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1, BLOCK)
    nb = b.shape[0]
    ql, qh = b[:, :128].reshape(nb, 2, 64).astype(np.int32), b[:, 128:192].reshape(nb, 2, 32).astype(np.int32)
    a = np.empty((nb, 2, 4, 32), dtype=np.int32)
    a[:, :, 0] = (ql[:, :, :32] & 15) | (((qh >> 0) & 3) << 4)
    a[:, :, 1] = (ql[:, :, 32:] & 15) | (((qh >> 2) & 3) << 4)
    a[:, :, 2] = (ql[:, :, :32] >> 4) | (((qh >> 4) & 3) << 4)
    a[:, :, 3] = (ql[:, :, 32:] >> 4) | (((qh >> 6) & 3) << 4)
    sc = b[:, 192:208].copy().view(np.int8)
    d = b[:, 208:210].copy().view(np.float16).reshape(-1)
    return d, sc, (a.reshape(nb, QK) - 32).astype(np.int8)


def pack(d, sc, L):
    """(d [nb] float16, scales [nb][16] int8, L [nb][256] in 0 .. 63) -> bytes, quantize_row_q6_K_ref's packing."""
    nb = L.shape[0]
    L = L.astype(np.uint8).reshape(nb, 2, 4, 32)
    out = np.zeros((nb, BLOCK), dtype=np.uint8)
    ql = np.empty((nb, 2, 64), dtype=np.uint8)
    ql[:, :, :32] = (L[:, :, 0] & 15) | ((L[:, :, 2] & 15) << 4)
    ql[:, :, 32:] = (L[:, :, 1] & 15) | ((L[:, :, 3] & 15) << 4)
    qh = (L[:, :, 0] >> 4) | ((L[:, :, 1] >> 4) << 2) | ((L[:, :, 2] >> 4) << 4) | ((L[:, :, 3] >> 4) << 6)
    out[:, :128] = ql.reshape(nb, 128)
    out[:, 128:192] = qh.reshape(nb, 64)
    out[:, 192:208] = np.asarray(sc, dtype=np.int8).view(np.uint8)
    out[:, 208:210] = np.asarray(d, dtype=np.float16).view(np.uint8).reshape(nb, 2)
    return out.reshape(-1)


def rand_q6_K(rng, N, K):
    """Random Q6_K rows [N][K] as bytes: every code, scales over all of int8, d around 1e-4 (normal fp16)."""
    nb = N * (K // QK)
    d = (1e-4 * (0.5 + rng.random(nb))).astype(np.float16)
    sc = rng.integers(-128, 128, size=(nb, 16)).astype(np.int8)
    return pack(d, sc, rng.integers(0, 64, size=(nb, QK)))


def dequantize(q, K, N):
    """dequantize_row_q6_K: y[e] = (d * (float)scales[e / 16]) * (float)a[e], each product rounded to f32."""
    d, sc, a = unpack(q)
    ds = (d.astype(f32)[:, None] * sc.astype(f32)).astype(f32)  # [nb][16]
    return (np.repeat(ds, 16, axis=1) * a.astype(f32)).astype(f32).reshape(N, K)


def nearest_int(v):
    """ggml's nearest_int on f32 values: round half to even."""
    return np.rint(np.asarray(v, dtype=f32)).astype(np.int32)


def quantize_row_q8_K(x):
    """quantize_row_q8_K_ref over x [M][K] -> (d [M][nb] float32, q8 [M][nb][256] int8): the signed value of largest
    magnitude (the first of equals) gives iscale = -127 / max, q = min(127, nearest_int(iscale * x)), d = 1 / iscale;
    an all-zero block has d = 0."""
    x = np.ascontiguousarray(x, dtype=f32)
    M, K = x.shape
    xb = x.reshape(-1, QK)
    idx = np.argmax(np.abs(xb), axis=1)
    mx = xb[np.arange(xb.shape[0]), idx]
    nz = np.abs(mx) != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        iscale = np.where(nz, f32(-127.0) / mx, f32(0)).astype(f32)
        d = np.where(nz, f32(1.0) / iscale, f32(0)).astype(f32)
    q = np.minimum(127, nearest_int((iscale[:, None] * xb).astype(f32)))
    return d.reshape(M, K // QK), q.astype(np.int8).reshape(M, K // QK, QK)


def aux32(q, x, N):
    """The integer sums of every (column, row, block): aux[M][N][nb][8], aux[.., l] = sum over e = l (mod 8) of
    scales[e / 16] * q8[e] * a[e]; also (d_w [N][nb] f32, d_x [M][nb] f32)."""
    x = np.ascontiguousarray(x, dtype=f32)
    M, K = x.shape
    nb = K // QK
    dw, sc, a = unpack(q)
    sa = (np.repeat(sc.astype(np.int64), 16, axis=1) * a.astype(np.int64)).reshape(N, nb, 32, 8)  # e = 8 t + l
    dx, q8 = quantize_row_q8_K(x)
    q8 = q8.astype(np.int64).reshape(M, nb, 32, 8)
    aux = np.einsum("mbtl,nbtl->mnbl", q8, sa)
    return aux, dw.astype(f32).reshape(N, nb), dx


def vec_dot_q6_K_q8_K(q, x, N):
    """y[M][N] by ggml_vec_dot_q6_K_q8_K's generic C loop: per (row, column), blocks ascending, dd = d_w * d_x (one
    rounding), sums[l] = sums[l] + dd * (float)aux32[l] (multiply and add each rounded), then
    sumf = ((0 + sums[0]) + sums[1]) + .. + sums[7]."""
    aux, dw, dx = aux32(q, x, N)
    M, _, nb, _ = aux.shape
    assert np.abs(aux).max(initial=0) < 2 ** 24  # (float)aux32 is exact
    sums = np.zeros((M, N, 8), dtype=f32)
    for b in range(nb):
        dd = (dw[None, :, b] * dx[:, b, None]).astype(f32)  # [M][N]
        sums = (sums + (dd[:, :, None] * aux[:, :, b].astype(f32)).astype(f32)).astype(f32)
    y = np.zeros((M, N), dtype=f32)
    for l in range(8):
        y = (y + sums[:, :, l]).astype(f32)
    return y


def vec_dot_one_sum_per_block(q, x, N):
    """Another order, which the kernels must not compute: sumf += dd * (float)(aux32[0] + .. + aux32[7]) per block."""
    aux, dw, dx = aux32(q, x, N)
    nb = aux.shape[2]
    y = np.zeros(aux.shape[:2], dtype=f32)
    for b in range(nb):
        dd = (dw[None, :, b] * dx[:, b, None]).astype(f32)
        y = (y + (dd * aux[:, :, b].sum(axis=2).astype(f32)).astype(f32)).astype(f32)
    return y


def _qx_round(iscale, x):
    return np.clip(nearest_int((iscale[:, None] * x).astype(f32)), -32, 31)


def _qx_sums(x, l):
    """sumlx = sum (w * x) * l and suml2 = sum (w * l) * l with w = x * x, accumulated in element order in f32."""
    w = (x * x).astype(f32)
    lf = l.astype(f32)
    tx, t2 = ((w * x).astype(f32) * lf).astype(f32), ((w * lf).astype(f32) * lf).astype(f32)
    sumlx, suml2 = np.zeros(x.shape[0], dtype=f32), np.zeros(x.shape[0], dtype=f32)
    for i in range(x.shape[1]):
        sumlx = (sumlx + tx[:, i]).astype(f32)
        suml2 = (suml2 + t2[:, i]).astype(f32)
    return sumlx, suml2


def make_qx_quants(x):
    """make_qx_quants(16, 32, x, L, rmse_type = 1, no weights) over sub-blocks x [n][16] -> (scale [n] f32, L [n][16]
    in 0 .. 63).  19 candidate scales -(32 + 0.1 is) / max, is = -9 .. 9 (is = 0 first), weights x^2; a later candidate
    wins only when its sumlx^2 / suml2 is strictly larger."""
    x = np.ascontiguousarray(x, dtype=f32)
    n = x.shape[0]
    idx = np.argmax(np.abs(x), axis=1)
    mx = x[np.arange(n), idx]
    live = np.abs(mx) >= f32(1e-15)
    mxs = np.where(live, mx, f32(1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iscale = (f32(-32.0) / mxs).astype(f32)
        l = _qx_round(iscale, x)
        L = l + 32
        sumlx, suml2 = _qx_sums(x, l)
        scale = np.where(suml2 != 0, sumlx / np.where(suml2 != 0, suml2, f32(1)), f32(0)).astype(f32)
        best = (scale * sumlx).astype(f32)
        for i_s in range(-9, 10):
            if i_s == 0:
                continue
            iscale = (-(f32(32.0) + f32(0.1) * f32(i_s)).astype(f32) / mxs).astype(f32)
            l = _qx_round(iscale, x)
            sumlx, suml2 = _qx_sums(x, l)
            better = (suml2 > 0) & ((sumlx * sumlx).astype(f32) > (best * suml2).astype(f32))
            L = np.where(better[:, None], l + 32, L)
            ns = (sumlx / np.where(suml2 > 0, suml2, f32(1))).astype(f32)
            scale = np.where(better, ns, scale).astype(f32)
            best = np.where(better, (ns * sumlx).astype(f32), best).astype(f32)
    scale = np.where(live, scale, f32(0)).astype(f32)
    L = np.where(live[:, None], L, 0)
    return scale, L


def quantize_row_q6_K(x):
    """quantize_row_q6_K_ref over the rows of x [N][K] float32 -> Q6_K bytes."""
    x = np.ascontiguousarray(x, dtype=f32)
    xb = x.reshape(-1, 16, 16)
    nb = xb.shape[0]
    scale, L = make_qx_quants(xb.reshape(-1, 16))
    scale, L = scale.reshape(nb, 16), L.reshape(nb, 16, 16)
    idx = np.argmax(np.abs(scale), axis=1)  # the first sub-block of largest |scale|
    max_scale = scale[np.arange(nb), idx]
    zero = np.abs(max_scale) < f32(1e-15)
    ms = np.where(zero, f32(1), max_scale)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iscale = (f32(-128.0) / ms).astype(f32)
        d16 = (f32(1.0) / iscale).astype(f32).astype(np.float16)
        sc = np.minimum(127, nearest_int((iscale[:, None] * scale).astype(f32)))
        d = (d16.astype(f32)[:, None] * sc.astype(f32)).astype(f32)  # [nb][16]
        live = d != 0
        ds = np.where(live, d, f32(1))
        l = np.clip(nearest_int((xb / ds[:, :, None]).astype(f32)), -32, 31) + 32
    L = np.where(live[:, :, None], l, L)
    L = np.where(zero[:, None, None], 0, L)
    sc = np.where(zero[:, None], 0, sc)
    d16 = np.where(zero, np.float16(0), d16)
    return pack(d16, sc.astype(np.int8), L.reshape(nb, QK))


# ---- the kernel cases of tests/test_q6_k_gpu.py, shared with the CPU check that the reference tells orders apart ----
# odd N at K = 256: every other row is 2-byte aligned only; 33, 100, 17: rows that fill no 8-row wave tile
GEMV_SHAPES = [(256, 1), (256, 3), (256, 33), (512, 96), (768, 100), (1024, 64), (2048, 17), (4096, 8),
               (256, 7), (256, 9), (512, 31), (512, 41)]  # 7 / 9 / 31 / 33 / 41: either side of the 8-row and 32-row tiles
GEMV_COLS = [1, 2, 3, 5, 8]
GEMM_SHAPES = [(256, 3), (512, 96), (1024, 100), (4096, 16)]
GEMM_COLS = [9, 12, 15, 16, 17, 32, 33, 64, 65, 100]  # 15 / 16 / 17, 32 / 33, 64 / 65: the 16-column tile's edges


def case(K, N, M, seed=0):
    rng = np.random.default_rng(K * 7 + N * 3 + M + 1000003 * seed)
    return rand_q6_K(rng, N, K), rng.standard_normal((M, K)).astype(f32)
