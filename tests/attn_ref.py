"""A numpy reference for decode attention (k_attn.hip) that shares no code with the kernels, the oracle or ops_ref.

`attention(q, k, v, ...)` takes each operand as a Tensor(ne, nb, buf, offs): ggml extents and byte strides over a
byte buffer, gathered with as_strided, so cache views, padding, misaligned bases and shared heads are only strides:

  q [hd, n, H, B]    k [hd, P, Hk, Bk]    v [P, hd, Hv, Bv]    mask rows of P floats    bias [P, n, H]

Query head h reads K head h // (H / Hk) and V head h // (H / Hv); sequence b reads K / V sequence b // (B / Bk).
A ragged launch gives each sequence its own key count (pseq), byte offsets of its K and V (koff, voff) and the
float offset of its mask rows (moff), whose row stride is then that sequence's key count.

It rounds where the unfused op chain rounds, and nowhere else:

  s_i  = f32(fsum_d f32(K[d, i] * q[d]))       mul_mat: f32 products, summed exactly, rounded once
  w_i  = f32(s_i + bias_i)                     (only with a bias; the T5 chain adds it before the scale)
  w_i  = f32(w_i * scale)                      soft_max_ext
  w_i  = f32(w_i + mask_i)
  m    = max_i w_i
  e_i  = f32(exp(f64(f32(w_i - m))))           the float64 exp, rounded once
  inv  = f32(1 / fsum_i e_i)                   the division in f64
  p_i  = f32(e_i * inv)
  o_d  = f32(fsum_i f32(p_i * V[i, d]))        mul_mat again

Why a kernel that is right lands on these values: the kernels and the oracle form the same f32 products and add
them in f64.  A sum of n f32 values accumulated in f64 in any order is within n * 2^-53 relative of the exact sum
of their magnitudes, under 2^-44 for up to 512 terms of like sign and still far below the 2^-24 spacing of the f32
result otherwise, so after the one rounding to f32 it is the exact sum's rounding except when the exact sum lies
within that distance of an f32 midpoint (about one value in 2^20).  Everything else in the chain is a single
IEEE operation or the correctly rounded exp.  The tests' seeds are chosen so that the oracle, which sums in
sequence, meets the bars below against this reference on the CPU before any device is involved.

The bars (`check`):

  "bits"    bit equality: wherever the kernel's sums are the oracle's, term by term (up to 64 keys; k_attn_bias).
  "ulp1"    at most 1 ulp, at least 99.9 % of the elements bit-equal: kernels that reassociate the f64 sums.
  "large"   rows whose largest |w| exceeds 8.  An f32 midpoint flip in one score w_i moves its term by about
            2^-24 |w_i| relative, so no bound in ulps of the output holds; the error is held per element to
            C * 2^-24 * (1 + max|w|) * sum_i p_i |v_i|.  C from the rounding points, u = 2^-24, W = max|w|: s_i,
            the scale and the mask add each put at most u |w_i| on w_i (3u W); the maximum carries the same 3u W;
            the subtraction rounds once more on |w_i - m| <= 2W (2u W): the exponent is off by at most 8u W,
            and e_i by that plus its own rounding, (8W + 1) u relative.  The denominator is a weighted mean of
            the same relative errors, (8W + 1) u again; inv and p_i round once each: p_i is within (16W + 4) u.
            The product with v and the final rounding add 2u: one evaluation is within (16W + 6) u sum p|v| of
            exact arithmetic, two independent ones (device and reference) within (32W + 12) u <= 32 (1 + W) u.
            C = 32.  test_attn_ref_cpu.py prints the worst ratio the oracle reaches against this reference and
            asserts that twice that figure is still within C.

A row whose keys are all masked has no defined result (max = -inf, exp(nan)); the reference leaves it NaN and
reports it in `dead`, and the tests compare that row's NaN positions with the oracle's instead.
"""
import math
from collections import namedtuple

import numpy as np
from numpy.lib.stride_tricks import as_strided

Tensor = namedtuple("Tensor", "ne nb buf offs")
Result = namedtuple("Result", "out wmax pav dead")   # out, pav [B, n, H, hd]; wmax, dead [B, n, H]

C_LARGE = 32.0
f32 = np.float32


def tensor(arr, ne, nb, offs=0):
    """A Tensor over a float32 array's bytes."""
    return Tensor(list(ne), list(nb), np.ascontiguousarray(arr).view(np.uint8).reshape(-1), int(offs))


def gather(t, offs=0):
    """The tensor's elements as an (ne3, ne2, ne1, ne0) float32 array."""
    at = t.offs + int(offs)
    end = at + sum((t.ne[d] - 1) * t.nb[d] for d in range(4)) + 4
    assert at >= 0 and end <= t.buf.nbytes and min(t.nb) >= 0, (at, end, t.buf.nbytes)
    return as_strided(t.buf[at:at + 4].view(np.float32), shape=t.ne[::-1], strides=t.nb[::-1]).copy()


def _fsum_last(a):
    """Exact sums over the last axis of a float32 array, correctly rounded to float64: math.fsum.  A row skips the
    Python loop where numpy's float64 sum is provably exact already: every term is a multiple of q = 2^(emin - 24)
    (emin the smallest binary exponent among the non-zero terms, each of which has 24 significant bits), and
    when sum |term| < 2^53 q every partial sum in any order is a multiple of q below 2^53 q, hence a float64."""
    rows = a.reshape(-1, a.shape[-1]).astype(np.float64)
    _, ex = np.frexp(rows)
    emin = np.where(rows == 0, 4096, ex).min(axis=1)
    sums = rows.sum(axis=1)
    proven = np.abs(rows).sum(axis=1) * 1.001 < np.ldexp(1.0, np.minimum(emin, 900) - 24 + 53)
    for i in np.flatnonzero(~proven):
        sums[i] = math.fsum(rows[i].tolist())
    return sums.reshape(a.shape[:-1])


def attention(q, k, v, scale, mask=None, mask_per_seq=False, bias=None, pseq=None, koff=None, voff=None, moff=None):
    """mask: float32 array, any shape, read as rows of P floats: row t of sequence b starts at float
    (b * n * P if mask_per_seq else 0) + t * P, or at moff[b] + t * pseq[b] in a ragged launch."""
    hd, n, H, B = q.ne
    Hk, Bk, Hv, Bv = k.ne[2], k.ne[3], v.ne[2], v.ne[3]
    assert k.ne[0] == hd and v.ne[1] == hd and v.ne[0] == k.ne[1]
    assert H % Hk == 0 and H % Hv == 0
    ragged = pseq is not None
    assert ragged or (B % Bk == 0 and B % Bv == 0)
    qa = gather(q)                                                   # [B, H, n, hd]
    mflat = None if mask is None else np.ascontiguousarray(mask, np.float32).reshape(-1)
    ba = None if bias is None else np.ascontiguousarray(bias, np.float32)   # [H, n, P]
    scale = f32(scale)
    out = np.full((B, n, H, hd), np.nan, np.float32)
    pav = np.full((B, n, H, hd), np.nan, np.float64)
    wmax = np.zeros((B, n, H), np.float64)
    dead = np.zeros((B, n, H), bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            P = int(pseq[b]) if ragged else k.ne[1]
            kt = Tensor([hd, P, Hk, 1], k.nb, k.buf, k.offs)
            vt = Tensor([P, hd, Hv, 1], v.nb, v.buf, v.offs)
            ka = gather(kt, koff[b] if ragged else (b // (B // Bk)) * k.nb[3])[0]      # [Hk, P, hd]
            va = gather(vt, voff[b] if ragged else (b // (B // Bv)) * v.nb[3])[0]      # [Hv, hd, P]
            for h in range(H):
                kh, vh = ka[h // (H // Hk)], va[h // (H // Hv)]
                for t in range(n):
                    w = _fsum_last(kh * qa[b, h, t][None, :]).astype(np.float32)
                    if ba is not None:
                        w = w + ba[h, t, :P]
                    w = w * scale
                    if mflat is not None:
                        m0 = int(moff[b]) + t * P if ragged and moff is not None else (b * n * P if mask_per_seq else 0) + t * P
                        w = w + mflat[m0:m0 + P]
                    mx = w.max()
                    if not np.isfinite(mx):
                        assert mx == -np.inf, "a score is NaN or +inf"
                        dead[b, t, h] = True
                        continue
                    wmax[b, t, h] = np.abs(w[np.isfinite(w)]).max()
                    e = np.exp((w - mx).astype(np.float64)).astype(np.float32)
                    inv = f32(1.0 / math.fsum(e.astype(np.float64).tolist()))
                    p = e * inv
                    out[b, t, h] = _fsum_last(vh * p[None, :]).astype(np.float32)
                    pav[b, t, h] = _fsum_last(np.abs(vh * p[None, :]))
    return Result(out, wmax, pav, dead)


def ulps(a, b):
    """Elementwise distance in f32 steps between finite arrays (monotone integer mapping of the bit patterns)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def large_ratio(got, ref):
    """|got - ref| / (2^-24 (1 + max|w|) sum p|v|) per element of the live rows; the "large" bar holds it to C_LARGE."""
    live = ~ref.dead
    bound = 2.0 ** -24 * (1.0 + ref.wmax[live])[:, None] * ref.pav[live]
    return np.abs(got[live].astype(np.float64) - ref.out[live].astype(np.float64)) / bound


def check(name, got, ref, bar, verbose=True):
    """got [B, n, H, hd] against a Result at the bar; rows in ref.dead are the caller's.  -> (differing, worst ulp)."""
    live = ~ref.dead
    g, r = got[live], ref.out[live]
    assert np.isfinite(g).all(), f"{name}: a live row holds a non-finite value"
    d = ulps(g, r)
    nd, worst = int(np.count_nonzero(d)), int(d.max()) if d.size else 0
    line = f"{name}: {nd} of {d.size} differ, worst {worst} ulp"
    if bar == "large":
        ratio = float(large_ratio(got, ref).max())
        line += f", max|w| {ref.wmax.max():.2f}, bound ratio {ratio:.3f}"
    if verbose:
        print(line)
    if bar == "bits":
        assert nd == 0, line
    elif bar == "ulp1":
        assert worst <= 1 and nd <= 1e-3 * d.size, line
    elif bar == "large":
        assert ratio <= C_LARGE, line
    else:
        raise KeyError(bar)
    return nd, worst
