"""Kokoro's unrolled LSTM (tests/lstm.py = build_lstm_run node for node) with Q4_0 weight leaves.

A direction's eight matrices (W_ih and W_hh per gate) become Q4_0 leaves, as the quantize tool's Kokoro rule
leaves them in a file; the biases stay F32.  `mode` chooses the leaves (tests/q4_0_ref.py):
  "general"  quantize_row_q4_0's bytes, d with all its bits -- HIP fused against HIP unfused;
  "trimmed"  the same with every d trimmed to nine bits -- what HIP runs against the oracle;
  "twin"     the trimmed blocks' Q8_0 twins -- what the oracle runs;
  "twin-general"  the untrimmed blocks' Q8_0 twins: the product in Q8_0's order sumi * (d_w * d_x), which is not
             ggml's for Q4_0 -- the oracle runs it only to show that a test's inputs tell the two orders apart.

Random weights and states never tell them apart (|sumi| stays below 2^13, where both orders are exact up to one
rounding), so `parting_inputs` builds recurrent matrices and an initial state on which the first step's terms do.
"""
import numpy as np

import lstm
import q4_0_ref as q4
import ttship

F32, Q8_0, Q4_0 = ttship.F32, ttship.Q8_0, ttship.Q4_0
UN_TANH, UN_SIGMOID = lstm.UN_TANH, lstm.UN_SIGMOID


def weight_leaf(g, w, mode, q=None):
    """w [N][K] float32 -> a Q4_0 leaf (rows of K), or its (trimmed) twin's Q8_0 leaf.  q: the rows' Q4_0 bytes,
    where the caller built them itself."""
    N, K = w.shape
    if q is None:
        q = q4.quantize_row_q4_0(np.ascontiguousarray(w, dtype=np.float32))
    if mode == "general":
        return g.leaf(raw=q, typ=Q4_0, ne=[K, N])
    if mode == "twin-general":
        return g.leaf(raw=q4.twin_q8_0(q), typ=Q8_0, ne=[K, N])
    q = q4.trim_d(q)
    if mode == "trimmed":
        return g.leaf(raw=q, typ=Q4_0, ne=[K, N])
    assert mode == "twin"
    return g.leaf(raw=q4.twin_q8_0(q), typ=Q8_0, ne=[K, N])


def lstm_run(g, x, h0, c0, d, reversed_=False, mode="general"):
    """lstm.lstm_run with the eight matrices as Q4_0 leaves."""
    hd = d["w_hh"].shape[1]
    T = x.ne[1]
    ws, bs = [], []
    for gi in range(4):
        for key, bkey in (("w_ih", "b_ih"), ("w_hh", "b_hh")):
            q = d.get(key + "_q")  # Q4_0 bytes of all 4 * hd rows (parting_inputs), or None: quantize the floats
            if q is not None:
                q = np.ascontiguousarray(q.reshape(4 * hd, -1)[gi * hd:(gi + 1) * hd]).reshape(-1)
            ws.append(weight_leaf(g, d[key][gi * hd:(gi + 1) * hd], mode, q))
            bs.append(g.leaf(d[bkey][gi * hd:(gi + 1) * hd]))
    pre = []
    for gi in range(4):
        m = g.node("MUL_MAT", F32, [hd, T], [ws[2 * gi], x])
        pre.append(g.node("ADD", F32, [hd, T], [m, bs[2 * gi]]))
    h, c, outputs = h0, c0, None
    for index in range(T):
        i = T - 1 - index if reversed_ else index
        gates = []
        for gi, uop in enumerate((UN_SIGMOID, UN_SIGMOID, UN_TANH, UN_SIGMOID)):
            P = pre[gi]
            cur = g.view(P, [hd, 1, 1, 1], [4, P.nb[1], P.nb[2], P.nb[3]], offs=P.nb[1] * i)
            mm = g.node("MUL_MAT", F32, [hd, 1], [ws[2 * gi + 1], h])
            ab = g.node("ADD", F32, [hd, 1], [mm, bs[2 * gi + 1]])
            ap = g.node("ADD", F32, [hd, 1], [cur, ab])
            gates.append(g.node("UNARY", F32, [hd, 1], [ap], params=[uop]))
        I, Fg, G, O = gates
        fc = g.node("MUL", F32, [hd, 1], [Fg, c])
        ig = g.node("MUL", F32, [hd, 1], [I, G])
        c = g.node("ADD", F32, [hd, 1], [fc, ig])
        th = g.node("UNARY", F32, [hd, 1], [c], params=[UN_TANH])
        h = g.node("MUL", F32, [hd, 1], [th, O])
        if index == 0:
            outputs = h
        else:
            srcs = [h, outputs] if reversed_ else [outputs, h]
            outputs = g.node("CONCAT", F32, [hd, index + 1], srcs, params=[1])
    return outputs, h, c


def lstm_cell(g, x_arr, dirs, mode, h0=None, c0=None):
    """build_lstm for one cell (one direction or the paired chains)."""
    hd = dirs[0]["w_hh"].shape[1]
    x = g.leaf(x_arr)
    h0l = g.leaf(np.zeros(hd, np.float32) if h0 is None else h0)
    c0l = g.leaf(np.zeros(hd, np.float32) if c0 is None else c0)
    out, _, _ = lstm_run(g, x, h0l, c0l, dirs[0], False, mode)
    if len(dirs) == 1:
        return out
    rout, _, _ = lstm_run(g, x, h0l, c0l, dirs[1], True, mode)
    return g.node("CONCAT", F32, [2 * hd, x_arr.shape[0]], [out, rout], params=[0])


# seeds kept because the orders part on them in enough rows (tests/test_q4_0_cpu.py checks the condition)
PART_SEED = {(32, False): 4, (32, True): 2}
PART_HD = [32, 64, 96, 256, 512]


def parting_inputs(T, n_in, hd, bi):
    """x, dirs, h0, c0 like test_lstm_quant_gpu.inputs, but the first step's recurrent terms tell ggml's Q4_0 order
    ((float)sumi * d_w) * d_x from the Q8_0 / Q5_0 kernels' sumi * (d_w * d_x).  As in q4_0_ref._case: block b of h0 is a
    pattern p[b] of large quants (|q - 8| >= 4) times a random scale, and every W_hh row's block b holds p[b] but for
    four random elements, under a d with all its mantissa bits and a random sign; so |sumi| is near 127 / 8 * sum p^2
    = 19000 > 2^13, where the two orders differ in about one term in ten.  d_w near 0.003 and small W_ih, biases
    and c0 keep the gates' inputs within about +-1, where tanh and the sigmoid pass a last-bit difference on.
    dirs[i]["w_hh_q"] holds the Q4_0 bytes (lstm_run takes them as they are); "w_hh" their dequantized values."""
    rng = np.random.default_rng(PART_SEED.get((hd, bi), 0) * 100000 + 1000 * T + hd)
    nb = hd // q4.QK
    x = (rng.standard_normal((T, n_in)) * 0.5).astype(np.float32)
    dirs = lstm.lstm_weights(T + hd, n_in, hd, scale=0.05, bidirectional=bi)
    big = np.array([0, 1, 2, 3, 4, 12, 13, 14, 15], np.uint8)
    pat = rng.choice(big, size=(nb, q4.QK))
    for d in dirs:
        N = 4 * hd
        w = q4.rand_q4_0(rng, N, hd).reshape(N, nb, q4.BLOCK)
        dw = (0.003 * (0.5 + rng.random((N, nb))) * rng.choice([-1.0, 1.0], size=(N, nb))).astype(np.float16)
        w[:, :, 0:2] = dw.view(np.uint8).reshape(N, nb, 2)
        qs = np.broadcast_to(pat, (N, nb, q4.QK)).copy()
        for _ in range(4):
            j = rng.integers(0, q4.QK, size=(N, nb, 1))
            np.put_along_axis(qs, j, rng.integers(0, 16, size=(N, nb, 1), dtype=np.uint8), axis=2)
        w[:, :, 2:] = qs[:, :, :16] | (qs[:, :, 16:] << 4)
        d["w_hh_q"] = w.reshape(-1)
        d["w_hh"] = q4.dequantize(d["w_hh_q"], hd, N)
    scale = (0.02 + 0.04 * rng.random((nb, 1))).astype(np.float32)
    h0 = ((pat.astype(np.float32) - 8.0) * scale * rng.choice(np.array([-1.0, 1.0], np.float32), size=(nb, 1))).reshape(hd)
    c0 = (rng.standard_normal(hd) * 0.05).astype(np.float32)
    return x, dirs, h0.astype(np.float32), c0


def first_step_gate_inputs(x, d, h0, reversed_, order):
    """The four gates' inputs [4 * hd] at a direction's first step, every f32 operation in the node chain's order:
    (W_ih x_i + b_ih) + (W_hh h0 + b_hh).  order "q4_0": both products by R1 (ggml's Q4_0 order); "twin": the
    recurrent product in the Q8_0 twin's order, as the oracle computes it on the untrimmed twin."""
    import py_oracle
    hd = d["w_hh"].shape[1]
    i = x.shape[0] - 1 if reversed_ else 0
    cur = q4.vec_dot_q4_0_q8_0(q4.quantize_row_q4_0(d["w_ih"]), x[i:i + 1], 4 * hd)[0] + d["b_ih"]
    if order == "q4_0":
        mm = q4.vec_dot_q4_0_q8_0(d["w_hh_q"], h0[None], 4 * hd)[0]
    else:
        mm = py_oracle.gemv(Q8_0, q4.twin_q8_0(d["w_hh_q"]), h0[None], 4 * hd)[0]
    return (cur.astype(np.float32) + (mm + d["b_hh"]).astype(np.float32)).astype(np.float32), mm
