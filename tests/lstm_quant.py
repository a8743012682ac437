"""Kokoro's unrolled LSTM (tests/lstm.py = build_lstm_run node for node) with quantized weight leaves.

A direction's eight matrices (W_ih and W_hh per gate) become Q8_0 or Q5_0 leaves, as the quantize tool's
Kokoro rule leaves them in a file; the biases stay F32.  The CPU oracle has no Q5_0: it runs the Q8_0 twin
(tests/q5_0_ref.py), whose dot rounds the same operations in the same order, so `twin=True` builds the
oracle's graph of a Q5_0 case.
"""
import numpy as np

import lstm
import py_oracle
import q5_0_ref
import ttship

F32, F16, Q8_0, Q5_0 = ttship.F32, ttship.F16, ttship.Q8_0, ttship.Q5_0
UN_TANH, UN_SIGMOID = lstm.UN_TANH, lstm.UN_SIGMOID


def weight_leaf(g, w, wtype, twin=False):
    """w [N][K] float32 -> a leaf of wtype (rows of K)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    N, K = w.shape
    if wtype == F32:
        return g.leaf(w)
    if wtype == F16:
        return g.leaf(w.astype(np.float16), typ=F16)
    if wtype == Q8_0:
        return g.leaf(raw=py_oracle.quantize(Q8_0, w), typ=Q8_0, ne=[K, N])
    assert wtype == Q5_0
    q = q5_0_ref.quantize_row_q5_0(w)
    if twin:
        return g.leaf(raw=q5_0_ref.twin_q8_0(q), typ=Q8_0, ne=[K, N])
    return g.leaf(raw=q, typ=Q5_0, ne=[K, N])


def lstm_run(g, x, h0, c0, d, reversed_=False, wtype=Q8_0, twin=False):
    """lstm.lstm_run with the eight matrices as leaves of wtype."""
    hd = d["w_hh"].shape[1]
    T = x.ne[1]
    ws, bs = [], []
    for gi in range(4):
        for key, bkey in (("w_ih", "b_ih"), ("w_hh", "b_hh")):
            ws.append(weight_leaf(g, d[key][gi * hd:(gi + 1) * hd], wtype, twin))
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


def lstm_cell(g, x_arr, dirs, wtypes, twin=False, h0=None, c0=None):
    """build_lstm for one cell; wtypes: one weight type per direction."""
    hd = dirs[0]["w_hh"].shape[1]
    x = g.leaf(x_arr)
    h0l = g.leaf(np.zeros(hd, np.float32) if h0 is None else h0)
    c0l = g.leaf(np.zeros(hd, np.float32) if c0 is None else c0)
    out, _, _ = lstm_run(g, x, h0l, c0l, dirs[0], False, wtypes[0], twin)
    if len(dirs) == 1:
        return out
    rout, _, _ = lstm_run(g, x, h0l, c0l, dirs[1], True, wtypes[1], twin)
    return g.node("CONCAT", F32, [2 * hd, x_arr.shape[0]], [out, rout], params=[0])
