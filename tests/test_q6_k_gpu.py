"""Q6_K weights on the HIP backend, every comparison bit for bit against tests/q6_k_ref.py (ggml_vec_dot_q6_K_q8_K's
generic order, dequantize_row_q6_K and quantize_row_q6_K_ref restated in numpy): the GEMV of up to 8 columns, the
many-column product, graphs whose fused plans must equal their unfused ones and numpy, GET_ROWS, the device
quantizer and tool, and Parler, Orpheus and Dia runners on Q6_K weights.  tests/test_q6_k_cpu.py checks that the
reference's order can be told from another one on the product cases used here."""
import numpy as np
import pytest

import nodes as nd
import py_oracle
import q6_k_ref as q6
import ttship
import weights_pin as wp
from runner_gguf import ORPHEUS, SNAC
from test_gguf_cpu import DAC_TINY, TINY

pytestmark = pytest.mark.gpu
Q6, Q4K, F32, I32 = ttship.Q6_K, ttship.Q4_K, ttship.F32, ttship.I32
MIX = ttship.QUANT_MIX_Q4_K_M
MASKS = [0, ttship.FUSE_ALL]
TINY8 = dict(TINY, n_layers=8)
ORPHEUS8 = dict(ORPHEUS, n_layers=8)


def bits_equal(got, ref, what=""):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
        raise AssertionError(f"{what}: {np.sum(got != ref)} / {got.size} differ, max {np.nanmax(np.abs(got.astype(np.float64) - ref)):.3e}")


def run_gemv(hip, w, x, N, offset=0, wtype=Q6):
    """tts_hip_gemv on Q6_K bytes w; offset: the weight pointer's distance from a 256-B aligned address."""
    M, K = x.shape
    dw, dx, dy = hip.alloc(w.nbytes + 16), hip.alloc(x.nbytes), hip.alloc(4 * M * N)
    try:
        hip.set(dw + offset, w)
        hip.set(dx, x)
        assert ttship.lib().tts_hip_gemv(hip.ptr, wtype, dw + offset, dx, dy, K, N, M) == 0
        y = np.empty((M, N), dtype=np.float32)
        hip.get(y, dy)
        return y
    finally:
        for p in (dw, dx, dy):
            hip.free(p)


def test_supports_op_and_refusals(hip):
    """K = 128 is refused by supports_op for MUL_MAT and GET_ROWS; K = 256 is accepted; a ragged or odd-addressed
    direct product is refused before anything is launched."""
    import ctypes

    from test_abi_cpu import _t
    L = ttship.lib()
    L.tts_hip_supports_op.argtypes = [ctypes.POINTER(ttship.TtsTensor)]
    for K, want in ((128, 0), (256, 1), (384, 0), (1024, 1)):
        w = _t(Q6, [max(K // 256, 1) * 256, 4])
        w.ne[0] = K
        mm = _t(F32, [4, 2], op=ttship.OP["MUL_MAT"], srcs=(w, _t(F32, [K, 2])))
        gr = _t(F32, [K, 2], op=ttship.OP["GET_ROWS"], srcs=(w, _t(I32, [2])))
        assert L.tts_hip_supports_op(ctypes.byref(mm)) == want, K
        assert L.tts_hip_supports_op(ctypes.byref(gr)) == want, K
    dw = hip.alloc(4096)
    try:
        assert L.tts_hip_gemv(hip.ptr, Q6, dw, dw, dw, 128, 1, 1) != 0
        assert L.tts_hip_gemv(hip.ptr, Q6, dw + 1, dw, dw, 256, 1, 1) != 0
    finally:
        hip.free(dw)


@pytest.mark.parametrize("K,N", q6.GEMV_SHAPES)
@pytest.mark.parametrize("M", q6.GEMV_COLS)
def test_gemv(hip, K, N, M):
    w, x = q6.case(K, N, M)
    ref = q6.vec_dot_q6_K_q8_K(w, x, N)
    bits_equal(run_gemv(hip, w, x, N), ref, "aligned matrix")
    bits_equal(run_gemv(hip, w, x, N, offset=2), ref, "matrix at a 2-byte aligned address")


@pytest.mark.parametrize("K,N", q6.GEMM_SHAPES)
@pytest.mark.parametrize("M", q6.GEMM_COLS)
def test_many_columns(hip, K, N, M):
    w, x = q6.case(K, N, M)
    ref = q6.vec_dot_q6_K_q8_K(w, x, N)
    bits_equal(run_gemv(hip, w, x, N), ref, "aligned matrix")
    if M in (9, 33):
        bits_equal(run_gemv(hip, w, x, N, offset=2), ref, "matrix at a 2-byte aligned address")


def test_wide_and_tall(hip):
    """K = 8192 (the 16-column tile just fits LDS), K = 16384 (it does not: 8-column tiles) and N = 5000 (row groups
    beyond the grid)."""
    for K, N, M in ((8192, 9, 12), (16384, 9, 12), (256, 5000, 3)):
        w, x = q6.case(K, N, M)
        bits_equal(run_gemv(hip, w, x, N), q6.vec_dot_q6_K_q8_K(w, x, N), f"K {K} N {N} M {M}")


# ---- graph level ----
def rnd(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def run_hip_graph(hip, g, mask):
    hip.set_option(ttship.OPT["FUSION"], mask)
    try:
        g.run_hip(hip)
    finally:
        hip.set_option(ttship.OPT["FUSION"], ttship.FUSE_ALL)


def q4k_bytes(seed, N, K):
    return py_oracle.quantize(Q4K, rnd(seed, N, K, scale=0.05))


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("M", [1, 2, 8, 12])
def test_graph_layer_norm_into_mul_mat(hip, mask, M):
    """The oracle computes the LayerNorm chain, numpy the product of its output."""
    K, N = 512, 97
    w = q6.rand_q6_K(np.random.default_rng(M), N, K)
    x, gam, bet = rnd(1, M, K) + 0.25, rnd(2, K) * 0.1 + 1.0, rnd(3, K) * 0.02

    def chain(g):
        n = g.node("NORM", F32, [K, M], [g.leaf(x)], fparams={0: 1e-5})
        n = g.node("MUL", F32, [K, M], [n, g.leaf(gam)])
        return g.node("ADD", F32, [K, M], [n, g.leaf(bet)])
    g1, g2 = nd.Graph(), nd.Graph()
    n1 = chain(g1)
    y1 = g1.node("MUL_MAT", F32, [N, M], [g1.leaf(raw=w, typ=Q6, ne=[K, N]), n1])
    n2 = chain(g2)
    run_hip_graph(hip, g1, mask)
    g2.run_oracle()
    ln = g2.node_array(n2).reshape(M, K)
    bits_equal(g1.node_array(n1).reshape(M, K), ln, f"LayerNorm output, fusion mask {mask}")
    bits_equal(g1.node_array(y1).reshape(M, N), q6.vec_dot_q6_K_q8_K(w, ln, N), f"product, fusion mask {mask}")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("M", [1, 2, 12])
def test_graph_rms_norm_swiglu_mlp_mixed(hip, mask, M):
    """RMS_NORM * gamma -> silu(gate x) * (up x) -> down with gate / up in Q4_K and down in Q6_K: the oracle computes
    everything up to the down product's input, numpy the down product."""
    D, F = 512, 1024
    wg, wu = q4k_bytes(10, F, D), q4k_bytes(11, F, D)
    wd = q6.rand_q6_K(np.random.default_rng(12), D, F)
    x, gam = rnd(6, M, D), rnd(7, D) * 0.1 + 1.0

    def build(g, with_down):
        h = g.node("RMS_NORM", F32, [D, M], [g.leaf(x)], fparams={0: 1e-5})
        h = g.node("MUL", F32, [D, M], [h, g.leaf(gam)])
        gate = g.node("MUL_MAT", F32, [F, M], [g.leaf(raw=wg, typ=Q4K, ne=[D, F]), h])
        silu = g.node("UNARY", F32, [F, M], [gate], params=[ttship.UNARY["SILU"]])
        up = g.node("MUL_MAT", F32, [F, M], [g.leaf(raw=wu, typ=Q4K, ne=[D, F]), h])
        e = g.node("MUL", F32, [F, M], [silu, up])
        return e, (g.node("MUL_MAT", F32, [D, M], [g.leaf(raw=wd, typ=Q6, ne=[F, D]), e]) if with_down else None)
    g1, g2 = nd.Graph(), nd.Graph()
    e1, y1 = build(g1, True)
    e2, _ = build(g2, False)
    run_hip_graph(hip, g1, mask)
    g2.run_oracle()
    e = g2.node_array(e2).reshape(M, F)
    bits_equal(g1.node_array(e1).reshape(M, F), e, f"down product's input, fusion mask {mask}")
    bits_equal(g1.node_array(y1).reshape(M, D), q6.vec_dot_q6_K_q8_K(wd, e, D), f"down product, fusion mask {mask}")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("K,N,M", [(256, 41, 1), (1024, 130, 3), (512, 64, 20)])
def test_graph_mul_mat_residual(hip, mask, K, N, M):
    w, x = q6.case(K, N, M, seed=1)
    res = rnd(9, M, N)
    g = nd.Graph()
    y = g.node("MUL_MAT", F32, [N, M], [g.leaf(raw=w, typ=Q6, ne=[K, N]), g.leaf(x)])
    out = g.node("ADD", F32, [N, M], [y, g.leaf(res)])
    run_hip_graph(hip, g, mask)
    bits_equal(g.node_array(out).reshape(M, N), (q6.vec_dot_q6_K_q8_K(w, x, N) + res).astype(np.float32), f"fusion mask {mask}")


@pytest.mark.parametrize("mask", MASKS)
def test_graph_qkv_group_with_q6_K_v(hip, mask):
    """A decoder layer's K, V, Q products of one activation in Parler's order, K and Q in Q4_K and V in Q6_K, K stored
    into a row of its cache and V into a column of the transposed cache (the KV-store epilogues)."""
    K = N = 256
    ctx, pos = 8, 3
    wk, wq = q4k_bytes(20, N, K), q4k_bytes(21, N, K)
    wv = q6.rand_q6_K(np.random.default_rng(22), N, K)
    x = rnd(23, 1, K)
    g = nd.Graph()
    xl = g.node("SCALE", F32, [K, 1], [g.leaf(x)], fparams={0: 0.5})
    kcache, vcache = g.leaf(np.zeros((ctx, N), np.float32)), g.leaf(np.zeros((N, ctx), np.float32))
    k = g.node("MUL_MAT", F32, [N, 1], [g.leaf(raw=wk, typ=Q4K, ne=[K, N]), xl])
    kd = g.view(kcache, [N, 1, 1, 1], [4, 4 * N, 4 * N, 4 * N], offs=4 * N * pos)
    kcp = g.node("CPY", F32, [N, 1], [k, kd], on=(kd, 0))
    v = g.node("MUL_MAT", F32, [N, 1], [g.leaf(raw=wv, typ=Q6, ne=[K, N]), xl])
    vr = g.view(v, [N, 1, 1, 1], [4, 4 * N, 4 * N, 4 * N], op="RESHAPE")
    vc = g.node("CONT", F32, [1, N], [g.transpose(vr, op="TRANSPOSE")])
    vd = g.view(vcache, [1, N, 1, 1], [4, 4 * ctx, 4 * ctx * N, 4 * ctx * N], offs=4 * pos)
    vcp = g.node("CPY", F32, [1, N], [vc, vd], nb=[vd.nb[i] for i in range(4)], on=(vd, 0))
    q = g.node("MUL_MAT", F32, [N, 1], [g.leaf(raw=wq, typ=Q4K, ne=[K, N]), xl])
    qs = g.node("SCALE", F32, [N, 1], [q], fparams={0: 0.125})
    run_hip_graph(hip, g, mask)
    xs = (x * np.float32(0.5)).astype(np.float32)
    bits_equal(g.node_array(kcache).reshape(ctx, N)[pos], py_oracle.gemv(Q4K, wk, xs, N)[0], f"K cache row, mask {mask}")
    bits_equal(g.node_array(vcache).reshape(N, ctx)[:, pos], q6.vec_dot_q6_K_q8_K(wv, xs, N)[0], f"V cache column, mask {mask}")
    bits_equal(g.node_array(qs).reshape(N), (py_oracle.gemv(Q4K, wq, xs, N)[0] * np.float32(0.125)).astype(np.float32), f"Q, mask {mask}")
    assert not g.node_array(kcache).reshape(ctx, N)[[0, 1, 2, 4, 5, 6, 7]].any()
    assert kcp is not None and vcp is not None


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("K", [256, 1024])
def test_graph_get_rows(hip, mask, K):
    """GET_ROWS from a Q6_K table with repeated and out-of-order ids (R = 51: odd, so every other row of the K = 256
    table is 2-byte aligned only), alone and as the terms of an embedding sum."""
    R = 51
    rng = np.random.default_rng(K)
    t1, t2 = q6.rand_q6_K(rng, R, K), q6.rand_q6_K(rng, R, K)
    i1 = np.array([0, 50, 7, 7, 31, 16, 1], np.int32)
    i2 = np.array([5, 4, 3, 2, 1, 0, 50], np.int32)
    g = nd.Graph()
    a = g.node("GET_ROWS", F32, [K, 7], [g.leaf(raw=t1, typ=Q6, ne=[K, R]), g.leaf(i1, typ=I32)])
    b = g.node("GET_ROWS", F32, [K, 7], [g.leaf(raw=t1, typ=Q6, ne=[K, R]), g.leaf(i2, typ=I32)])
    c = g.node("GET_ROWS", F32, [K, 7], [g.leaf(raw=t2, typ=Q6, ne=[K, R]), g.leaf(i1, typ=I32)])
    s = g.node("ADD", F32, [K, 7], [b, c])
    run_hip_graph(hip, g, mask)
    d1, d2 = q6.dequantize(t1, K, R), q6.dequantize(t2, K, R)
    bits_equal(g.node_array(a).reshape(7, K), d1[i1], f"rows, mask {mask}")
    bits_equal(g.node_array(s).reshape(7, K), (d1[i2] + d2[i1]).astype(np.float32), f"sum of rows, mask {mask}")


# ---- device quantizer ----
def quantizer_rows(K=256, seed=0):
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal(K), rng.standard_normal(K) * 300.0, rng.standard_normal(K) * 1e-6, np.zeros(K),
            np.abs(rng.standard_normal(K)), -np.abs(rng.standard_normal(K)), np.full(K, 0.37), np.full(K, -0.37), np.full(K, 1e-20)]
    z = rng.standard_normal(K)
    z[32:48] = 0.0  # a zero sub-block inside a live block
    rows.append(z)
    o = rng.standard_normal(K) * 0.01
    o[77] = 3.0e4   # one huge outlier: every other sub-block's scale code rounds to 0
    rows.append(o)
    for first in (1.0, -1.0):  # the largest magnitude at both signs: the first one met wins
        t = rng.uniform(-0.9, 0.9, K)
        t[3::16], t[12::16] = first * 2.5, -first * 2.5
        rows.append(t)
    return np.asarray(rows, dtype=np.float32)


def test_device_quantizer_bytes(hip):
    x = np.concatenate([quantizer_rows(), rnd(11, 40, 256) * 0.02, rnd(12, 3, 768)[:, :256]])
    got, want = hip.quantize(Q6, x), q6.quantize_row_q6_K(x)
    assert got.shape == want.shape == (x.shape[0] * 210,)
    bad = np.flatnonzero((got != want).reshape(-1, 210).any(axis=1))
    assert bad.size == 0, f"blocks {bad[:8]} differ: {got.reshape(-1, 210)[bad[0]]} vs {want.reshape(-1, 210)[bad[0]]}"
    x3 = rnd(13, 5, 768)  # three blocks per row: odd rows start 2-byte aligned only
    assert np.array_equal(hip.quantize(Q6, x3), q6.quantize_row_q6_K(x3))
    assert not hip.quantize(Q6, np.zeros((1, 256), np.float32)).any()


def host_rows(ty, x):
    return q6.quantize_row_q6_K(x) if ty == Q6 else py_oracle.quantize(ty, x)


@pytest.fixture(scope="module")
def files(hip, tmp_path_factory):
    """Tiny 8-layer Parler and Orpheus files in F32 and their Q4_K_M-style mixes (heads quantized) written by the device tool."""
    d = tmp_path_factory.mktemp("q6_k")
    p32, pmix, o32, omix = d / "parler-f32.gguf", d / "parler-mix.gguf", d / "orpheus-f32.gguf", d / "orpheus-mix.gguf"
    ttship.write_parler_synthetic_gguf(p32, ttship.parler_config(weight_type=F32, head_type=F32, **TINY8), ttship.dac_config(**DAC_TINY))
    ttship.write_orpheus_synthetic_gguf(o32, ttship.orpheus_config(**dict(ORPHEUS8, weight_type=F32)), ttship.snac_config(**SNAC))
    p = ttship.quantize_params(Q4K, mix=MIX, quantize_output_heads=1)
    ttship.quantize_gguf(p32, pmix, p, backend=hip)
    ttship.quantize_gguf(o32, omix, p, backend=hip)
    return d, p32, pmix, o32, omix


def test_device_quantize_tool_bytes(hip, files):
    d, p32, pmix, o32, omix = files
    p = ttship.quantize_params(Q4K, mix=MIX, quantize_output_heads=1)
    for src, dev in ((p32, pmix), (o32, omix)):
        ref = d / (dev.name + ".host")
        ttship.quantize_gguf(src, ref, p, rows_fn=host_rows)
        assert dev.read_bytes() == ref.read_bytes(), dev.name
    plain, ref = d / "parler-q6k.gguf", d / "parler-q6k.host"
    ttship.quantize_gguf(p32, plain, ttship.quantize_params(Q6), backend=hip)  # a plain Q6_K type: every quantized tensor
    ttship.quantize_gguf(p32, ref, ttship.quantize_params(Q6), rows_fn=host_rows)
    assert plain.read_bytes() == ref.read_bytes()
    with ttship.Gguf(plain) as g:
        assert g.tensor_type("decoder.layers.1.fc1.weight") == Q6 and g.get("general.quantization_type") == Q6


# ---- runners ----
def parler_prompt(batch):
    return (np.arange(5 * batch, dtype=np.int32).reshape(batch, 5) * 53) % TINY["prompt_vocab"]


def parler_step(hip, path, batch, mask):
    """(first decode logits, final LayerNorm output [batch][H], generated tokens) of the mix file's runner under a fusion mask."""
    hip.set_option(ttship.OPT["FUSION"], mask)
    try:
        with ttship.Gguf(path) as g:
            # debug_no_reuse: every node keeps its own memory, so the final LayerNorm's output outlives the step
            cfg = ttship.parler_config_from_gguf(g, max_ctx=TINY["max_ctx"], batch=batch, debug_no_reuse=1)
            assert (cfg.weight_type, cfg.head_type) == (Q4K, Q6)
            assert g.tensor_type("decoder.layers.3.self_attn.v_proj.weight") == Q6 and g.tensor_type("decoder.layers.2.fc2.weight") == Q4K
            head = [g.tensor_bytes(f"decoder.lm_heads.{h}.weight.head") for h in range(cfg.n_output_heads)]
            run = ttship.Parler(hip.iface(), cfg, gguf=g)
        try:
            run.prefill(parler_prompt(batch))
            logits = run.decode(np.full((batch, cfg.n_output_heads), 1025, dtype=np.int32))
            # the step graph's last ADD of [H, batch] is the final LayerNorm's output, the input of the Q6_K heads
            H, act = cfg.hidden_size, None
            for i in range(run.last_graph_nodes() - 1, -1, -1):
                op, ty, ne, data = run.node(i)
                if op == "ADD" and ty == F32 and ne[0] == H and data is not None and data.size == H * batch:
                    act = data.reshape(batch, H)
                    break
            toks = run.generate(6)
        finally:
            run.close()
    finally:
        hip.set_option(ttship.OPT["FUSION"], ttship.FUSE_ALL)
    return logits, act, toks, head, cfg


@pytest.mark.parametrize("batch", [1, 3, 12])  # 12 columns: the decode step's products take the 16-column tile
def test_parler_from_mix_file(hip, files, batch):
    _, _, pmix, _, _ = files
    fused = parler_step(hip, pmix, batch, ttship.FUSE_ALL)
    plain = parler_step(hip, pmix, batch, 0)
    assert np.all(np.isfinite(fused[0]))
    bits_equal(fused[0], plain[0], "decode logits, FUSE_ALL against fusion mask 0")
    assert np.array_equal(fused[2], plain[2]) and fused[2].min() >= 0
    # in situ: the activation entering the Q6_K head products and their outputs, against numpy
    for logits, act, _, head, cfg in (fused, plain):
        assert act is not None
        V = cfg.output_vocab
        lg = np.asarray(logits).reshape(batch, cfg.n_output_heads, V)
        for h in range(cfg.n_output_heads):
            bits_equal(lg[:, h], q6.vec_dot_q6_K_q8_K(head[h], act, V), f"head {h} in the step graph")


def orpheus_tokens(batch, n, step=0):
    return ((np.arange(batch * n, dtype=np.int32).reshape(batch, n) * 37 + 11 * step) % ORPHEUS["vocab_size"]).astype(np.int32)


@pytest.mark.parametrize("batch", [1, 2])
def test_orpheus_from_mix_file_with_q6_K_head(hip, files, batch):
    _, _, _, _, omix = files
    out = []
    for mask in (ttship.FUSE_ALL, 0):
        hip.set_option(ttship.OPT["FUSION"], mask)
        try:
            with ttship.Gguf(omix) as g:
                assert g.tensor_type("orpheus.lm_head") == Q6 and g.tensor_type("orpheus.layers.3.mlp.down_proj") == Q6
                assert g.tensor_type("orpheus.layers.3.self_attn.v_proj") == Q6 and g.tensor_type("orpheus.layers.3.self_attn.q_proj") == Q4K
                assert g.tensor_type("orpheus.layers.2.mlp.down_proj") == Q4K
                cfg = ttship.orpheus_config_from_gguf(g, max_ctx=ORPHEUS["max_ctx"], batch=batch, arena_bytes=ORPHEUS["arena_bytes"])
                run = ttship.Orpheus(hip.iface(), cfg, gguf=g)
            try:
                lg = [run.prefill(orpheus_tokens(batch, 6))]
                for s in range(2):
                    lg.append(run.decode(orpheus_tokens(batch, 1, s + 1)))
                toks = run.generate(lg[-1].reshape(batch, -1).argmax(axis=1).astype(np.int32), 5)
                out.append((np.concatenate([np.asarray(a).reshape(-1) for a in lg]), np.asarray(toks)))
            finally:
                run.close()
        finally:
            hip.set_option(ttship.OPT["FUSION"], ttship.FUSE_ALL)
    assert np.all(np.isfinite(out[0][0]))
    bits_equal(out[0][0], out[1][0], "logits, FUSE_ALL against fusion mask 0")
    assert np.array_equal(out[0][1], out[1][1])


DIA_Q6 = dict(wp.DIA_TINY, encoder_hidden_size=256, decoder_hidden_size=256, encoder_attn_heads=8, decoder_attn_heads=8,
              encoder_ffn_size=512, decoder_ffn_size=512, weight_type=Q6)


def test_dia_synthetic_q6_K(hip):
    """Synthetic Dia on Q6_K matrices and embeddings at the CFG pair: fused equals unfused."""
    text = np.frombuffer(b"\x01 The birch canoe slid on the smooth planks.", dtype=np.uint8).astype(np.int32)[:32]
    runs = []
    for mask in (ttship.FUSE_ALL, 0):
        hip.set_option(ttship.OPT["FUSION"], mask)
        try:
            r = ttship.Dia(hip.iface(), ttship.dia_config(**DIA_Q6))
            try:
                assert any(ty == Q6 for ty, _, _ in r.weights_raw().values())
                audio, seq = np.full(9, 1026, dtype=np.int32), []
                for s in range(3):
                    lg = r.prefill(text, audio) if s == 0 else r.decode(audio)
                    assert np.all(np.isfinite(lg))
                    audio = lg.argmax(axis=1).astype(np.int32)
                    seq.append(np.asarray(lg).reshape(-1))
                runs.append(np.concatenate(seq))
            finally:
                r.close()
        finally:
            hip.set_option(ttship.OPT["FUSION"], ttship.FUSE_ALL)
    bits_equal(runs[0], runs[1], "logits, FUSE_ALL against fusion mask 0")


def test_parler_and_orpheus_synthetic_q6_K(hip):
    """weight_type = Q6_K for the synthetic runners: they build, run and repeat themselves."""
    toks = []
    for _ in range(2):
        r = ttship.Parler(hip.iface(), ttship.parler_config(weight_type=Q6, head_type=F32, batch=2, **TINY))
        try:
            r.prefill(parler_prompt(2))
            toks.append(r.generate(4))
        finally:
            r.close()
    assert np.array_equal(toks[0], toks[1]) and toks[0].min() >= 0
    o = ttship.Orpheus(hip.iface(), ttship.orpheus_config(**dict(ORPHEUS, weight_type=Q6)))
    try:
        assert np.all(np.isfinite(o.prefill(orpheus_tokens(1, 6))))
    finally:
        o.close()
