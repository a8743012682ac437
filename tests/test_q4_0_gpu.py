"""Q4_0 weights on the HIP backend, every comparison bit for bit, against the two references of tests/q4_0_ref.py:
R1, ggml_vec_dot_q4_0_q8_0 restated in numpy (general d; the only one that sees the ((float)sumi * d_w) * d_x
order), for every kernel route -- GEMV general and slab, with and without the in-kernel quantize prologue, the
matrix-core GEMM direct and staged -- and for the graphs that end in a product; R2, the unchanged CPU oracle on the
Q8_0 twin of weights whose d is trimmed to nine bits, for whole graphs and the Parler runner from a file.  The
kernel cases' and the residual graph's inputs are built so that the Q4_0 order and the twin's differ on them
(tests/test_q4_0_cpu.py); the LayerNorm graph's are not, and it says so."""
import numpy as np
import pytest

import nodes as nd
import py_oracle
import q4_0_ref as q4
import ttship
import weights_pin as wp
from test_gguf_cpu import DAC_TINY, TINY

pytestmark = pytest.mark.gpu
Q4, Q8, F32 = ttship.Q4_0, ttship.Q8_0, ttship.F32


def bits_equal(got, ref, what=""):
    if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
        raise AssertionError(f"{what}: {np.sum(got != ref)} / {got.size} differ, max {np.nanmax(np.abs(got.astype(np.float64) - ref)):.3e}")


def run_gemv(hip, w, x, N, offset=0):
    """tts_hip_gemv on Q4_0 bytes w; offset: the weight pointer's distance from a 256-B aligned address."""
    M, K = x.shape
    dw, dx, dy = hip.alloc(w.nbytes + 16), hip.alloc(x.nbytes), hip.alloc(4 * M * N)
    try:
        hip.set(dw + offset, w)
        hip.set(dx, x)
        assert ttship.lib().tts_hip_gemv(hip.ptr, Q4, dw + offset, dx, dy, K, N, M) == 0
        y = np.empty((M, N), dtype=np.float32)
        hip.get(y, dy)
        return y
    finally:
        for p in (dw, dx, dy):
            hip.free(p)


class options:
    """with options(hip, GEMV_Q40_SLAB=0, ...): backend options set, then back to their defaults."""
    DEFAULTS = {"GEMM_Q4_0_STAGED": 2}

    def __init__(self, hip, **kv):
        self.hip, self.kv = hip, kv

    def __enter__(self):
        for k, v in self.kv.items():
            assert ttship.lib().tts_hip_set_option(self.hip.ptr, ttship.OPT[k], v) == 0, k

    def __exit__(self, *a):
        for k in self.kv:
            ttship.lib().tts_hip_set_option(self.hip.ptr, ttship.OPT[k], self.DEFAULTS.get(k, 1))


def test_ragged_rows_are_refused(hip):
    """Q4_0 rows whose length is no multiple of 32 are refused before anything is launched."""
    dw = hip.alloc(4096)
    try:
        assert ttship.lib().tts_hip_gemv(hip.ptr, Q4, dw, dw, dw, 48, 1, 1) != 0
    finally:
        hip.free(dw)


@pytest.mark.parametrize("K,N", q4.GEMV_SHAPES)
@pytest.mark.parametrize("M", q4.GEMV_COLS)
def test_gemv(hip, K, N, M):
    w, x = q4.gemv_case(K, N, M)
    ref = q4.vec_dot_q4_0_q8_0(w, x, N)  # R1
    for slab in (1, 0):
        for pro in (1, 0):
            with options(hip, GEMV_Q40_SLAB=slab, GEMV_Q80_PRO=pro):
                bits_equal(run_gemv(hip, w, x, N), ref, f"slab {slab} prologue {pro}")
    for pro in (1, 0):  # a 2-B aligned weight pointer: the general kernel whatever the slab option says
        with options(hip, GEMV_Q80_PRO=pro):
            bits_equal(run_gemv(hip, w, x, N, offset=2), ref, f"offset 2 prologue {pro}")


@pytest.mark.parametrize("rw", [1, 2, 32])
def test_gemv_slab_rows_per_workgroup(hip, rw):
    K, N, M = 1024, 70, 3  # 70 rows: the last workgroup's slab is short at every RW > 1
    w, x = q4.gemv_case(K, N, M)
    ref = q4.vec_dot_q4_0_q8_0(w, x, N)
    assert ttship.lib().tts_hip_set_option(hip.ptr, ttship.OPT["GEMV_Q40_RW"], rw) == 0
    try:
        bits_equal(run_gemv(hip, w, x, N), ref, f"RW {rw}")
    finally:
        ttship.lib().tts_hip_set_option(hip.ptr, ttship.OPT["GEMV_Q40_RW"], 0)


@pytest.mark.parametrize("K,N", q4.GEMM_SHAPES)
@pytest.mark.parametrize("M", q4.GEMM_COLS)
def test_gemm(hip, K, N, M):
    w, x = q4.gemm_case(K, N, M)
    ref = q4.vec_dot_q4_0_q8_0(w, x, N)  # R1
    for staged in (2, 1, 0):  # 64 x 128 tiles, 64 x 64 tiles, the direct-load kernel (the only one when K % 256 != 0)
        with options(hip, GEMM_Q4_0_STAGED=staged):
            bits_equal(run_gemv(hip, w, x, N), ref, f"matrix-core GEMM, staged {staged}")
    bits_equal(run_gemv(hip, w, x, N, offset=2), ref, "matrix-core GEMM, 2-B aligned rows: direct loads")
    with options(hip, GEMM_Q4_0=0):
        bits_equal(run_gemv(hip, w, x, N), ref, "GEMV per 8 columns")


# ---- graph level ----
def rnd(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


MASKS = [0, ttship.FUSE_ALL]


def run_hip_graph(hip, g, mask):
    hip.set_option(ttship.OPT["FUSION"], mask)
    try:
        g.run_hip(hip)
    finally:
        hip.set_option(ttship.OPT["FUSION"], ttship.FUSE_ALL)


def run_graphs(hip, build, mask):
    """R2: the same graph built twice, on trimmed Q4_0 leaves (HIP) and on their Q8_0 twins (oracle)."""
    g1, g2 = nd.Graph(), nd.Graph()
    o1 = build(g1, lambda w, K, N: g1.leaf(raw=w, typ=Q4, ne=[K, N]))
    o2 = build(g2, lambda w, K, N: g2.leaf(raw=q4.twin_q8_0(w), typ=Q8, ne=[K, N]))
    run_hip_graph(hip, g1, mask)
    g2.run_oracle()
    for k, (a, b) in enumerate(zip(o1, o2)):
        bits_equal(g1.node_array(a), g2.node_array(b), f"output {k}, fusion mask {mask}")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("M", [1, 2, 8, 12])
def test_graph_layer_norm_into_mul_mat(hip, mask, M):
    """General d: the oracle computes the LayerNorm chain, R1 the product of its output.  Random weights on a
    normalized activation: |sumi| stays below 2^13, where both association orders give the same bits, so this case
    does not see the order.  It checks the prologue's LayerNorm and quantization and the route's plumbing; the
    order is pinned by test_gemv and test_gemm, whose term code (BlkQ4_0::term) these instantiations share."""
    K, N = 512, 96
    w = q4.rand_q4_0(np.random.default_rng(M), N, K)
    x, gam, bet = rnd(1, M, K) + 0.25, rnd(2, K) * 0.1 + 1.0, rnd(3, K) * 0.02

    def chain(g):
        n = g.node("NORM", F32, [K, M], [g.leaf(x)], fparams={0: 1e-5})
        n = g.node("MUL", F32, [K, M], [n, g.leaf(gam)])
        return g.node("ADD", F32, [K, M], [n, g.leaf(bet)])
    g1, g2 = nd.Graph(), nd.Graph()
    n1 = chain(g1)
    y1 = g1.node("MUL_MAT", F32, [N, M], [g1.leaf(raw=w, typ=Q4, ne=[K, N]), n1])
    n2 = chain(g2)
    run_hip_graph(hip, g1, mask)
    g2.run_oracle()
    ln = g2.node_array(n2).reshape(M, K)
    bits_equal(g1.node_array(n1).reshape(M, K), ln, f"LayerNorm output, fusion mask {mask}")
    bits_equal(g1.node_array(y1).reshape(M, N), q4.vec_dot_q4_0_q8_0(w, ln, N), f"product, fusion mask {mask}")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("K,N,M", q4.RESIDUAL_SHAPES)
def test_graph_mul_mat_residual(hip, mask, K, N, M):
    """General d: R1 computes the product, numpy the final f32 add.  Weights and activations on which the two
    association orders part (q4_0_ref.residual_case; tests/test_q4_0_cpu.py checks that they do)."""
    w, x = q4.residual_case(K, N, M)
    res = rnd(9, M, N)
    g = nd.Graph()
    y = g.node("MUL_MAT", F32, [N, M], [g.leaf(raw=w, typ=Q4, ne=[K, N]), g.leaf(x)])
    out = g.node("ADD", F32, [N, M], [y, g.leaf(res)])
    run_hip_graph(hip, g, mask)
    ref = (q4.vec_dot_q4_0_q8_0(w, x, N) + res).astype(np.float32)
    bits_equal(g.node_array(out).reshape(M, N), ref, f"fusion mask {mask}")


@pytest.mark.parametrize("mask", MASKS)
def test_graph_rms_norm_swiglu_mlp(hip, mask):
    """Dia's decoder MLP at its shape: RMS_NORM * gamma -> silu(gate x) * (up x) -> down, 2048 / 8192, 2 columns (R2)."""
    D, F, M = 2048, 8192, 2
    rng = np.random.default_rng(5)
    wg, wu, wd = (q4.trim_d(q4.rand_q4_0(rng, n, k)) for n, k in ((F, D), (F, D), (D, F)))
    x, gam = rnd(6, M, D), rnd(7, D) * 0.1 + 1.0

    def build(g, wleaf):
        h = g.node("RMS_NORM", F32, [D, M], [g.leaf(x)], fparams={0: 1e-5})
        h = g.node("MUL", F32, [D, M], [h, g.leaf(gam)])
        gate = g.node("MUL_MAT", F32, [F, M], [wleaf(wg, D, F), h])
        silu = g.node("UNARY", F32, [F, M], [gate], params=[ttship.UNARY["SILU"]])
        up = g.node("MUL_MAT", F32, [F, M], [wleaf(wu, D, F), h])
        e = g.node("MUL", F32, [F, M], [silu, up])
        return [e, g.node("MUL_MAT", F32, [D, M], [wleaf(wd, F, D), e])]
    run_graphs(hip, build, mask)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("K", [256, 1024])
def test_graph_get_rows(hip, mask, K):
    """GET_ROWS from a Q4_0 table alone, and as the terms of an embedding sum (ADD over two GET_ROWS) (R2; a
    dequantized element is one product, the same under either reference)."""
    R = 50
    rng = np.random.default_rng(K)
    t1, t2 = q4.trim_d(q4.rand_q4_0(rng, R, K)), q4.trim_d(q4.rand_q4_0(rng, R, K))
    i1 = np.array([0, 49, 7, 7, 31, 16, 1], np.int32)
    i2 = np.array([5, 4, 3, 2, 1, 0, 49], np.int32)

    def build(g, wleaf):
        a = g.node("GET_ROWS", F32, [K, 7], [wleaf(t1, K, R), g.leaf(i1, typ=ttship.I32)])
        b = g.node("GET_ROWS", F32, [K, 7], [wleaf(t1, K, R), g.leaf(i2, typ=ttship.I32)])
        c = g.node("GET_ROWS", F32, [K, 7], [wleaf(t2, K, R), g.leaf(i1, typ=ttship.I32)])
        return [a, g.node("ADD", F32, [K, 7], [b, c])]
    run_graphs(hip, build, mask)


# ---- device quantizer ----
def quantizer_rows(K=256, seed=0):
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal(K), rng.standard_normal(K) * 300.0, rng.standard_normal(K) * 1e-6, np.zeros(K),
            np.abs(rng.standard_normal(K)), -np.abs(rng.standard_normal(K)), np.full(K, 0.37), np.full(K, -0.37)]
    z = rng.standard_normal(K)
    z[:32] = 0.0  # a block of zeros inside a live row
    rows.append(z)
    for first in (1.0, -1.0):  # the largest magnitude at both signs: the first one met gives d its sign
        t = rng.uniform(-0.9, 0.9, K)
        t[3::32], t[20::32] = first * 2.5, -first * 2.5
        rows.append(t)
    p = rng.uniform(-1, 1, K)
    p[5::32] = 3.0   # largest magnitude positive: it lands on q = 0, and -3 would clip at 15
    p[6::32] = -2.999
    rows.append(p)
    n = rng.uniform(-1, 1, K)
    n[9::32] = -3.0  # largest magnitude negative
    n[11::32] = 2.999
    rows.append(n)
    for at in (0, 31):  # +max and -max at either end of the block
        for v in (3.5, -3.5):
            e = rng.uniform(-1, 1, K)
            e[at::32] = v
            rows.append(e)
    return np.asarray(rows, dtype=np.float32)


def test_device_quantizer_bytes(hip):
    x = np.concatenate([quantizer_rows(), rnd(11, 40, 256) * 0.02])
    got = hip.quantize(Q4, x)
    want = q4.quantize_row_q4_0(x)
    assert got.shape == want.shape == (x.shape[0] * 256 // 32 * 18,)
    bad = np.flatnonzero((got != want).reshape(-1, 18).any(axis=1))
    assert bad.size == 0, f"blocks {bad[:8]} differ: {got.reshape(-1, 18)[bad[0]]} vs {want.reshape(-1, 18)[bad[0]]}"
    x96 = rnd(12, 3, 96)  # K % 256 != 0
    assert np.array_equal(hip.quantize(Q4, x96), q4.quantize_row_q4_0(x96))


@pytest.fixture(scope="module")
def files(hip, tmp_path_factory):
    """The TINY Parler file in F32, quantized to Q4_0 by the device tool, that file with every d trimmed (R2), and
    the trimmed file's Q8_0 twin."""
    d = tmp_path_factory.mktemp("q4_0")
    cfg32 = ttship.parler_config(weight_type=F32, head_type=F32, **TINY)
    src, dev, trim, twin = d / "parler-f32.gguf", d / "parler-q4_0.gguf", d / "parler-q4_0-trim.gguf", d / "parler-q4_0-twin.gguf"
    ttship.write_parler_synthetic_gguf(src, cfg32, ttship.dac_config(**DAC_TINY))
    ttship.quantize_gguf(src, dev, ttship.quantize_params(Q4), backend=hip)
    q4.trim_gguf(dev, trim)
    q4.twin_gguf(trim, twin)
    return d, src, dev, trim, twin


def test_device_quantize_tool_bytes(files):
    d, src, dev, _, _ = files
    ref = d / "parler-q4_0-host.gguf"
    ttship.quantize_gguf(src, ref, ttship.quantize_params(Q4), rows_fn=lambda ty, x: q4.quantize_row_q4_0(x))
    assert dev.read_bytes() == ref.read_bytes()


# ---- runners ----
def parler_prompt(batch):
    return (np.arange(5 * batch, dtype=np.int32).reshape(batch, 5) * 53) % TINY["prompt_vocab"]


@pytest.mark.parametrize("batch", [1, 3, 12])  # 12 columns: the decode step's products run the GEMM
def test_parler_from_q4_0_gguf(hip, files, batch):
    """R2: HIP on the trimmed Q4_0 file against the oracle on its twin."""
    _, _, _, trim, twin = files
    with ttship.Gguf(trim) as g, ttship.Gguf(twin) as t:
        assert g.get("general.quantization_type") == t.get("general.quantization_type") == Q4
        cg = ttship.parler_config_from_gguf(g, max_ctx=TINY["max_ctx"], batch=batch)
        ct = ttship.parler_config_from_gguf(t, max_ctx=TINY["max_ctx"], batch=batch)
        assert (cg.weight_type, ct.weight_type, cg.head_type) == (Q4, Q8, F32)
        assert g.tensor_type("decoder.embed_prompts") == F32 and g.tensor_type("decoder.lm_heads.0.weight.head") == F32
        run = ttship.Parler(hip.iface(), cg, gguf=g)
        ref = ttship.Parler(py_oracle.iface(8), ct, gguf=t)
    try:
        for r in (run, ref):
            r.prefill(parler_prompt(batch))
        tok = np.full((batch, 9), 1025, dtype=np.int32)
        bits_equal(run.decode(tok), ref.decode(tok), "decode logits")
        assert np.array_equal(run.generate(8), ref.generate(8))
    finally:
        run.close()
        ref.close()


@pytest.mark.parametrize("batch", [1, 3, 12])
def test_parler_untrimmed_file_fused_equals_unfused(hip, files, batch):
    """HIP against HIP: the untrimmed device-quantized file (general d) loads, and its first decode logits with
    every fusion on equal the same runner's with every fusion off."""
    _, _, dev, _, _ = files
    logits = []
    for mask in (ttship.FUSE_ALL, 0):
        hip.set_option(ttship.OPT["FUSION"], mask)
        try:
            with ttship.Gguf(dev) as g:
                cfg = ttship.parler_config_from_gguf(g, max_ctx=TINY["max_ctx"], batch=batch)
                assert cfg.weight_type == Q4
                run = ttship.Parler(hip.iface(), cfg, gguf=g)
            try:
                run.prefill(parler_prompt(batch))
                logits.append(run.decode(np.full((batch, 9), 1025, dtype=np.int32)))
            finally:
                run.close()
        finally:
            hip.set_option(ttship.OPT["FUSION"], ttship.FUSE_ALL)
    assert np.all(np.isfinite(logits[0]))
    bits_equal(logits[0], logits[1], "FUSE_ALL against fusion mask 0")


PARLER_SYNTH = dict(wp.PARLER_Q4K, weight_type=Q4, head_type=F32, batch=2)
DIA_SYNTH = dict(wp.DIA_TINY, weight_type=Q4)


def weight_bytes(runner, obj):
    """{name: (type, bytes tts_<runner>_weight returns)}"""
    import ctypes
    prefix = wp.RUNNERS[runner][2]
    n_fn, w_fn = getattr(obj.L, prefix + "_n_weights"), getattr(obj.L, prefix + "_weight")
    out = {}
    for i in range(n_fn(obj.ptr)):
        name, ne, ty = ctypes.create_string_buffer(128), (ctypes.c_int64 * 4)(), ctypes.c_int32()
        n = w_fn(obj.ptr, i, name, 128, ne, ctypes.byref(ty), None, 0)
        a = np.empty(n, dtype=np.uint8)
        assert w_fn(obj.ptr, i, name, 128, ne, ctypes.byref(ty), a.ctypes.data, n) == n
        out[name.value.decode()] = (int(ty.value), a, tuple(ne))
    return out


def test_parler_synthetic_q4_0(hip, tmp_path):
    toks = []
    for _ in range(2):
        r = ttship.Parler(hip.iface(), ttship.parler_config(**PARLER_SYNTH))
        try:
            r.prefill((np.arange(10, dtype=np.int32).reshape(2, 5) * 17) % 512)
            toks.append(r.generate(6))
            held = weight_bytes("parler", r)
        finally:
            r.close()
    assert np.array_equal(toks[0], toks[1]) and toks[0].min() >= 0
    # tts_parler_weight returns ggml's bytes: what weight_store::host_bytes made, which the synthetic file holds too
    path = tmp_path / "synth.gguf"
    ttship.write_parler_synthetic_gguf(path, ttship.parler_config(**PARLER_SYNTH))
    n_q = 0
    with ttship.Gguf(path) as g:
        for name, (ty, data, _) in held.items():
            assert ty == g.tensor_type("decoder." + name) and np.array_equal(data, g.tensor_bytes("decoder." + name)), name
            n_q += ty == Q4
    assert n_q == 9 + 8 * PARLER_SYNTH["n_layers"]


def test_dia_synthetic_q4_0(hip):
    text = np.frombuffer(b"\x01 The birch canoe slid on the smooth planks.", dtype=np.uint8).astype(np.int32)[:32]
    runs, held = [], []
    for _ in range(2):
        r = ttship.Dia(hip.iface(), ttship.dia_config(**DIA_SYNTH))
        try:
            audio, seq = np.full(9, 1026, dtype=np.int32), []
            for s in range(4):
                lg = r.prefill(text, audio) if s == 0 else r.decode(audio)
                assert np.all(np.isfinite(lg))
                audio = lg.argmax(axis=1).astype(np.int32)
                seq.append(audio)
            runs.append(np.stack(seq))
            held.append(weight_bytes("dia", r))
        finally:
            r.close()
    assert np.array_equal(runs[0], runs[1])
    # the weights read back are the same Q4_0 blocks both times, spread like the default (Q8_0) configuration's
    o = ttship.Dia(hip.iface(), ttship.dia_config(**wp.DIA_TINY))
    try:
        q8 = weight_bytes("dia", o)
    finally:
        o.close()
    n_q = 0
    for name, (ty, data, ne) in held[0].items():
        assert np.array_equal(data, held[1][name][1]), name
        if ty != Q4:
            continue
        n_q += 1
        assert q8[name][0] == Q8 and data.size == ne[0] * ne[1] // 32 * 18, name
        a = q4.dequantize(data, ne[0], ne[1])
        b = py_oracle.dequant_q8_0(q8[name][1], ne[0], ne[1])
        assert abs(a.std() / b.std() - 1) < 0.2, (name, a.std(), b.std())
    assert n_q == len([1 for v in q8.values() if v[0] == Q8]) > 0
