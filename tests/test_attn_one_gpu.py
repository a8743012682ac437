"""The one-launch many-prompt decode attention (k_attn_one, TTS_HIP_OPT_ATTN_ONE) against the split pair it
replaces (k_attn_scores + k_attn_pv_mp, the option off) on the same inputs: output and shadow output bit-identical
(every sum is the pair's, in its order), and within the existing attention tests' bar of the oracle's unfused chain
(<= 1 ulp, almost all elements exact; exact up to 64 keys).

The launches go through tts_hip_attn_decode, which takes per-sequence key counts and K / V / mask offsets as a
coalesced step of runners at different KV lengths does: three sequences at different key counts in one launch,
every boundary of the kernel's geometry among them (one 64-position step, one round of 128 / 256, one 512-position
V item and one more).  The kernel is chosen where k_attn_pv_mp is (past 512 keys: with >= 256 rows); elsewhere the
option must leave the pair in place, so those cases check the fallback.
"""
import ctypes

import numpy as np
import pytest

import audio_ops as ao
import nodes as nd
import py_oracle
import ttship

F32 = ttship.F32
HD = 64
KEYS = [1, 63, 64, 65, 129, 460, 512, 513, 1025]
# three different key counts per launch; every count of KEYS but 1 is the longest (the grid's) of one launch
TRIPLES = [(1, 63, 64), (65, 1, 63), (64, 129, 65), (129, 460, 1), (460, 64, 512), (513, 65, 460), (512, 1025, 513)]


def td(ptr, ne, nb):
    t = ttship.TtsTensor()
    t.type = F32
    t.data = ptr
    for i in range(4):
        t.ne[i] = ne[i]
        t.nb[i] = nb[i]
    return t


class Case:
    """B sequences of one query each: q (B, H, hd); sequence b's K cache (cap, Hk*hd) position-major and V cache
    (Hk*hd, cap) transposed, cap a multiple of 4; its mask row of Ps[b] floats."""

    def __init__(self, Ps, H, Hk, masked, seed):
        rng = np.random.default_rng(seed)
        self.Ps, self.H, self.Hk, self.B = list(Ps), H, Hk, len(Ps)
        self.cap = (max(Ps) + 8 + 3) // 4 * 4
        self.q = rng.standard_normal((self.B, H, HD)).astype(np.float32)
        self.kc = rng.standard_normal((self.B, self.cap, Hk * HD)).astype(np.float32)
        self.vc = rng.standard_normal((self.B, Hk * HD, self.cap)).astype(np.float32)
        self.masks = None
        if masked:
            self.masks = [np.zeros(P, np.float32) for P in Ps]
            for m in self.masks:
                m[len(m) // 3] = -np.inf if len(m) > 4 else -0.5
                m[-1] = -1.25

    def run(self, hip, one):
        """One ragged launch; returns (out, shadow out) as (B, H, hd) arrays."""
        B, H, Hk, cap = self.B, self.H, self.Hk, self.cap
        koff = np.arange(B, dtype=np.int64) * cap * Hk * HD * 4
        voff = np.arange(B, dtype=np.int64) * cap * Hk * HD * 4
        pseq = np.asarray(self.Ps, np.int32)
        mflat = np.concatenate(self.masks) if self.masks else None
        moff = np.concatenate([[0], np.cumsum(self.Ps)[:-1]]).astype(np.int64)
        host = [self.q, self.kc, self.vc, koff, voff, pseq, moff] + ([mflat] if self.masks else [])
        dev = [hip.alloc(max(a.nbytes, 16)) for a in host]
        dout, dout2 = hip.alloc(B * H * HD * 4), hip.alloc(B * H * HD * 4)
        try:
            for d, a in zip(dev, host):
                hip.set(d, np.ascontiguousarray(a))
            dq, dk, dv, dkoff, dvoff, dpseq, dmoff = dev[:7]
            dmask = dev[7] if self.masks else None
            P = max(self.Ps)
            tq = td(dq, [HD, 1, H, B], [4, HD * 4, HD * 4, H * HD * 4])
            tk = td(dk, [HD, P, Hk, 1], [4, Hk * HD * 4, HD * 4, 0])
            tv = td(dv, [P, HD, Hk, 1], [4, cap * 4, cap * HD * 4, 0])
            hip.set_option(ttship.OPT["ATTN_ONE"], one)
            try:
                for d in (dout, dout2):
                    hip.L.tts_hip_memset(hip.ptr, d, 0xFF, B * H * HD * 4)
                st = hip.L.tts_hip_attn_decode(hip.ptr, ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), dmask, 0,
                                               float(1.0 / np.sqrt(HD)), dout, dout2, dkoff, dvoff, dmoff if self.masks else None, dpseq)
                assert st == 0, st
                hip.sync()
            finally:
                hip.set_option(ttship.OPT["ATTN_ONE"], DEFAULT_ONE)
            out, out2 = np.empty((B, H, HD), np.float32), np.empty((B, H, HD), np.float32)
            hip.get(out, dout)
            hip.get(out2, dout2)
            return out, out2
        finally:
            for d in dev + [dout, dout2]:
                hip.free(d)

    def oracle(self, b):
        """Sequence b alone through the reference's unfused node chain on the CPU oracle: (H, hd).  Under GQA the
        chain sees every K / V head repeated for its H / Hk query heads (the models' repeat_interleave)."""
        P, H, cap = self.Ps[b], self.H, self.cap
        rep = H // self.Hk
        kcb = np.repeat(self.kc[b].reshape(cap, self.Hk, HD), rep, axis=1).reshape(1, cap, H * HD)
        vcb = np.repeat(self.vc[b].reshape(self.Hk, HD, cap), rep, axis=0).reshape(1, H * HD, cap)
        Hk = H
        g = nd.Graph()
        ql = g.leaf(self.q[b].reshape(1, 1, H, HD))
        qc = g.node("CONT", F32, [HD, 1, H, 1], [g.permute(ql, (0, 2, 1, 3))])
        kl = g.leaf(np.ascontiguousarray(kcb))
        kcont = g.node("CONT", F32, [HD, P, Hk, 1], [g.view(kl, [HD, P, Hk, 1], [4, Hk * HD * 4, HD * 4, kl.nb[2]])])
        kq = g.node("MUL_MAT", F32, [P, 1, H, 1], [kcont, qc])
        ml = g.leaf((self.masks[b] if self.masks else np.zeros(P, np.float32)).reshape(1, P))
        sm = g.node("SOFT_MAX", F32, [P, 1, H, 1], [kq, ml], fparams={0: float(1.0 / np.sqrt(HD)), 1: 0.0})
        vl = g.leaf(np.ascontiguousarray(vcb))
        v = g.view(vl, [P, HD, Hk, 1], [4, cap * 4, cap * HD * 4, vl.nb[2]])
        kqv = g.node("MUL_MAT", F32, [1, HD, H, 1], [sm, v])
        o = g.node("CONT", F32, [HD, H, 1, 1], [g.permute(kqv, (2, 0, 1, 3))])
        g.run_oracle(n_threads=4)
        return g.node_array(o).reshape(H, HD)


DEFAULT_ONE = ttship.ATTN_ONE_DEFAULT  # what the shared backend is put back to


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Ps", TRIPLES)
def test_three_key_counts_one_launch(hip, Ps, masked):
    """hd 64, H = 2, three sequences at different key counts in one launch, with and without a mask (one key masked
    out, one biased): both round depths of the option bit-identical to the pair, output and shadow; the pair's bar
    against the oracle.  Six rows: up to 512 keys the new kernel runs, past them the option must fall back."""
    c = Case(Ps, 2, 2, masked, seed=sum(Ps) * 2 + masked)
    ref, ref2 = c.run(hip, 0)
    assert np.array_equal(bits(ref), bits(ref2))
    for one in (1, 2):
        out, out2 = c.run(hip, one)
        assert np.array_equal(bits(out), bits(ref)), f"ATTN_ONE={one}: output differs from the pair's"
        assert np.array_equal(bits(out2), bits(ref)), f"ATTN_ONE={one}: shadow output differs from the pair's"
    orc = np.stack([c.oracle(b) for b in range(c.B)])
    print("ulp", ao.ulp_diff(ref, orc), "mismatch fraction", float(np.mean(ref != orc)))
    if max(Ps) <= 64:
        assert np.array_equal(ref, orc)
    else:
        assert ao.ulp_diff(ref, orc) <= 1 and np.mean(ref != orc) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("pmax", [460, 513, 1025])
def test_gqa_many_rows(hip, pmax):
    """One K / V head under 16 query heads (GQA), 16 sequences: 256 rows, so the new kernel also runs past 512 keys
    (two and three 512-position V items per pass); key counts from every boundary up to pmax, masked."""
    Ps = [p for p in KEYS if p < pmax][-7:] + [pmax]
    Ps = (Ps * 2)[:16]
    c = Case(Ps, 16, 1, True, seed=pmax)
    ref, ref2 = c.run(hip, 0)
    for one in (1, 2):
        out, out2 = c.run(hip, one)
        assert np.array_equal(bits(out), bits(ref)) and np.array_equal(bits(out2), bits(ref2)), one
    b = Ps.index(pmax)
    orc = c.oracle(b)
    print("ulp", ao.ulp_diff(ref[b], orc), "mismatch fraction", float(np.mean(ref[b] != orc)))
    assert ao.ulp_diff(ref[b], orc) <= 1 and np.mean(ref[b] != orc) <= 1e-3


@pytest.mark.gpu
def test_graph_attention_item(hip):
    """The same kernel behind a graph's fused attention item (32 sequences x 16 heads at 460 keys, the many-prompt
    step's shape, one shared mask): bit-identical to the pair."""
    P, H, B, cap = 460, 16, 32, 464
    rng = np.random.default_rng(7)
    q = rng.standard_normal((B, H, HD)).astype(np.float32)
    kc = rng.standard_normal((B, cap, H * HD)).astype(np.float32)
    vc = rng.standard_normal((B, H * HD, cap)).astype(np.float32)
    mask = np.zeros(P, np.float32)
    mask[P // 2] = -np.inf
    outs = []
    for one in (0, 1, 2):
        g = nd.Graph()
        ql = g.leaf(q.reshape(B, 1, H, HD))
        qc = g.node("CONT", F32, [HD, 1, H, B], [g.permute(ql, (0, 2, 1, 3))])
        kl = g.leaf(kc)
        kcont = g.node("CONT", F32, [HD, P, H, B], [g.view(kl, [HD, P, H, B], [4, H * HD * 4, HD * 4, kl.nb[2]])])
        kq = g.node("MUL_MAT", F32, [P, 1, H, B], [kcont, qc])
        sm = g.node("SOFT_MAX", F32, [P, 1, H, B], [kq, g.leaf(mask.reshape(1, P))], fparams={0: 0.125, 1: 0.0})
        vl = g.leaf(vc)
        kqv = g.node("MUL_MAT", F32, [1, HD, H, B], [sm, g.view(vl, [P, HD, H, B], [4, cap * 4, cap * HD * 4, vl.nb[2]])])
        o = g.node("CONT", F32, [HD, H, 1, B], [g.permute(kqv, (2, 0, 1, 3))])
        hip.set_option(ttship.OPT["ATTN_ONE"], one)
        try:
            g.run_hip(hip)
        finally:
            hip.set_option(ttship.OPT["ATTN_ONE"], DEFAULT_ONE)
        outs.append(g.node_array(o).copy())
    assert np.array_equal(bits(outs[1]), bits(outs[0])) and np.array_equal(bits(outs[2]), bits(outs[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("one", [1, 2])
def test_17_lockstep_prompts_tokens_exact(one):
    """Parler tiny, 17 lock-step prompts of 126 tokens, 4 steps (the key count crosses 128, where the split pair and
    with it the one-launch kernel take over from the row kernel): greedy tokens bit-exact vs the oracle."""
    kw = dict(n_layers=2, hidden_size=256, n_attn_heads=4, ffn_size=1024, output_vocab=1088, max_ctx=192, prompt_vocab=512,
              max_positions=256, batch=17)
    be = ttship.HipBackend(0)
    be.set_option(ttship.OPT["ATTN_ONE"], one)
    g = ttship.Parler(be.iface(), ttship.parler_config(**kw))
    c = ttship.Parler(py_oracle.iface(8), ttship.parler_config(**kw))
    try:
        prompt = (np.arange(126 * 17, dtype=np.int32).reshape(17, 126) * 53 + 11) % 512
        g.prefill(prompt)
        c.prefill(prompt)
        tg, tc = g.generate(4), c.generate(4)
        assert np.array_equal(tg, tc), f"token mismatch vs oracle\n{tg}\n{tc}"
    finally:
        g.close()
        c.close()
        be.close()
