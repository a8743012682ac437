"""T5 voice-description encoder on the HIP backend vs the CPU oracle running the same node list: every
layer's attention is one k_attn_bias launch (written through the staging buffer when the arena put the
output on top of an operand), the projections the float GEMV / GEMM kernels.  The bound is the project's
whole-model bar, 1e-4 of the scale + 1e-4 (tests/test_dia_gpu.py)."""
import numpy as np
import pytest

import py_oracle
import ttship
from test_t5_cpu import PARLER, TINY, TINY_F16, tokens

WIDE = dict(n_layers=2, hidden_size=1024, n_attn_heads=16, head_size=64, ffn_size=2816, vocab_size=512, max_context_length=64,
            output_size=1024, has_down_proj=1, weight_type=ttship.F32)  # flan-t5-large's widths, two layers


def close_enough(got, ref, tag):
    tol = 1e-4 * np.abs(ref).max() + 1e-4
    err = np.abs(got - ref).max()
    print(f"{tag}: max|gpu-oracle| {err:.3g} (bound {tol:.3g}), {int(np.sum(got != ref))} of {got.size} elements differ")
    assert np.isfinite(got).all()
    assert err <= tol, (tag, err, tol)
    # and the same bits at these shapes: the attention sums in the oracle's order by construction, the
    # projections' f64 sums (split over K at some shapes) round to the oracle's f32 values
    assert np.array_equal(got, ref), tag


@pytest.fixture(scope="module")
def pairs(hip):
    made = {}

    def get(name, cfg):
        if name not in made:
            made[name] = (ttship.T5(hip.iface(), ttship.t5_config(**cfg)), ttship.T5(py_oracle.iface(16), ttship.t5_config(**cfg)))
        return made[name]

    yield get
    for g, c in made.values():
        g.close()
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 65, 130])
@pytest.mark.parametrize("name,cfg", [("f32", TINY), ("f16", TINY_F16)])
def test_t5_tiny_matches_oracle(pairs, name, cfg, n):
    g, c = pairs(name, cfg)
    got, ref = g.encode(tokens(n)), c.encode(tokens(n))
    assert g.plan_stats()["attn"] == cfg["n_layers"]
    close_enough(got, ref, f"{name} n={n}")


@pytest.mark.gpu
def test_t5_wide_two_layers(pairs):
    g, c = pairs("wide", WIDE)
    ids = tokens(48, vocab=512)
    got, ref = g.encode(ids), c.encode(ids)
    assert g.plan_stats()["attn"] == 2
    close_enough(got, ref, "wide n=48")


@pytest.mark.gpu
def test_lengths_change_between_calls(pairs):
    """n = 13, then n = 5 on one runner: no bias, bucket or staging state of the longer call survives."""
    g, c = pairs("f32", TINY)
    for n in (13, 5, 13):
        close_enough(g.encode(tokens(n, seed=n)), c.encode(tokens(n, seed=n)), f"n={n}")
    # the same graph again (recorded on its second sighting) gives the same bits
    a = g.encode(tokens(5, seed=1))
    assert np.array_equal(a, g.encode(tokens(5, seed=1)))
    assert np.array_equal(a, g.encode(tokens(5, seed=1)))


@pytest.mark.gpu
def test_t5_encoding_sets_parlers_voice(hip):
    """T5.encode -> Parler.set_conditional_prompt -> 4 greedy steps: the oracle's tokens."""
    n = 6
    out = []
    for iface in (hip.iface(), py_oracle.iface(16)):
        t = ttship.T5(iface, ttship.t5_config(**dict(TINY, output_size=PARLER["hidden_size"])))
        p = ttship.Parler(iface, ttship.parler_config(**dict(PARLER, n_encode=n)))
        try:
            p.prefill((np.arange(5, dtype=np.int32)[None] * 13) % 300)
            before = p.generate(4)
            p.set_conditional_prompt(t.encode(tokens(n)))
            p.prefill((np.arange(5, dtype=np.int32)[None] * 13) % 300)
            out.append((before, p.generate(4)))
        finally:
            t.close()
            p.close()
    (gb, ga), (cb, ca) = out
    assert np.array_equal(gb, cb)
    assert np.array_equal(ga, ca)
