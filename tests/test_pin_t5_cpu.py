"""The T5 encoder graph pinned to an independent implementation: transformers' T5EncoderModel.

The oracle and the HIP backend both run the node list built by tts.cpp_amd/csrc/t5.cpp, so the GPU suite
proves kernels == oracle on that list, not that the list is a T5 encoder.  Here transformers'
T5EncoderModel (gated-gelu feed-forward, 32 relative attention buckets, maximum distance 128, d_kv 64)
runs on the runner's own tiny F32 weights:
  - Parler's down projection and its bias, which T5EncoderModel does not have, are applied by hand;
  - the feed-forward activation is ggml's GELU (the tanh form looked up through an fp16 table, restated as
    tests/test_pin_parler_cpu.py restates it), not transformers' gelu_new;
  - n = 3 and n = 12 run transformers unpatched: every distance is <= 11, where the reference's bucket
    formula and transformers' agree;
  - n = 40 runs with T5Attention._relative_position_bucket replaced by the reference's formula
    (t5_runner::set_inputs, /root/reference/src/models/parler/t5/model.cpp:308-316): it takes the logarithm of an
    integer quotient, so it parts from transformers' at distances 12-15, 23, ... (test_t5_cpu.py), and it is
    the behaviour the runner reproduces.
The encodings must agree to 1e-4 of their scale, the other pins' bar."""
import numpy as np
import pytest
import torch

import py_oracle
import ttship
from test_t5_cpu import TINY, reference_bucket, tokens
from test_pin_parler_cpu import GgmlGelu


def t5_from_runner(w, cfg):
    from transformers import T5Config, T5EncoderModel
    tc = T5Config(vocab_size=cfg.vocab_size, d_model=cfg.hidden_size, d_kv=cfg.head_size, d_ff=cfg.ffn_size, num_layers=cfg.n_layers,
                  num_heads=cfg.n_attn_heads, relative_attention_num_buckets=32, relative_attention_max_distance=128,
                  dropout_rate=0.0, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu", is_encoder_decoder=False, use_cache=False)
    tc._attn_implementation = "eager"
    m = T5EncoderModel(tc).eval()
    sd = {"shared.weight": w["token_embd"], "encoder.embed_tokens.weight": w["token_embd"],
          "encoder.final_layer_norm.weight": w["enc.final_layer_norm"],
          "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": w["enc.blk.0.attn_rel_b"]}
    for l in range(cfg.n_layers):
        a, f, pre = f"encoder.block.{l}.layer.0", f"encoder.block.{l}.layer.1", f"enc.blk.{l}"
        for hf, mine in (("q", "attn_q"), ("k", "attn_k"), ("v", "attn_v"), ("o", "attn_o")):
            sd[f"{a}.SelfAttention.{hf}.weight"] = w[f"{pre}.{mine}"]
        sd[f"{a}.layer_norm.weight"] = w[f"{pre}.attn_norm"]
        sd[f"{f}.layer_norm.weight"] = w[f"{pre}.ffn_norm"]
        sd[f"{f}.DenseReluDense.wi_0.weight"] = w[f"{pre}.ffn_up"]    # the GELU branch
        sd[f"{f}.DenseReluDense.wi_1.weight"] = w[f"{pre}.ffn_gate"]
        sd[f"{f}.DenseReluDense.wo.weight"] = w[f"{pre}.ffn_down"]
    have = set(m.state_dict())
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items() if k in have}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    for blk in m.encoder.block:
        blk.layer[1].DenseReluDense.act = GgmlGelu()
    return m


def run_t5(m, w, ids):
    with torch.no_grad():
        h = m(input_ids=torch.from_numpy(np.asarray(ids, dtype=np.int64))[None]).last_hidden_state[0]
        out = h @ torch.from_numpy(w["down_proj"]).T + torch.from_numpy(w["down_proj_bias"])
    return out.numpy()


def reference_buckets(relative_position, bidirectional=True, num_buckets=32, max_distance=128):
    """The reference's formula in _relative_position_bucket's place: relative_position = key - query."""
    rp = relative_position.numpy()
    out = np.vectorize(lambda d: reference_bucket(int(d), 0, num_buckets))(rp)
    return torch.from_numpy(out.astype(np.int64))


def oracle_and_model(n):
    cfg = ttship.t5_config(**TINY)
    t = ttship.T5(py_oracle.iface(4), cfg)
    try:
        w = t.weights()
        ids = tokens(n)
        got = t.encode(ids)
    finally:
        t.close()
    return got, w, ids, t5_from_runner(w, cfg)


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("n", [3, 12])
def test_t5_graph_matches_transformers_encoder(n):
    got, w, ids, m = oracle_and_model(n)
    ref = run_t5(m, w, ids)
    err = rel_err(got, ref)
    print(f"n={n}: max|got-ref| / max|ref| = {err:.3g}")
    assert err <= 1e-4, err


def test_t5_graph_matches_transformers_with_the_reference_buckets(monkeypatch):
    from transformers.models.t5.modeling_t5 import T5Attention
    got, w, ids, m = oracle_and_model(40)
    unpatched = rel_err(got, run_t5(m, w, ids))
    monkeypatch.setattr(T5Attention, "_relative_position_bucket", staticmethod(reference_buckets))
    err = rel_err(got, run_t5(m, w, ids))
    print(f"n=40: reference buckets {err:.3g}, transformers' own buckets {unpatched:.3g}")
    assert err <= 1e-4, err


def test_pin_is_sensitive_to_the_relative_bias():
    """Without the relative attention bias on the transformers side the n = 12 encodings part by far more
    than the bar: measured 0.483 of the scale against the 1e-4 bound (the pinned runs measure 6.6e-6 at n = 3,
    4.6e-5 at n = 12, 2.8e-5 at n = 40; n = 40 with transformers' own buckets: 0.608)."""
    got, w, ids, m = oracle_and_model(12)
    with torch.no_grad():
        m.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.zero_()
    err = rel_err(got, run_t5(m, w, ids))
    print(f"n=12, bias zeroed: {err:.3g}")
    assert err > 1e-4, err
