"""bench.py's host-side rules (no device): prompts per batched DAC decode, the --dump-outputs files."""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def ns(**kw):
    base = dict(dac_batch=None, steps=20, per_gpu_=64)
    base.update(kw)
    return argparse.Namespace(**base)


def test_dac_batch_rule():
    assert bench.dac_batch(ns()) == 8            # 64 prompts per GPU, short sequences: 8 per decode
    assert bench.dac_batch(ns(per_gpu_=32)) == 8
    assert bench.dac_batch(ns(per_gpu_=8)) == 4  # the 8-GPU share: two decoders of 4
    assert bench.dac_batch(ns(per_gpu_=2)) == 1
    assert bench.dac_batch(ns(steps=861)) == 1   # long sequences one by one
    assert bench.dac_batch(ns(steps=64)) == 8 and bench.dac_batch(ns(steps=65)) == 1
    assert bench.dac_batch(ns(dac_batch=3, steps=861)) == 3  # an explicit --dac-batch wins
    assert bench.dac_batch(ns(dac_batch=0)) == 1


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy files; PCM whole when it fits the budget, else the same seeded
    ascending sample of it on every call."""
    rng = np.random.default_rng(3)
    toks = rng.integers(0, 1088, (4, 5, 9)).astype(np.int32)
    pcms = [rng.standard_normal(5 * 512).astype(np.float32) for _ in range(4)]
    bench.dump_outputs(tmp_path / "a", toks, pcms)
    t, p = np.load(tmp_path / "a" / "codec_tokens.npy"), np.load(tmp_path / "a" / "pcm.npy")
    assert t.dtype == np.float32 and np.array_equal(t, toks)
    assert p.dtype == np.float32 and np.array_equal(p, np.concatenate(pcms))
    monkeypatch.setattr(bench, "DUMP_PCM_SAMPLES", 1000)
    bench.dump_outputs(tmp_path / "b", toks, pcms)
    bench.dump_outputs(tmp_path / "c", toks, None)  # --no-dac: tokens only
    s = np.load(tmp_path / "b" / "pcm.npy")
    assert s.shape == (1000,) and np.all(np.isin(s, p))
    bench.dump_outputs(tmp_path / "b2", toks, pcms)
    assert np.array_equal(s, np.load(tmp_path / "b2" / "pcm.npy"))
    assert not (tmp_path / "c" / "pcm.npy").exists() and (tmp_path / "c" / "codec_tokens.npy").exists()
