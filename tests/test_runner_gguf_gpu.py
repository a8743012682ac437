"""Dia, Orpheus and SNAC from GGUF files on the HIP backend against the CPU oracle, bit for bit: the files of
tests/test_runner_gguf_cpu.py through the quantize tool, each runner created from the file on both sides.  The oracle
holds no Q5_0 or Q4_0: it runs the file's Q8_0 twin, which equals a Q5_0 file and a Q4_0 file with trimmed block
scales under it (tests/runner_gguf.py); an untrimmed Q4_0 file is compared HIP against HIP, fused against unfused."""
import numpy as np
import pytest

import py_oracle
import runner_gguf as rg
import ttship
from runner_gguf import F16, F32, Q4_0, Q4_K, Q5_0, Q8_0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return rg.write_f32(tmp_path_factory.mktemp("runner_gguf_gpu"))


@pytest.fixture(scope="module")
def it():
    return py_oracle.iface(8)


def _close(*runners):
    for r in runners:
        r.close()


@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("qtype", [Q8_0, Q5_0, Q4_0, F16])
def test_dia_from_quantized_file(hip, it, files, qtype, heads):
    """Prefill with 5 real tokens in the 32-token context and 3 decode steps, a 4-step generate, then DAC on 4 frames from
    the same file.  heads: the nine heads quantized too, multiplied at the CFG pair's two columns."""
    _, run_f, twin_f = rg.quantized(files[0], qtype, heads)
    with ttship.Gguf(run_f) as g, ttship.Gguf(twin_f) as t:
        cg = ttship.dia_config_from_gguf(g, arena_bytes=rg.ARENA)
        assert (cg.weight_type, cg.head_type) == (qtype, qtype if heads else F32)
        run, ref = ttship.Dia(hip.iface(), cg, gguf=g), ttship.Dia.from_gguf(it, t, arena_bytes=rg.ARENA)
        dac, dac_ref = (ttship.Dac(i, ttship.dac_config_from_gguf(f, max_frames=16), gguf=f) for i, f in ((hip.iface(), g), (it, t)))
    try:
        got, want = rg.dia_logits(run), rg.dia_logits(ref)
        for s in range(len(want)):
            rg.bits_equal(want[s], got[s], f"dia {rg.TYPE_NAME[qtype]} step {s}")
        first = want[-1].argmax(axis=1).astype(np.int32)
        assert np.array_equal(run.generate(first, 4), ref.generate(first, 4))
        assert run.position() == ref.position() == 8
        rg.bits_equal(dac_ref.decode(rg.dac_codes(4)), dac.decode(rg.dac_codes(4)), "dac pcm")
    finally:
        _close(run, ref, dac, dac_ref)


@pytest.mark.parametrize("qtype,heads,batch", [(Q4_K, False, 1), (Q4_K, False, 2), (Q4_K, True, 1), (Q4_K, True, 2), (Q8_0, False, 1),
                                               (Q5_0, False, 2), (Q4_0, False, 1), (Q4_0, True, 2)])
def test_orpheus_from_quantized_file(hip, it, files, qtype, heads, batch):
    """Prefill of 5 tokens and 3 decode steps, then SNAC on 8 frames from the same file.  heads False: an F32 lm_head
    beside quantized matrices and a quantized embedding, as the tool writes without quantize_output_heads."""
    _, run_f, twin_f = rg.quantized(files[1], qtype, heads)
    kw = dict(max_ctx=rg.ORPHEUS["max_ctx"], arena_bytes=rg.ARENA, batch=batch)
    with ttship.Gguf(run_f) as g, ttship.Gguf(twin_f) as t:
        assert g.tensor_type("orpheus.lm_head") == (qtype if heads else F32) and g.tensor_type("orpheus.embed_tokens") == qtype
        run, ref = ttship.Orpheus.from_gguf(hip.iface(), g, **kw), ttship.Orpheus.from_gguf(it, t, **kw)
        snac, snac_ref = ttship.Snac.from_gguf(hip.iface(), g, max_frames=32), ttship.Snac.from_gguf(it, t, max_frames=32)
    try:
        got, want = rg.orpheus_logits(run, batch), rg.orpheus_logits(ref, batch)
        for s in range(len(want)):
            rg.bits_equal(want[s], got[s], f"orpheus {rg.TYPE_NAME[qtype]} step {s}")
        heads_in, z = rg.snac_inputs(8, snac.noise_per_frame)
        rg.bits_equal(snac_ref.decode(heads_in, z), snac.decode(heads_in, z), "snac pcm")
    finally:
        _close(run, ref, snac, snac_ref)


@pytest.mark.parametrize("which", ["dia", "orpheus"])
def test_untrimmed_q4_0_file_fused_equals_unfused(hip, files, which):
    """HIP against HIP: the Q4_0 file as the tool writes it (general block scales, heads quantized) loads, and its logits
    with every fusion on equal the same runner's with every fusion off."""
    out, _, _ = rg.quantized(files[0 if which == "dia" else 1], Q4_0, True)
    logits = []
    for mask in (ttship.FUSE_ALL, 0):
        hip.set_option(ttship.OPT["FUSION"], mask)
        try:
            with ttship.Gguf(out) as g:
                if which == "dia":
                    run = ttship.Dia.from_gguf(hip.iface(), g, arena_bytes=rg.ARENA)
                else:
                    run = ttship.Orpheus.from_gguf(hip.iface(), g, max_ctx=rg.ORPHEUS["max_ctx"], arena_bytes=rg.ARENA, batch=2)
            try:
                logits.append(rg.dia_logits(run) if which == "dia" else rg.orpheus_logits(run, 2))
            finally:
                run.close()
        finally:
            hip.set_option(ttship.OPT["FUSION"], ttship.FUSE_ALL)
    rg.bits_equal(logits[1], logits[0], "FUSE_ALL against fusion mask 0")


@pytest.mark.parametrize("qtype", [Q4_K, Q5_0])
def test_synthetic_runner_with_the_files_weights_set(hip, files, qtype):
    """tts_orpheus_set_weight on the device: a synthetic runner given the file's bytes weight by weight (the backend
    lays each out as at upload) computes what the runner loaded from the file computes."""
    _, run_f, _ = rg.quantized(files[1], qtype, True)
    with ttship.Gguf(run_f) as g:
        run = ttship.Orpheus.from_gguf(hip.iface(), g, max_ctx=rg.ORPHEUS["max_ctx"], arena_bytes=rg.ARENA)
        ref = ttship.Orpheus(hip.iface(), rg.orpheus_cfg(weight_type=qtype))
        try:
            before = rg.orpheus_logits(ref)
            ref.L.tts_orpheus_reset(ref.ptr)
            rg.set_weights_from_file(ref, g, "orpheus.", rg.orpheus_name_map())
            got = rg.orpheus_logits(run)
            rg.bits_equal(got, rg.orpheus_logits(ref), "logits after set_weight")
            assert not np.array_equal(before, got)
        finally:
            _close(run, ref)


@pytest.mark.parametrize("qtype", [Q4_K, Q4_0])
def test_device_quantize_tool_on_the_orpheus_file(hip, files, qtype):
    host, _, _ = rg.quantized(files[1], qtype, False)
    dev, _, _ = rg.quantized(files[1], qtype, False, backend=hip)
    assert dev != host and dev.read_bytes() == host.read_bytes()
