"""Every byte a runner uploads, and the two synthetic GGUF files, against tests/golden/weights_pin.json.gz
(tests/weights_pin.py; CPU oracle backend), and the load path of the three runners that read a file."""
import ctypes

import numpy as np
import pytest

import py_oracle
import ttship
import weights_pin as wp

BF16 = 30  # a GGUF storage type the file format knows and no runner takes
T5_HIDDEN = wp.T5_TINY["hidden_size"]


@pytest.fixture(scope="module")
def fixture():
    return wp.load_fixture()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The two synthetic files, written once; {file id: sha256} rides along."""
    d = tmp_path_factory.mktemp("weights_pin")
    return d, {fid: wp.file_digest(fid, d) for fid in wp.FILES}


def test_every_weight_matches_the_pin(fixture):
    assert list(wp.CONFIGS) == list(fixture["configs"])  # nothing listed in the fixture is left unvisited
    for cid in wp.CONFIGS:
        got = wp.config_digests(cid, py_oracle.iface(4))
        assert len(got) == len(fixture["configs"][cid]) > 0, cid
        diff = wp.first_difference(cid, got, fixture["configs"][cid])
        assert diff is None, diff


def test_reference_counts(fixture):
    n = {cid: len(w) for cid, w in fixture["configs"].items()}
    assert (n["parler_q4k"], n["t5_f32"], n["orpheus_default"], n["dac"]) == (55, 23, 22, 117)


def test_synthetic_files_match_the_pin(files, fixture, tmp_path):
    assert sorted(files[1]) == sorted(fixture["files"])
    for fid, digest in files[1].items():
        assert digest == fixture["files"][fid], f"synthetic file {fid} differs from the pinned bytes"
        assert wp.file_digest(fid, tmp_path) == digest, f"two writes of {fid} differ"


def _from_file(runner, g):
    if runner == "parler":
        return ttship.Parler(py_oracle.iface(4), ttship.parler_config_from_gguf(g, max_ctx=wp.PARLER_Q4K["max_ctx"], arena_bytes=wp.SMALL_ARENA), gguf=g)
    if runner == "t5":
        return ttship.T5.from_gguf(py_oracle.iface(4), g, arena_bytes=wp.SMALL_ARENA)
    return ttship.Dac(py_oracle.iface(4), ttship.dac_config_from_gguf(g, max_frames=wp.DAC_TINY["max_frames"], arena_bytes=wp.SMALL_ARENA), gguf=g)


LOADS = [("parler", "parler_q4k_dac.gguf", "parler_q4k"), ("t5", "t5_f32.gguf", "t5_f32"), ("dac", "parler_q4k_dac.gguf", "dac")]


@pytest.mark.parametrize("runner,fid,cid", LOADS)
def test_runner_from_synthetic_file_holds_the_pinned_weights(files, fixture, runner, fid, cid):
    with ttship.Gguf(files[0] / fid) as g:
        r = _from_file(runner, g)
    try:
        diff = wp.first_difference(f"{cid} from {fid}", wp.weight_digests(runner, r), fixture["configs"][cid])
        assert diff is None, diff
    finally:
        r.close()


def _rewrite(src, dst, victim, how):
    """src's keys and tensors into dst, with tensor `victim` left out ("missing") or stored as BF16 ("type")."""
    with ttship.Gguf(src) as g:
        w = ttship.GgufWriter()
        w.copy_kv(g)
        seen = False
        for name, ty, ne, _, _ in g.tensors():
            if name != victim:
                w.add_tensor(name, ty, ne, g.tensor_bytes(name))
                continue
            seen = True
            if how == "type":
                w.add_tensor(name, BF16, ne, np.zeros(int(np.prod(ne)), dtype=np.uint16))
        assert seen, victim
        w.write(dst)
        w.close()


VICTIMS = {"parler": "decoder.layers.1.fc2.weight", "t5": "t5encoder.enc.blk.1.ffn_down",
           "dac": "audio_encoder.decoder_block.2.residual_unit.1.res.final.weight"}


@pytest.mark.parametrize("how", ["type", "missing"])
@pytest.mark.parametrize("runner,fid,cid", LOADS)
def test_create_from_gguf_refuses_a_damaged_file(files, tmp_path, runner, fid, cid, how):
    bad = tmp_path / f"{runner}-{how}.gguf"
    _rewrite(files[0] / fid, bad, VICTIMS[runner], how)
    with ttship.Gguf(bad) as g:
        with pytest.raises(RuntimeError):
            _from_file(runner, g)


def test_t5_takes_a_vector_stored_as_a_row(files, fixture, tmp_path):
    """The shared file check compares shapes with the 1-sized dimensions dropped (as Parler's and DAC's always
    did): a norm vector [N] that a file stores as [1, N] holds the same elements in the same order."""
    src, dst, victim = files[0] / "t5_f32.gguf", tmp_path / "row.gguf", "t5encoder.enc.final_layer_norm"
    with ttship.Gguf(src) as g:
        w = ttship.GgufWriter()
        w.copy_kv(g)
        for name, ty, ne, _, _ in g.tensors():
            w.add_tensor(name, ty, (1,) + tuple(ne) if name == victim else ne, g.tensor_bytes(name))
        w.write(dst)
        w.close()
    with ttship.Gguf(dst) as g:
        assert dict((t[0], t[2]) for t in g.tensors())[victim] == (1, T5_HIDDEN)
        r = _from_file("t5", g)
    try:
        diff = wp.first_difference("t5_f32 from a row vector", wp.weight_digests("t5", r), fixture["configs"]["t5_f32"])
        assert diff is None, diff
    finally:
        r.close()


def test_size_query_and_bounds(fixture):
    """tts_*_weight past the last weight returns 0, and a size query (dst NULL) returns the byte size."""
    t5 = ttship.T5(py_oracle.iface(2), wp.make_config("t5_f16"))
    try:
        L, name, ne, ty = t5.L, ctypes.create_string_buffer(8), (ctypes.c_int64 * 4)(), ctypes.c_int32()
        n = L.tts_t5_n_weights(t5.ptr)
        assert L.tts_t5_weight(t5.ptr, n, name, 8, ne, ctypes.byref(ty), None, 0) == 0
        assert L.tts_t5_weight(t5.ptr, -1, name, 8, ne, ctypes.byref(ty), None, 0) == 0
        assert L.tts_t5_weight(t5.ptr, 0, name, 8, ne, ctypes.byref(ty), None, 0) == 2 * ne[0] * ne[1] and ty.value == ttship.F16
        assert name.value == b"token_e"  # truncated to the caller's buffer, terminated
    finally:
        t5.close()
