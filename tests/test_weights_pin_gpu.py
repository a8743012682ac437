"""The weight pin (tests/weights_pin.py, tests/golden/weights_pin.json.gz) through the HIP backend, for the
configurations whose tensors are all F32 or F16: the device holds those as ggml does, so what
tts_<runner>_weight reads back is the uploaded bytes.  Quantized weights live in the backend's own
layout; the GPU-against-oracle parity tests cover them."""
import pytest

import weights_pin as wp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", wp.GPU_CONFIGS)
def test_uploaded_weights_match_the_pin(hip, cid):
    want = wp.load_fixture()["configs"][cid]
    assert all(w[1] in (0, 1) for w in want), f"{cid} holds a quantized tensor"  # F32 / F16 only, none left out
    got = wp.config_digests(cid, hip.iface())
    assert len(got) == len(want) > 0
    diff = wp.first_difference(cid, got, want)
    assert diff is None, diff
