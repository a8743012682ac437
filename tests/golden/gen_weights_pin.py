"""Generates tests/golden/weights_pin.json.gz: the bytes every runner uploads, and the two synthetic GGUF files.

Generated once, from the commit before the shared weight store (csrc/weights.cpp), on the CPU oracle
backend; tests/test_weights_pin_cpu.py and tests/test_weights_pin_gpu.py compare against it.  The
configurations live in tests/weights_pin.py.  Regenerating it after that commit defeats its purpose.

Run (after `make`): python tests/golden/gen_weights_pin.py
"""
import pathlib
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in ("tts.cpp_amd", "oracle", "tests"):
    sys.path.insert(0, str(ROOT / p))

import py_oracle  # noqa: E402
import weights_pin  # noqa: E402


def main():
    out = {"configs": {}, "files": {}}
    for cid in weights_pin.CONFIGS:
        out["configs"][cid] = weights_pin.config_digests(cid, py_oracle.iface(4))
        print(cid, len(out["configs"][cid]), "weights")
    with tempfile.TemporaryDirectory() as d:
        for fid in weights_pin.FILES:
            a, b = weights_pin.file_digest(fid, d), weights_pin.file_digest(fid, d)
            assert a == b, f"{fid}: two writes differ"
            out["files"][fid] = a
    weights_pin.save_fixture(out)
    print("wrote", weights_pin.FIXTURE, weights_pin.FIXTURE.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
