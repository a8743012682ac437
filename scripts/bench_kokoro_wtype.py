"""Kokoro-82M run() by weight type: F16, Q8_0, Q5_0 and Q4_0 runners (synthetic weights in the real shapes) in one
process, called in turn over several rounds; and, per type, both graphs with the LSTM fusion on and off.

One JSON line per type: ms per run() call (median over the rounds), audio-seconds per wall-second, the
duration graph and the main graph fused, and both with TTS_FUSE_LSTM cleared (the recurrences then run node
by node), with the unfused / fused ratios.
Usage: python scripts/bench_kokoro_wtype.py [n_tokens=64] [rounds=5]
"""
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tts.cpp_amd"))
import ttship  # noqa: E402

FUSE_LSTM = 64


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1000.0 * (time.perf_counter() - t0), out


def main():
    args = [int(a) for a in sys.argv[1:3]]
    n, rounds = args + [64, 5][len(args):]
    be = ttship.HipBackend(0)
    rng = np.random.default_rng(0)
    toks = rng.integers(1, 178, n).astype(np.int32)
    toks[0] = toks[-1] = 0
    types = [("F16", ttship.F16), ("Q8_0", ttship.Q8_0), ("Q5_0", ttship.Q5_0), ("Q4_0", ttship.Q4_0)]
    runners = {name: ttship.Kokoro(be.iface(), ttship.kokoro_config(max_tokens=max(n, 16), max_total=n * 12, weight_type=wt))
               for name, wt in types}
    res = {name: {"run": [], "dur": [], "dec": [], "dur_nofuse": [], "dec_nofuse": []} for name, _ in types}
    state = {}
    for name, k in runners.items():  # warm-up: plans, code objects, arena
        h, l = k.durations(toks)
        state[name] = (h, l, k.run(toks))
    for _ in range(rounds):
        for name, k in runners.items():
            h, l, _ = state[name]
            res[name]["run"].append(ms(lambda: k.run(toks))[0])
            res[name]["dur"].append(ms(lambda: k.durations(toks))[0])
            res[name]["dec"].append(ms(lambda: k.decode(toks, h, l))[0])
            be.set_option(0, ttship.FUSE_ALL & ~FUSE_LSTM)
            try:
                res[name]["dur_nofuse"].append(ms(lambda: k.durations(toks))[0])
                res[name]["dec_nofuse"].append(ms(lambda: k.decode(toks, h, l))[0])
            finally:
                be.set_option(0, ttship.FUSE_ALL)
    for name, _ in types:
        m = {key: float(np.median(v)) for key, v in res[name].items()}
        pcm = state[name][2]
        audio = pcm.shape[0] / 24000.0
        print(json.dumps({"bench": "kokoro_wtype", "type": name, "tokens": n, "rounds": rounds, "frames": int(state[name][1].sum()),
                          "audio_s": round(audio, 3), "ms_run": round(m["run"], 3), "audio_sec_per_s": round(audio / (m["run"] / 1000.0), 2),
                          "ms_durations": round(m["dur"], 3), "ms_decode": round(m["dec"], 3),
                          "ms_durations_lstm_unfused": round(m["dur_nofuse"], 3), "ms_decode_lstm_unfused": round(m["dec_nofuse"], 3),
                          "durations_unfused_over_fused": round(m["dur_nofuse"] / m["dur"], 3),
                          "decode_unfused_over_fused": round(m["dec_nofuse"] / m["dec"], 3),
                          "ms_run_all": [round(v, 3) for v in res[name]["run"]], "pcm_std": round(float(np.std(pcm)), 4)}), flush=True)
    for k in runners.values():
        k.close()
    be.close()


if __name__ == "__main__":
    main()
