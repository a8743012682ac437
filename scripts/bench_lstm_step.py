"""The fused LSTM step by weight type: one bidirectional chain at Kokoro's shape (n_in 640, hidden 256)
through the planner, slots F16, Q8_0, Q5_0, Q4_0, F16 in turn, several rounds in one process.

Each slot's graph (tests/lstm_quant.py: build_lstm_run node for node) is mirrored to the device once and
timed with device events around tts_hip_graph_compute.  A graph also holds the eight input projections and
the output writes, which differ by type, so the step time is the slope between two lengths:
(t(T) - t(T_short)) / (T - T_short) per launch (a launch advances both directions).  The two F16 slots give
the run-to-run margin.  One JSON line per slot, then a summary line.
Usage: python scripts/bench_lstm_step.py [T=512] [T_short=128] [rounds=7]
"""
import ctypes
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for d in ("tts.cpp_amd", "oracle", "tests"):
    sys.path.insert(0, str(ROOT / d))
import lstm  # noqa: E402
import lstm_q4_0 as l4  # noqa: E402
import lstm_quant as lq  # noqa: E402
import nodes as nd  # noqa: E402
import ttship  # noqa: E402

HIP = ctypes.CDLL("libamdhip64.so")


def event():
    e = ctypes.c_void_p()
    assert HIP.hipEventCreate(ctypes.byref(e)) == 0
    return e


class DeviceGraph:
    """A tests/nodes.Graph with every buffer on the device (Graph.run_hip's mirroring, kept across runs)."""

    def __init__(self, hip, g):
        self.hip, self.g, self.dev = hip, g, {}
        for t in g.tensors:
            if id(t) in g.arrays:
                buf = g.arrays[id(t)]
                d = hip.alloc(buf.nbytes)
                hip.set(d, buf)
                self.dev[id(t)] = d
                t.data = d
        for t in g.tensors:  # views (a gate's projection column) point into their owner's device buffer
            if getattr(t, "_root", None) is not None:
                owner, at = g.buffer_of(t)
                t.data = self.dev[id(owner)] + at
        assert all(ttship.lib().tts_hip_is_device_pointer(ctypes.c_void_p(t.data)) for t in g.tensors)
        self.ptrs, self.n = g.node_ptrs(), len(g.nodes)
        self.e0, self.e1 = event(), event()

    def run_ms(self):
        L = ttship.lib()
        L.tts_hip_event_record(ctypes.c_void_p(self.hip.ptr), self.e0)
        st = L.tts_hip_graph_compute(self.hip.ptr, self.ptrs, self.n)
        L.tts_hip_event_record(ctypes.c_void_p(self.hip.ptr), self.e1)
        assert st == 0 and HIP.hipEventSynchronize(self.e1) == 0
        ms = ctypes.c_float()
        assert HIP.hipEventElapsedTime(ctypes.byref(ms), self.e0, self.e1) == 0
        return ms.value

    def close(self):
        for d in self.dev.values():
            self.hip.free(d)


def main():
    args = [int(a) for a in sys.argv[1:4]]
    T, Ts, rounds = args + [512, 128, 7][len(args):]
    n_in, hd = 640, 256
    hip = ttship.HipBackend(0)
    rng = np.random.default_rng(0)
    dirs = lstm.lstm_weights(1, n_in, hd)
    slots = [("F16", ttship.F16), ("Q8_0", ttship.Q8_0), ("Q5_0", ttship.Q5_0), ("Q4_0", ttship.Q4_0), ("F16b", ttship.F16)]
    graphs = {}
    for name, wt in slots:
        for t in (T, Ts):
            x = (rng.standard_normal((t, n_in)) * 0.5).astype(np.float32)
            g = nd.Graph()
            if wt == ttship.Q4_0:
                l4.lstm_cell(g, x, dirs, "general")
            else:
                lq.lstm_cell(g, x, dirs, [wt, wt])
            graphs[name, t] = DeviceGraph(hip, g)
    times = {k: [] for k in graphs}
    c0 = hip.counters()
    for k, dg in graphs.items():
        dg.run_ms()  # warm-up: plan, code objects
    steps_per_pass = hip.counters()["lstm_steps"] - c0["lstm_steps"]
    assert steps_per_pass == 2 * len(slots) * (T + Ts), steps_per_pass  # every chain fused
    for _ in range(rounds):
        for k, dg in graphs.items():
            times[k].append(dg.run_ms())
    out = {}
    for name, _ in slots:
        a, b = float(np.median(times[name, T])), float(np.median(times[name, Ts]))
        out[name] = 1000.0 * (a - b) / (T - Ts)
        print(json.dumps({"bench": "lstm_step", "slot": name, "T": T, "T_short": Ts, "rounds": rounds, "graph_ms": round(a, 4),
                          "graph_ms_short": round(b, 4), "us_per_step_launch": round(out[name], 3),
                          "graph_ms_all": [round(v, 4) for v in times[name, T]]}), flush=True)
    f16 = 0.5 * (out["F16"] + out["F16b"])
    print(json.dumps({"bench": "lstm_step_summary", "f16_us": round(f16, 3), "f16_margin": round(abs(out["F16"] - out["F16b"]) / f16, 4),
                      "q8_0_over_f16": round(out["Q8_0"] / f16, 4), "q5_0_over_f16": round(out["Q5_0"] / f16, 4),
                      "q4_0_over_f16": round(out["Q4_0"] / f16, 4)}), flush=True)
    for dg in graphs.values():
        dg.close()
    hip.close()


if __name__ == "__main__":
    main()
