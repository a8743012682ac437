"""R one-prompt Orpheus-3B workers on one GPU, TTS.cpp's server shape: every worker has its own backend, its own
copy of the weights and its own host thread, and runs TTS.cpp's loop (decode through graph_compute, read the
logits back, host argmax, next token).  Measures what the step coalescer buys them.

Synthetic Q4_K weights in the Orpheus-3B shapes, as scripts/bench_orpheus.py.  Each worker prefills a prompt of
its own length (prompt_len + 3 * worker), so the members sit at different KV positions.  After a warm-up round
with the coalescer on and one with it off, rounds alternate coalesce_enable(True) / coalesce_enable(False) within
the one process (ROUNDS of each); a round is `steps` decode steps per worker, the workers released together by a
barrier, timed from the release to the last worker's last logits.  Prints one JSON line: the median wall
milliseconds per step (a step = every worker advanced by one token) for both settings, the spread (min, max) within
each setting, and the coalescer's counters summed over the coalesced rounds.
usage: bench_orpheus_workers.py [R] [steps] [prompt_len] [layers]"""
import json
import pathlib
import statistics
import sys
import threading
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tts.cpp_amd"))
import ttship  # noqa: E402

ROUNDS = 3


def main():
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    n_prompt = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    kw = {"n_layers": int(sys.argv[4])} if len(sys.argv) > 4 and int(sys.argv[4]) > 0 else {}
    rounds = 2 * (ROUNDS + 1)
    max_ctx = n_prompt + 3 * R + rounds * steps + 8
    cfg = ttship.orpheus_config(batch=1, max_ctx=max_ctx, arena_bytes=1 << 28, **kw)
    t0 = time.perf_counter()
    bes = [ttship.HipBackend(0) for _ in range(R)]
    runs = [ttship.Orpheus(b.iface(reference_flow=True), cfg) for b in bes]
    t_load = time.perf_counter() - t0
    tok = [None] * R
    for r in range(R):
        n = n_prompt + 3 * r
        p = (np.arange(n, dtype=np.int32).reshape(1, n) * (7919 + 2 * r) + 128000 + r) % cfg.vocab_size
        tok[r] = runs[r].prefill(p).argmax(axis=1).astype(np.int32)
        bes[r].sync()
    errors = []

    def one_round():
        gate = threading.Barrier(R + 1)
        done = [0.0] * R

        def go(r):
            try:
                gate.wait()
                for _ in range(steps):
                    tok[r] = runs[r].decode(tok[r]).argmax(axis=1).astype(np.int32)  # TTS.cpp's loop: logits, host argmax
                done[r] = time.perf_counter()
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                gate.abort()

        th = [threading.Thread(target=go, args=(r,)) for r in range(R)]
        for t in th:
            t.start()
        gate.wait()
        t0 = time.perf_counter()
        for t in th:
            t.join()
        if errors:
            raise errors[0]
        return 1000.0 * (max(done) - t0) / steps

    keys = ("launches", "member_steps", "alone", "refused", "exec_us", "plan_us", "tables_us", "layout_us", "wait_us", "member_node_runs")
    ms = {True: [], False: []}
    counters = dict.fromkeys(keys, 0)
    prev = ttship.coalesce_enable(True)
    try:
        for i in range(rounds):
            on = i % 2 == 0
            ttship.coalesce_enable(on)
            c0 = ttship.coalesce_stats(0)
            t = one_round()
            c1 = ttship.coalesce_stats(0)
            if i < 2:
                continue  # warm-up: plans, code objects, the executor's memory, the members' verification
            ms[on].append(t)
            if on:
                for k in keys:
                    counters[k] += c1.get(k, 0) - c0.get(k, 0)
    finally:
        ttship.coalesce_enable(prev)
    launches = max(counters["launches"], 1)
    print(json.dumps({
        "workload": f"Orpheus-3B Q4_K, {R} one-prompt workers (own backend, weights and thread), {cfg.n_layers} layers, "
                    f"prompts {n_prompt}+3r, {steps} steps per round, {ROUNDS} rounds per setting",
        "coalesced_ms_per_step": round(statistics.median(ms[True]), 3),
        "coalesced_spread_ms": [round(min(ms[True]), 3), round(max(ms[True]), 3)],
        "alone_ms_per_step": round(statistics.median(ms[False]), 3),
        "alone_spread_ms": [round(min(ms[False]), 3), round(max(ms[False]), 3)],
        "coalescer": counters,
        "per_coalesced_launch_us": {k: round(counters[k] / launches, 1) for k in ("exec_us", "plan_us", "tables_us", "layout_us")},
        "members_per_launch": round(counters["member_steps"] / launches, 2),
        "load_s": round(t_load, 1)}), flush=True)
    for r in runs:
        r.close()
    for b in bes:
        b.close()


if __name__ == "__main__":
    main()
