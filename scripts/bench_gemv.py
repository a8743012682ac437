"""GEMV micro-benchmark (raw tts_hip_gemv entry, HIP-event timed on the backend stream).

Shapes: the Parler-mini decode matrices, Orpheus-3B / Dia sizes, at M = 1 and 8 columns.
Prints one JSON line per shape with avg us per launch and algorithmic GB/s.

bench_gemv.py q5 [reps] [rounds] [M list] [cold]: Q5_0 beside Q8_0 at the same shapes in the same run,
interleaved -- per (shape, M) and round the slots Q8_0, Q5_0, Q8_0 again, `reps` launches each; one JSON
line with the per-round averages, the medians and the Q8_0-against-Q8_0 spread (the margin a Q5_0 / Q8_0
difference has to clear).

bench_gemv.py q4 [reps] [rounds] [M list] [cold]: the same with the slots Q8_0, Q5_0, Q4_0, Q8_0 again.  Cold:
every type's launches rotate through enough copies that 512 MiB of the smallest type's weights pass between two
uses of one copy.

bench_gemv.py q6 [reps] [rounds] [M list] [cold] [shape names]: Q6_K beside Q4_K and Q8_0 on the Parler and Orpheus
matrices (Q6_K_SHAPES), slots Q8_0, Q4_K, Q6_K, Q8_0 again; times are per tts_hip_gemv call (a call may be several
launches).
"""
import json
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tts.cpp_amd"))
import ttship  # noqa: E402

SHAPES = [  # (name, type, K, N)
    ("parler_qkvo", ttship.Q4_K, 1024, 1024),
    ("parler_fc1", ttship.Q4_K, 1024, 4096),
    ("parler_fc2", ttship.Q4_K, 4096, 1024),
    ("orpheus_q", ttship.Q4_K, 3072, 3072),
    ("orpheus_up", ttship.Q4_K, 3072, 8192),
    ("orpheus_down", ttship.Q4_K, 8192, 3072),
    ("orpheus_head", ttship.Q4_K, 3072, 156940),
    ("dia_ffn", ttship.Q8_0, 2048, 8192),
    ("parler_head_f32", ttship.F32, 1024, 1088 * 9),
]


Q5_SHAPES = [(1024, 1024), (1024, 4096), (4096, 1024), (2048, 2048), (2048, 8192)]  # (K, N)


Q6_K_SHAPES = [("parler_qkvo", 1024, 1024), ("parler_fc1", 1024, 4096), ("parler_fc2", 4096, 1024), ("orpheus_q", 3072, 3072),
               ("orpheus_up", 3072, 8192), ("orpheus_down", 8192, 3072), ("orpheus_head", 3072, 156940)]  # (name, K, N)


def quant_bytes(rng, wt, K, N, dmin=False):
    """Random blocks of type wt with a small finite fp16 d (Q6_K: d is the block's last field; dmin: Q4_K's dmin too,
    which the q6 mode sets and the older modes, which never pass Q4_K, do not)."""
    bs = ttship.TYPE_SIZE[wt]
    w = rng.integers(0, 256, size=ttship.row_size(wt, K) * N, dtype=np.uint8)
    d = np.frombuffer(np.float16(1e-3).tobytes(), dtype=np.uint8)
    blk = w.reshape(-1, bs)
    if wt == ttship.Q6_K:
        blk[:, 208:210] = d
    else:
        blk[:, 0:2] = d
        if wt == ttship.Q4_K and dmin:
            blk[:, 2:4] = d
    return w


def compare_q6():
    """q6 mode: per (shape, M) and round the slots Q8_0, Q4_K, Q6_K, Q8_0 again."""
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    mlist = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1, 2, 8, 32]
    cold = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    only = sys.argv[6].split(",") if len(sys.argv) > 6 else None
    hip = ttship.HipBackend(0)
    L = ttship.lib()
    rng = np.random.default_rng(0)
    types = (ttship.Q8_0, ttship.Q4_K, ttship.Q6_K)
    for name, K, N in Q6_K_SHAPES:
        if only and name not in only:
            continue
        dev = {}
        for wt in types:
            w = quant_bytes(rng, wt, K, N, dmin=True)
            # cold: as many copies of the SMALLEST (Q4_K) matrix as pass 512 MiB, the same count for every type
            ncopy = -(-(512 << 20) // (ttship.row_size(ttship.Q4_K, K) * N)) if cold else 1
            dev[wt] = [hip.alloc(w.nbytes) for _ in range(ncopy)]
            for d in dev[wt]:
                hip.set(d, w)
        at = {wt: 0 for wt in types}
        for M in mlist:
            x = rng.standard_normal((M, K)).astype(np.float32)
            dx, dy = hip.alloc(x.nbytes), hip.alloc(4 * M * N)
            hip.set(dx, x)

            def slot(wt, n):
                for _ in range(n):
                    L.tts_hip_gemv_ex(hip.ptr, wt, dev[wt][at[wt] % len(dev[wt])], dx, dy, K, N, M, 0)
                    at[wt] += 1

            for wt in dev:
                slot(wt, 2)
            hip.sync()
            hip.set_option(ttship.OPT["PROFILE_GEMV"], 1)
            order = (("q8_0_a", ttship.Q8_0), ("q4_K", ttship.Q4_K), ("q6_K", ttship.Q6_K), ("q8_0_b", ttship.Q8_0))
            us = {key: [] for key, _ in order}
            for _ in range(rounds):
                for key, wt in order:
                    hip.gemv_stats(-1, reset=True)
                    slot(wt, reps)
                    ms, n, _ = hip.gemv_stats(wt, reset=True)
                    assert n >= reps, (n, reps)
                    us[key].append(round(1000.0 * ms / reps, 2))
            hip.set_option(ttship.OPT["PROFILE_GEMV"], 0)
            med = {k: float(np.median(v)) for k, v in us.items()}
            q8 = 0.5 * (med["q8_0_a"] + med["q8_0_b"])
            b6 = ttship.row_size(ttship.Q6_K, K) * N
            print(json.dumps({"shape": name, "K": K, "N": N, "M": M, "cold": cold, "copies": len(dev[ttship.Q6_K]), "reps": reps, "us_per_round": us,
                              "median_us": med, "q8_0_vs_q8_0_spread_us": round(max(abs(a - b) for a, b in zip(us["q8_0_a"], us["q8_0_b"])), 2),
                              "q6_K_over_q8_0": round(med["q6_K"] / q8, 3), "q6_K_over_q4_K": round(med["q6_K"] / med["q4_K"], 3),
                              "q6_K_weight_GBps": round(b6 / (med["q6_K"] * 1e-6) / 1e9, 1)}), flush=True)
            hip.free(dx)
            hip.free(dy)
        for ds in dev.values():
            for d in ds:
                hip.free(d)
    hip.close()


def compare_q5():
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    mlist = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1, 2, 8, 32]
    cold = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    hip = ttship.HipBackend(0)
    L = ttship.lib()
    rng = np.random.default_rng(0)
    for K, N in Q5_SHAPES:
        dev = {}
        for wt in (ttship.Q8_0, ttship.Q5_0):
            w = quant_bytes(rng, wt, K, N)
            # cold: as many copies of the LARGER (Q8_0) matrix as pass 512 MiB, the same count for both types
            ncopy = max(1, min(64, -(-(512 << 20) // (ttship.row_size(ttship.Q8_0, K) * N)))) if cold else 1
            dev[wt] = [hip.alloc(w.nbytes) for _ in range(ncopy)]
            for d in dev[wt]:
                hip.set(d, w)
        for M in mlist:
            x = rng.standard_normal((M, K)).astype(np.float32)
            dx, dy = hip.alloc(x.nbytes), hip.alloc(4 * M * N)
            hip.set(dx, x)

            def slot(wt, n):
                for c in range(n):
                    L.tts_hip_gemv_ex(hip.ptr, wt, dev[wt][c % len(dev[wt])], dx, dy, K, N, M, 0)

            for wt in dev:
                slot(wt, 3)
            hip.sync()
            hip.set_option(ttship.OPT["PROFILE_GEMV"], 1)
            us = {"q8_0_a": [], "q5_0": [], "q8_0_b": []}
            for _ in range(rounds):
                for key, wt in (("q8_0_a", ttship.Q8_0), ("q5_0", ttship.Q5_0), ("q8_0_b", ttship.Q8_0)):
                    hip.gemv_stats(-1, reset=True)
                    slot(wt, reps)
                    ms, n, _ = hip.gemv_stats(wt, reset=True)
                    assert n == reps, (n, reps)
                    us[key].append(round(1000.0 * ms / n, 2))
            hip.set_option(ttship.OPT["PROFILE_GEMV"], 0)
            med = {k: float(np.median(v)) for k, v in us.items()}
            q8 = 0.5 * (med["q8_0_a"] + med["q8_0_b"])
            b8, b5 = ttship.row_size(ttship.Q8_0, K) * N, ttship.row_size(ttship.Q5_0, K) * N
            print(json.dumps({"K": K, "N": N, "M": M, "cold": cold, "reps": reps, "us_per_round": us, "median_us": med,
                              "q8_0_vs_q8_0_spread_us": round(max(abs(a - b) for a, b in zip(us["q8_0_a"], us["q8_0_b"])), 2),
                              "q5_0_over_q8_0": round(med["q5_0"] / q8, 3), "bytes_ratio": round(b5 / b8, 3),
                              "q8_0_weight_GBps": round(b8 / (q8 * 1e-6) / 1e9, 1),
                              "q5_0_weight_GBps": round(b5 / (med["q5_0"] * 1e-6) / 1e9, 1)}), flush=True)
            hip.free(dx)
            hip.free(dy)
        for ds in dev.values():
            for d in ds:
                hip.free(d)
    hip.close()


def compare_q4():
    """q4 mode: per (shape, M) and round the slots Q8_0, Q5_0, Q4_0, Q8_0 again."""
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    mlist = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1, 2, 8, 32]
    cold = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    hip = ttship.HipBackend(0)
    L = ttship.lib()
    rng = np.random.default_rng(0)
    types = (ttship.Q8_0, ttship.Q5_0, ttship.Q4_0)
    for K, N in Q5_SHAPES:
        dev = {}
        for wt in types:
            w = quant_bytes(rng, wt, K, N)
            # cold: as many copies of the SMALLEST (Q4_0) matrix as pass 512 MiB, the same count for every type, and
            # a type's launches go on through its copies from slot to slot and round to round: between two uses of
            # a copy at least 512 MiB of that type's own weights pass, twice the 256 MB last-level cache
            ncopy = -(-(512 << 20) // (ttship.row_size(ttship.Q4_0, K) * N)) if cold else 1
            dev[wt] = [hip.alloc(w.nbytes) for _ in range(ncopy)]
            for d in dev[wt]:
                hip.set(d, w)
        at = {wt: 0 for wt in types}
        for M in mlist:
            x = rng.standard_normal((M, K)).astype(np.float32)
            dx, dy = hip.alloc(x.nbytes), hip.alloc(4 * M * N)
            hip.set(dx, x)

            def slot(wt, n):
                for _ in range(n):
                    L.tts_hip_gemv_ex(hip.ptr, wt, dev[wt][at[wt] % len(dev[wt])], dx, dy, K, N, M, 0)
                    at[wt] += 1

            for wt in dev:
                slot(wt, 3)
            hip.sync()
            hip.set_option(ttship.OPT["PROFILE_GEMV"], 1)
            order = (("q8_0_a", ttship.Q8_0), ("q5_0", ttship.Q5_0), ("q4_0", ttship.Q4_0), ("q8_0_b", ttship.Q8_0))
            us = {key: [] for key, _ in order}
            for _ in range(rounds):
                for key, wt in order:
                    hip.gemv_stats(-1, reset=True)
                    slot(wt, reps)
                    ms, n, _ = hip.gemv_stats(wt, reset=True)
                    assert n == reps, (n, reps)
                    us[key].append(round(1000.0 * ms / n, 2))
            hip.set_option(ttship.OPT["PROFILE_GEMV"], 0)
            med = {k: float(np.median(v)) for k, v in us.items()}
            q8 = 0.5 * (med["q8_0_a"] + med["q8_0_b"])
            b4 = ttship.row_size(ttship.Q4_0, K) * N
            print(json.dumps({"K": K, "N": N, "M": M, "cold": cold, "copies": len(dev[ttship.Q4_0]), "reps": reps, "us_per_round": us, "median_us": med,
                              "q8_0_vs_q8_0_spread_us": round(max(abs(a - b) for a, b in zip(us["q8_0_a"], us["q8_0_b"])), 2),
                              "q8_0_vs_q8_0_margin": round(abs(med["q8_0_a"] - med["q8_0_b"]) / q8, 3),
                              "q4_0_over_q8_0": round(med["q4_0"] / q8, 3), "q4_0_over_q5_0": round(med["q4_0"] / med["q5_0"], 3),
                              "q5_0_over_q8_0": round(med["q5_0"] / q8, 3),
                              "q4_0_weight_GBps": round(b4 / (med["q4_0"] * 1e-6) / 1e9, 1)}), flush=True)
            hip.free(dx)
            hip.free(dy)
        for ds in dev.values():
            for d in ds:
                hip.free(d)
    hip.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "q5":
        return compare_q5()
    if len(sys.argv) > 1 and sys.argv[1] == "q4":
        return compare_q4()
    if len(sys.argv) > 1 and sys.argv[1] == "q6":
        return compare_q6()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    mlist = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 8]
    tiled = int(sys.argv[3]) if len(sys.argv) > 3 else 0  # 1: Q4_K in the tile layout (matrix-core kernel)
    only = sys.argv[4].split(",") if len(sys.argv) > 4 else None
    mr_tiles = None
    hip = ttship.HipBackend(0)
    dbg = int(sys.argv[6]) if len(sys.argv) > 6 else 0  # TTS_HIP_OPT_GEMV_DEBUG phase study
    hip.set_option(ttship.OPT["GEMV_DEBUG"], dbg)
    # cold: cycle through enough weight copies (>= 512 MiB) that every launch streams from HBM, as in a
    # decode step (the Infinity Cache holds 256 MiB); kernel selection from the environment
    cold = int(sys.argv[7]) if len(sys.argv) > 7 else 0
    for opt in ("GEMV_UNIQUE", "GEMV_KS"):
        if os.environ.get(opt) is not None:
            hip.set_option(ttship.OPT[opt], int(os.environ[opt]))
    L = ttship.lib()
    rng = np.random.default_rng(0)
    for name, wt, K, N in SHAPES:
        if only and name not in only:
            continue
        wbytes = ttship.row_size(wt, K) * N
        w = rng.integers(0, 256, size=wbytes, dtype=np.uint8)
        if wt == ttship.Q4_K:  # keep d/dmin finite: small fp16 in the block headers
            blk = w.reshape(-1, 144)
            blk[:, 0:2] = np.frombuffer(np.float16(1e-3).tobytes(), dtype=np.uint8)
            blk[:, 2:4] = np.frombuffer(np.float16(1e-3).tobytes(), dtype=np.uint8)
        elif wt == ttship.Q8_0:
            blk = w.reshape(-1, 34)
            blk[:, 0:2] = np.frombuffer(np.float16(1e-3).tobytes(), dtype=np.uint8)
        else:
            w = (rng.standard_normal(K * N).astype(np.float32) * 0.02).view(np.uint8)
        flags = 0
        if tiled and wt == ttship.Q4_K:  # random bytes are valid in any layout; only the flag matters
            flags = 32
            if N % 4:
                continue
        ncopy = max(1, min(64, -(-(512 << 20) // w.nbytes))) if cold else 1
        dws = [hip.alloc(w.nbytes) for _ in range(ncopy)]
        for d in dws:
            hip.set(d, w)
        for M in mlist:
            x = rng.standard_normal((M, K)).astype(np.float32)
            dx = hip.alloc(x.nbytes)
            dy = hip.alloc(4 * M * N)
            hip.set(dx, x)
            for c in range(3):
                L.tts_hip_gemv_ex(hip.ptr, wt, dws[c % ncopy], dx, dy, K, N, M, flags)
            hip.sync()
            hip.set_option(1, 1)
            hip.gemv_stats(-1, reset=True)
            for c in range(reps):
                L.tts_hip_gemv_ex(hip.ptr, wt, dws[c % ncopy], dx, dy, K, N, M, flags)
            ms, n, nbytes = hip.gemv_stats(wt, reset=True)
            hip.set_option(1, 0)
            us = 1000.0 * ms / n
            print(json.dumps({"shape": name, "type": ttship.lib().tts_type_name(wt).decode(), "K": K, "N": N, "M": M,
                              "weight_MB": round(wbytes / 1e6, 3), "tiled": bool(tiled and wt == ttship.Q4_K), "dbg": dbg, "cold": cold,
                              "avg_us": round(us, 2),
                              "GBps": round(nbytes / n / (us * 1e-6) / 1e9, 1)}), flush=True)
            hip.free(dx)
            hip.free(dy)
        for d in dws:
            hip.free(d)
    hip.close()


if __name__ == "__main__":
    main()
