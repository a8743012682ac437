"""Achieved TFLOP/s of the fused conv_1d launches of a DAC-44k decode, per (IC, OC, K, d), from a
rocprofv3 --kernel-trace CSV of scripts/bench_dac.py <frames> --default-only.

A launch is matched to its conv by its grid (64-position tiles x 64- or 96-channel tiles of k_conv1d_f64,
1024-position tiles x channels of k_conv1d_f64v) and, among the convs that share a grid (a block's residual
units: k7 d1, k1, k7 d3, k1, k7 d9, k1), by launch order.

  python3 scripts/dac_conv_table.py run_kernel_trace.csv 861 > table.md
"""
import collections
import csv
import sys

RATES = (8, 8, 4, 2)
LATENT, DIM = 1024, 1536


def dac_convs(T):
    """(name, IC, OC, K, d, OL) of every conv_1d of the decoder at T frames."""
    out = [("quantizer.out_proj", 8, LATENT, 1, 1, T)] * 9 + [("in", LATENT, DIM, 7, 1, T)]
    c, L = DIM, T
    for b, r in enumerate(RATES):
        c, L = c // 2, L * r
        for d in (1, 3, 9):
            out.append((f"b{b + 1}.ru.k7", c, c, 7, d, L))
            out.append((f"b{b + 1}.ru.k1", c, c, 1, 1, L))
    out.append(("out", c, 1, 7, 1, L))
    return out


def main():
    path, T = sys.argv[1], int(sys.argv[2])
    groups = collections.defaultdict(list)  # (OL, OC) -> its convs in launch order
    keys = {}                                # (kernel, grid x, grid y) -> (OL, OC)
    for cv in dac_convs(T):
        name, IC, OC, K, d, OL = cv
        groups[OL, OC].append(cv)
        keys["mfma64", (OL + 63) // 64 * 256, (OC + 63) // 64] = (OL, OC)
        if OC % 96 == 0:
            keys["mfma96", (OL + 63) // 64 * 256, OC // 96] = (OL, OC)
        keys["vfma", (OL + 1023) // 1024 * 256, OC] = (OL, OC)
    seen = collections.Counter()
    ns = collections.defaultdict(list)
    other = 0
    for row in csv.DictReader(open(path)):
        if "k_conv1d_f64" not in row["Kernel_Name"]:
            continue
        name = row["Kernel_Name"]  # k_conv1d_f64<W16, BIAS, RES, H32, MT>, k_conv1d_f64p<BIAS, RES, MT, XREG>: MT = 3 is the 96-row tile
        targs = name.split("(")[0].rstrip().rstrip(">").split("<")[-1].split(", ")
        mt = targs[2] if "k_conv1d_f64p" in name and len(targs) > 3 else targs[-1]
        kind = "vfma" if "k_conv1d_f64v" in name else "mfma96" if mt == "3" else "mfma64"
        g = keys.get((kind, int(row["Grid_Size_X"]), int(row["Grid_Size_Y"])))
        dur = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
        if g is not None:
            ns[groups[g][seen[g] % len(groups[g])]].append(dur)
            seen[g] += 1
        else:
            other += dur
    print("| conv | IC | OC | K | d | OL | launches | median us | GFLOP | TFLOP/s | share of conv time |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    total = sum(sum(v) for v in ns.values()) + other
    for (name, IC, OC, K, d, OL), v in sorted(ns.items(), key=lambda kv: -sum(kv[1])):
        v.sort()
        med = v[len(v) // 2]
        fl = 2.0 * IC * OC * K * OL
        print(f"| {name} | {IC} | {OC} | {K} | {d} | {OL} | {len(v)} | {med / 1e3:.1f} | {fl / 1e9:.2f} | {fl / med / 1e3:.1f} | {100 * sum(v) / total:.1f} % |")
    print(f"\nunmatched conv1d launches: {other / 1e3:.1f} us of {total / 1e3:.1f} us")
    convt_table(path, T)


def convt_table(path, T):
    """The transposed-conv launches (k_convt_f64_lds / k_convt_f64_img: 64-position x 32-channel workgroup tiles over
    L + 1 polyphase positions) per (IC, OC, S), matched by their grid in workgroups."""
    keys, c, L = {}, DIM, T
    for b, r in enumerate(RATES):
        keys[(L + 1 + 63) // 64, (c // 2 + 31) // 32] = (f"b{b + 1}.convt", c, c // 2, r, L)
        c, L = c // 2, L * r
    ns = collections.defaultdict(list)
    for row in csv.DictReader(open(path)):
        if "k_convt_f64" not in row["Kernel_Name"]:
            continue
        g = keys.get((int(row["Grid_Size_X"]) // int(row["Workgroup_Size_X"]), int(row["Grid_Size_Y"])))
        if g is not None:
            ns[g + (row["Kernel_Name"].split("(")[0].replace("void tts::", ""),)].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    print("\n| transposed conv | kernel | IC | OC | S | L | launches | median us | GFLOP | TFLOP/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (name, IC, OC, S, L, kern), v in sorted(ns.items()):
        v.sort()
        med = v[len(v) // 2]
        fl = 2.0 * IC * OC * 2 * S * L
        print(f"| {name} | `{kern}` | {IC} | {OC} | {S} | {L} | {len(v)} | {med / 1e3:.1f} | {fl / 1e9:.2f} | {fl / med / 1e3:.1f} |")


if __name__ == "__main__":
    main()
