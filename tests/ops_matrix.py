"""The declared case list of the generic op kernels (k_ops.hip), shared by test_supports_op_cpu.py,
test_ops_ref_cpu.py and test_ops_strided_gpu.py.

A case is one small graph: `build(g)` adds it to a nodes.Graph and returns the tensor(s) to compare.  `expect`
says what tts_hip_supports_op must answer for the case's last node: "run" cases execute (on the device, on the
oracle, on ops_ref); "refuse" cases are only ever shown to supports_op -- a quantized operand read through
td_load could leave its buffer.  `bar` is the comparison against ops_ref:

  "bits"  bit equality: moves and the singly rounded ops (numpy float32 arithmetic is IEEE);
  "ulp1"  at most 1 ulp of the f32 result and at least 99.9 % of the elements bit-equal: the transcendental
          ops (both sides round one f64 value whose error is ~2^-52 relative, so they part only across an
          f32 rounding midpoint) and the reductions (an f64 sum of <= 257 terms is off by < 2^-44 relative).

NaN results compare as "NaN in the same places".  `oracle` is False where the oracle does not implement the
case (none today).  Shapes are tiny: every dim <= 8 but ne0, and ne0 from {1, 3, 63, 64, 65, 257} -- below, on
and above the 64-lane wave and the 256-thread block of the row kernels -- except the cases past the grid caps.
"""
import numpy as np

import chains
import ttship

F32, F16, I32 = ttship.F32, ttship.F16, ttship.I32
Q8_0, Q4_K = ttship.Q8_0, ttship.Q4_K
NP = {F32: np.float32, F16: np.float16, I32: np.int32}
ES = {F32: 4, F16: 2, I32: 4}
TN = {F32: "f32", F16: "f16", I32: "i32"}
U = ttship.UNARY

INF, NAN = np.inf, np.nan
FLT_MAX = np.float32(3.4028235e38)
MIN_NORMAL = np.array([0x00800000], np.uint32).view(np.float32)[0]
MAX_SUBNORMAL = np.array([0x007FFFFF], np.uint32).view(np.float32)[0]
MIN_SUBNORMAL = np.array([0x00000001], np.uint32).view(np.float32)[0]
EDGE = np.array([0.0, -0.0, INF, -INF, NAN, MIN_NORMAL, MAX_SUBNORMAL, MIN_SUBNORMAL, FLT_MAX, -FLT_MAX], np.float32)
FINITE_EDGE = EDGE[np.isfinite(EDGE)]
# F32 -> F16 stores: the largest f16, just under / on the overflow midpoint, ties to even and to odd in the
# normal range, the smallest f16 subnormal, half of it (a tie to zero) and just above that (rounds up)
TO_F16 = np.array([65504.0, 65519.996, 65520.0, 1 + 2.0**-11, 1 + 3 * 2.0**-11, 2.0**-24, 2.0**-25,
                   2.0**-25 * (1 + 2.0**-10)], np.float32)
TO_F16 = np.concatenate([TO_F16, -TO_F16])
I32_EDGE = np.array([0, -1, 2**24 + 1, 2**31 - 1, -2**31], np.int32)
F16_SUBNORMAL = np.array([2.0**-24, 3 * 2.0**-24, 2.0**-15, -2.0**-16, 2.0**-14 - 2.0**-24], np.float32)
EXTRA = {
    "ROUND": [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, 8388609.0],
    "MOD": [-5.5, -0.25, -7.0, 5.5, 3.0e9],
    "GELU": [10.0, -10.0, np.nextafter(np.float32(10), np.float32(0)), np.nextafter(np.float32(10), np.float32(20)),
             np.nextafter(np.float32(-10), np.float32(0)), np.nextafter(np.float32(-10), np.float32(-20)), 9.996, -9.996,
             *F16_SUBNORMAL],
    "EXP": [-104.0, -87.4, 88.7, 89.0],
    "SIGMOID": [20.0, -20.0, 100.0, -100.0],
    "TANH": [20.0, -20.0, 100.0, -100.0],
    "SILU": [20.0, -20.0, 100.0, -100.0],
    "SIN": [1.0e5, 1.0e8],
    "COS": [1.0e5, 1.0e8],
}
NE0 = (1, 3, 63, 64, 65, 257)


class Case:
    def __init__(self, group, name, build, expect="run", bar="bits", oracle=True):
        self.group, self.name, self.build, self.expect, self.bar, self.oracle = group, name, build, expect, bar, oracle
        self.id = f"{group}-{name}"


CASES = []


def case(group, name, expect="run", bar="bits", oracle=True):
    def deco(fn):
        CASES.append(Case(group, name, fn, expect, bar, oracle))
        return fn
    return deco


# ---- inputs --------------------------------------------------------------------------------------------------
def values(seed, ne, first=(), scale=1.0, shift=0.0):
    """Gaussian draws of logical shape ne, the values of `first` at the front (as many as fit)."""
    n = int(np.prod(ne))
    v = (np.random.default_rng(seed).standard_normal(n) * scale + shift).astype(np.float32)
    f = np.asarray(first, np.float32).reshape(-1)[:n]
    v[:len(f)] = f
    return v.reshape(list(ne)[::-1])


def ints(seed, ne):
    n = int(np.prod(ne))
    v = np.random.default_rng(seed).integers(-2**31, 2**31 - 1, size=n).astype(np.int32)
    v[:min(n, len(I32_EDGE))] = I32_EDGE[:n]
    return v.reshape(list(ne)[::-1])


def pairs(seed, ne):
    """Two arrays whose first len(EDGE)^2 elements walk every (edge, edge) pair: inf - inf, 0 * inf, x / 0, 0 / 0 ..."""
    L = len(EDGE)
    k = np.arange(L * L)
    return values(seed, ne, EDGE[k % L]), values(seed + 1, ne, EDGE[k // L], shift=2.0)


# ---- layouts: a tensor whose logical content is `arr` (numpy shape = ne reversed) ------------------------------
def lay(g, arr, typ=F32, layout="cont"):
    with np.errstate(over="ignore"):      # FLT_MAX into an F16 leaf is inf on purpose
        arr = np.ascontiguousarray(arr.astype(NP[typ]))
    arr = arr.reshape((1,) * (4 - arr.ndim) + arr.shape)
    es = ES[typ]
    ne = list(arr.shape[::-1])
    if layout == "cont":
        return g.leaf(arr, typ=typ)
    if layout == "perm":        # permute(0, 2, 1, 3)
        return g.permute(g.leaf(arr.swapaxes(1, 2), typ=typ), (0, 2, 1, 3))
    if layout == "transpose":
        return g.transpose(g.leaf(arr.swapaxes(2, 3), typ=typ))
    if layout == "pad":         # rows 1.5 x as long as their data; the slack holds a sentinel
        assert ne[0] % 2 == 0
        wide = np.full(arr.shape[:3] + (ne[0] * 3 // 2,), 7, NP[typ])
        wide[..., :ne[0]] = arr
        t = g.leaf(wide, typ=typ)
        return g.view(t, ne, [t.nb[i] for i in range(4)])
    if layout == "off4":        # a dense view 4 bytes into its buffer: 4-byte, not 16-byte, aligned
        assert ne[0] % 4 == 0
        lead = 4 // es
        flat = np.concatenate([np.full(lead, 7, NP[typ]), arr.reshape(-1), np.full(8, 7, NP[typ])])
        t = g.leaf(flat, typ=typ)
        return g.view(t, ne, [es, es * ne[0], es * ne[0] * ne[1], es * ne[0] * ne[1] * ne[2]], offs=4)
    raise KeyError(layout)


def padded_nb(ne, typ):
    es = ES[typ]
    nb1 = (es * ne[0] * 3 // 2 + 3) // 4 * 4
    return [es, nb1, nb1 * ne[1], nb1 * ne[1] * ne[2] + 16]


def out_node(g, op, typ, ne, srcs, dst="cont", **kw):
    """dst: "cont", "dpad" (a destination with its own padded strides) or "inplace" (on src0's bytes)."""
    ne = list(ne) + [1] * (4 - len(ne))
    if dst == "dpad":
        return g.node(op, typ, ne, srcs, nb=padded_nb(ne, typ), **kw)
    if dst == "inplace":
        return g.node(op, typ, ne, srcs, nb=[srcs[0].nb[i] for i in range(4)], on=(srcs[0], 0), **kw)
    return g.node(op, typ, ne, srcs, **kw)


def ne_of(t):
    return [int(t.ne[i]) for i in range(4)]


SRC_LAYOUTS = ("cont", "perm", "transpose", "pad", "off4")
A_NE = [6, 4, 3, 2]


# ---- copies: DUP / CONT / CPY ----------------------------------------------------------------------------------
def _copy_cases():
    ne = [8, 4, 3, 2]
    for op in ("DUP", "CONT", "CPY"):
        for st, dt in ((F32, F32), (F32, F16), (F16, F32), (F16, F16), (I32, I32)):
            for layout in SRC_LAYOUTS:
                for dst in ("cont", "dpad"):
                    if op != "CONT" and (layout in ("transpose", "off4") or (st, dt) == (F16, F16)) and dst == "cont":
                        continue        # DUP and CPY walk the same kernel as CONT: a thinner cut of the grid
                    @case("copy", f"{op}-{TN[st]}-{TN[dt]}-{layout}-{dst}")
                    def _(g, op=op, st=st, dt=dt, layout=layout, dst=dst):
                        arr = ints(1, ne) if st == I32 else values(2, ne, np.concatenate([EDGE, TO_F16]), scale=3.0)
                        s = lay(g, arr, st, layout)
                        if op != "CPY":
                            return out_node(g, op, dt, ne_of(s), [s], dst)
                        cache = g.leaf(np.zeros((2, int(np.prod(ne)) * 2), NP[dt]), typ=dt)   # cpy(a, b): the node is b's view
                        nb = padded_nb(ne_of(s), dt) if dst == "dpad" else None
                        es = ES[dt]
                        n4 = ne_of(s)
                        nb = nb or [es, es * n4[0], es * n4[0] * n4[1], es * n4[0] * n4[1] * n4[2]]
                        dv = g.view(cache, n4, nb, offs=8)
                        return g.node("CPY", dt, n4, [s, dv], nb=nb, on=(dv, 0))
    for st, dt in ((F32, F32), (F32, F16), (I32, I32)):
        for layout in ("cont", "perm"):
            for op in ("CONT", "DUP"):
                @case("copy", f"{op}-reshape-{TN[st]}-{TN[dt]}-{layout}")
                def _(g, op=op, st=st, dt=dt, layout=layout):
                    arr = ints(3, ne) if st == I32 else values(4, ne, EDGE)
                    return g.node(op, dt, [12, 16, 1, 1], [lay(g, arr, st, layout)])   # same nel, another ne

            @case("copy", f"CPY-reshape-{TN[st]}-{TN[dt]}-{layout}")
            def _(g, st=st, dt=dt, layout=layout):
                arr = ints(3, ne) if st == I32 else values(4, ne, EDGE)
                cache = g.leaf(np.zeros((3, 64), NP[dt]), typ=dt)
                es = ES[dt]
                dv = g.view(cache, [3, 64, 1, 1], [es, es * 3, es * 192, es * 192])
                return g.node("CPY", dt, [3, 64, 1, 1], [lay(g, arr, st, layout), dv], on=(dv, 0))


_copy_cases()


# ---- binary ----------------------------------------------------------------------------------------------------
B_NES = ([6, 4, 3, 2], [6, 1, 1, 1], [1, 4, 1, 1], [1, 1, 3, 1], [1, 1, 1, 2], [6, 4, 1, 1], [6, 4, 1, 2], [1, 4, 3, 1],
         [3, 2, 1, 1], [1, 1, 1, 1])


def _binary_cases():
    for op in ("ADD", "SUB", "MUL", "DIV"):
        for bne in B_NES:
            for layout in ("cont", "perm"):
                @case("binary", f"{op}-b{'x'.join(map(str, bne))}-{layout}")
                def _(g, op=op, bne=bne, layout=layout):
                    a, bfull = pairs(10, A_NE)
                    b = bfull[:bne[3], :bne[2], :bne[1], :bne[0]] if bne != A_NE else bfull
                    ta = lay(g, a, F32, layout)
                    return out_node(g, op, F32, A_NE, [ta, g.leaf(np.ascontiguousarray(b))])
        for ta_, tb_, td_ in ((F16, F32, F32), (F32, F16, F32), (F32, F32, F16), (F16, F16, F16)):
            @case("binary", f"{op}-{TN[ta_]}-{TN[tb_]}-{TN[td_]}")
            def _(g, op=op, ta_=ta_, tb_=tb_, td_=td_):
                a, b = pairs(12, A_NE)
                return out_node(g, op, td_, A_NE, [lay(g, a, ta_), lay(g, b, tb_)])
        for la, lb, dst in (("pad", "cont", "cont"), ("cont", "pad", "cont"), ("transpose", "cont", "cont"),
                            ("cont", "perm", "dpad"), ("cont", "cont", "dpad"), ("cont", "cont", "inplace"),
                            ("perm", "cont", "inplace"), ("pad", "pad", "inplace")):
            @case("binary", f"{op}-a_{la}-b_{lb}-{dst}")
            def _(g, op=op, la=la, lb=lb, dst=dst):
                a, b = pairs(14, A_NE)
                return out_node(g, op, F32, A_NE, [lay(g, a, F32, la), lay(g, b, F32, lb)], dst)
        # the row broadcast of a per-row scalar (k_binary_rowbc): 4 per lane on 16-byte aligned rows of a multiple
        # of 4, else the scalar form -- on a view 4 bytes in, on ne0 = 63, and one column short of the predicate
        for name, ane, bne, layout in (("rowbc-v4", [64, 4], [1, 4], "cont"), ("rowbc-off4", [64, 4], [1, 4], "off4"),
                                       ("rowbc-odd", [63, 4], [1, 4], "cont"), ("rowbc-one", [64, 4], [1, 1], "cont"),
                                       ("rowbc-3d", [64, 4, 2], [1, 4, 1], "cont"), ("rowbc-miss", [64, 4, 2], [1, 4, 2], "cont"),
                                       ("fast-row", [64, 4, 2], [64, 1, 1], "cont"), ("fast-off4", [64, 4, 2], [64, 4, 1], "off4")):
            @case("binary", f"{op}-{name}")
            def _(g, op=op, ane=ane, bne=bne, layout=layout):
                a = values(16, ane, EDGE)
                b = values(17, bne, [0.0, INF, 2.5, -1.5], shift=2.0)
                return out_node(g, op, F32, ane, [lay(g, a, F32, layout), g.leaf(b)])


_binary_cases()


# ---- unary maps ------------------------------------------------------------------------------------------------
MAPS = (("SQR", {}), ("SQRT", {}), ("SIN", {}), ("COS", {}), ("SCALE", {0: 0.37}), ("CLAMP", {0: -0.5, 1: 0.75}),
        ("LEAKY_RELU", {0: 0.2}), ("ROUND", {}), ("MOD", {0: 1.75}))
TRANSC = ("SIN", "COS", "TANH", "SIGMOID", "SILU", "EXP")


def _unary_node(g, name, s, typ, dst):
    if name in U:
        return out_node(g, "UNARY", typ, ne_of(s), [s], dst, params=[U[name]])
    return out_node(g, name, typ, ne_of(s), [s], dst, fparams=dict(MAPS)[name])


def _unary_cases():
    ne = [8, 4, 3, 2]
    names = [m for m, _ in MAPS] + list(U)
    for name in names:
        bar = "ulp1" if name in TRANSC else "bits"
        combos = [(F32, F32, layout, "cont") for layout in SRC_LAYOUTS]
        combos += [(F32, F32, "cont", "dpad"), (F32, F32, "cont", "inplace"), (F32, F32, "perm", "inplace"),
                   (F16, F32, "cont", "cont"), (F32, F16, "cont", "cont"), (F16, F16, "perm", "dpad")]
        for st, dt, layout, dst in combos:
            @case("unary", f"{name}-{TN[st]}-{TN[dt]}-{layout}-{dst}", bar=bar)
            def _(g, name=name, st=st, dt=dt, layout=layout, dst=dst):
                first = np.concatenate([EDGE, np.asarray(EXTRA.get(name, []), np.float32), TO_F16 if dt == F16 else []])
                return _unary_node(g, name, lay(g, values(20, ne, first, scale=3.0), st, layout), dt, dst)
        for n0 in NE0:
            @case("unary", f"{name}-ne0_{n0}", bar=bar)
            def _(g, name=name, n0=n0):
                return _unary_node(g, name, g.leaf(values(21, [n0, 3], EDGE, scale=3.0)), F32, "cont")

    @case("unary", "GELU-every-f16")
    def _(g):
        h = np.arange(65536, dtype=np.uint16).view(np.float16)
        x = h[np.isfinite(h)].astype(np.float32)
        return _unary_node(g, "GELU", g.leaf(x), F32, "cont")


_unary_cases()


# ---- NORM / RMS_NORM -------------------------------------------------------------------------------------------
def _norm_cases():
    for op in ("NORM", "RMS_NORM"):
        for n0 in NE0:
            for layout, dst in (("cont", "cont"), ("perm", "cont"), ("cont", "inplace")):
                @case("norm", f"{op}-ne0_{n0}-{layout}-{dst}", bar="ulp1")
                def _(g, op=op, n0=n0, layout=layout, dst=dst):
                    x = values(30, [n0, 4, 3, 2], FINITE_EDGE[:6], shift=0.25)
                    return out_node(g, op, F32, [n0, 4, 3, 2], [lay(g, x, F32, layout)], dst, fparams={0: 1e-5})
        for layout, dst in (("pad", "cont"), ("off4", "cont"), ("cont", "dpad"), ("pad", "inplace"), ("perm", "inplace"),
                            ("pad", "dpad")):
            @case("norm", f"{op}-ne0_64-{layout}-{dst}", bar="ulp1")
            def _(g, op=op, layout=layout, dst=dst):
                x = values(31, [64, 4, 3, 2], FINITE_EDGE[:6], shift=0.25)
                return out_node(g, op, F32, [64, 4, 3, 2], [lay(g, x, F32, layout)], dst, fparams={0: 1e-5})


_norm_cases()


# ---- SUM_ROWS --------------------------------------------------------------------------------------------------
def _sum_rows_cases():
    for n0 in NE0:
        for st, dt, layout in ((F32, F32, "cont"), (F16, F32, "cont"), (F32, F32, "perm"), (F16, F16, "perm"),
                               (F32, F16, "transpose")):
            @case("sum_rows", f"ne0_{n0}-{TN[st]}-{TN[dt]}-{layout}", bar="ulp1")
            def _(g, n0=n0, st=st, dt=dt, layout=layout):
                ne = [n0, 4, 3, 2]
                s = lay(g, values(40, ne, FINITE_EDGE[:6], scale=2.0), st, layout)
                return out_node(g, "SUM_ROWS", dt, [1] + ne_of(s)[1:], [s])
    for layout, dst in (("pad", "cont"), ("off4", "cont"), ("cont", "dpad")):
        @case("sum_rows", f"ne0_64-{layout}-{dst}", bar="ulp1")
        def _(g, layout=layout, dst=dst):
            s = lay(g, values(41, [64, 4, 3, 2], scale=2.0), F32, layout)
            if dst == "dpad":
                return g.node("SUM_ROWS", F32, [1, 4, 3, 2], [s], nb=[4, 12, 60, 200])
            return out_node(g, "SUM_ROWS", F32, [1, 4, 3, 2], [s])


_sum_rows_cases()


# ---- SOFT_MAX --------------------------------------------------------------------------------------------------
def _mask(seed, ne):
    """0 / -inf with row 1 fully masked and never a fully masked row 0."""
    m = np.where(np.random.default_rng(seed).random(ne[::-1]) < 0.3, -INF, 0.0).astype(np.float32)
    m[..., 0, 0] = 0.0
    if ne[1] > 1:
        m[..., 1, :] = -INF
    return m


def _soft_max_cases():
    for nc in (1, 77, 257):
        for mk in ("none", "f32", "f16", "tall", "4d"):
            for dst in ("cont", "inplace"):
                @case("soft_max", f"nc{nc}-mask_{mk}-{dst}", bar="ulp1")
                def _(g, nc=nc, mk=mk, dst=dst):
                    ne = [nc, 4, 3, 2]
                    srcs = [g.leaf(values(50, ne, FINITE_EDGE[:6], scale=3.0))]
                    if mk != "none":
                        mne = {"f32": [nc, 4], "f16": [nc, 4], "tall": [nc, 7], "4d": [nc, 4, 3, 2]}[mk]
                        srcs.append(lay(g, _mask(51, mne), F16 if mk == "f16" else F32))
                    return out_node(g, "SOFT_MAX", F32, ne, srcs, dst, fparams={0: 0.125 if nc > 1 else 1.0, 1: 0.0})

    @case("soft_max", "mask-3d-broadcast", bar="ulp1")
    def _(g):     # a mask per sequence (ne3), one for all heads (ne2)
        srcs = [g.leaf(values(52, [77, 4, 3, 2], scale=3.0)), g.leaf(_mask(53, [77, 5, 1, 2]))]
        return out_node(g, "SOFT_MAX", F32, [77, 4, 3, 2], srcs, fparams={0: 0.5, 1: 0.0})


_soft_max_cases()


# ---- GET_ROWS --------------------------------------------------------------------------------------------------
def _get_rows_cases():
    for tt in (F32, F16):
        for nc in (3, 64, 257):
            @case("get_rows", f"2d-{TN[tt]}-nc{nc}")
            def _(g, tt=tt, nc=nc):
                tab = lay(g, values(60, [nc, 7], EDGE), tt)
                idx = g.leaf(np.array([0, 6, 6, 3, 0, 6], np.int32), typ=I32)
                return g.node("GET_ROWS", F32, [nc, 6], [tab, idx])

        @case("get_rows", f"3d-{TN[tt]}")
        def _(g, tt=tt):     # ne11 = 3, ne12 = 2: the index's dims 1 / 2 pick the table's dims 2 / 3
            tab = lay(g, values(61, [65, 5, 3, 2], EDGE), tt)
            idx = g.leaf(np.array([[[0, 4, 4, 1], [4, 0, 2, 2], [3, 3, 0, 4]], [[4, 4, 4, 4], [0, 0, 0, 0], [1, 2, 3, 4]]], np.int32), typ=I32)
            return g.node("GET_ROWS", F32, [65, 4, 3, 2], [tab, idx])

        @case("get_rows", f"strided-index-{TN[tt]}")
        def _(g, tt=tt):     # every second entry of an index buffer: nb[0] = 8
            tab = lay(g, values(62, [64, 7], EDGE), tt)
            buf = g.leaf(np.array([6, 99, 0, 99, 3, 99, 6, 99, 1, 99], np.int32), typ=I32)
            idx = g.view(buf, [5, 1, 1, 1], [8, 40, 40, 40])
            return g.node("GET_ROWS", F32, [64, 5], [tab, idx])

        @case("get_rows", f"padded-table-dpad-{TN[tt]}")
        def _(g, tt=tt):
            tab = lay(g, values(63, [64, 7], EDGE), tt, "pad")
            idx = g.leaf(np.array([6, 0, 3], np.int32), typ=I32)
            return g.node("GET_ROWS", F32, [64, 3], [tab, idx], nb=padded_nb([64, 3, 1, 1], F32))


_get_rows_cases()


# ---- CONCAT / REPEAT -------------------------------------------------------------------------------------------
def _concat_repeat_cases():
    ane = [5, 4, 3, 2]
    for dim in range(4):
        bne = list(ane)
        bne[dim] = ane[dim] + 2          # unequal parts
        one = [ane[i] + (bne[i] if i == dim else 0) for i in range(4)]
        for ta_, tb_, td_, lb in ((F32, F32, F32, "cont"), (F32, F32, F32, "perm"), (F16, F32, F32, "cont"),
                                  (F32, F16, F16, "perm"), (F16, F16, F16, "cont"), (I32, I32, I32, "cont"),
                                  (I32, I32, I32, "perm")):
            for dst in ("cont", "dpad"):
                if dst == "dpad" and lb == "perm":
                    continue

                @case("concat", f"dim{dim}-{TN[ta_]}-{TN[tb_]}-{TN[td_]}-b_{lb}-{dst}")
                def _(g, dim=dim, bne=bne, one=one, ta_=ta_, tb_=tb_, td_=td_, lb=lb, dst=dst):
                    a = ints(70, ane) if ta_ == I32 else values(71, ane, EDGE)
                    b = ints(72, bne)[..., ::-1].copy() if tb_ == I32 else values(73, bne, EDGE[::-1])
                    return out_node(g, "CONCAT", td_, one, [lay(g, a, ta_), lay(g, b, tb_, lb)], dst, params=[dim])
        for la, lb in (("perm", "cont"), ("transpose", "perm")):
            @case("concat", f"dim{dim}-f32-a_{la}-b_{lb}")
            def _(g, dim=dim, bne=bne, one=one, la=la, lb=lb):
                srcs = [lay(g, values(77, ane, EDGE), F32, la), lay(g, values(78, bne, EDGE[::-1]), F32, lb)]
                return out_node(g, "CONCAT", F32, one, srcs, params=[dim])
    for la in ("pad", "off4"):
        @case("concat", f"dim1-f32-a_{la}-b_{la}")
        def _(g, la=la):
            srcs = [lay(g, values(77, [8, 4, 3, 2], EDGE), F32, la), lay(g, values(78, [8, 2, 3, 2]), F32, la)]
            return out_node(g, "CONCAT", F32, [8, 6, 3, 2], srcs, params=[1])
    reps = ([2, 1, 1, 1], [1, 3, 1, 1], [1, 1, 2, 1], [1, 1, 1, 3], [2, 1, 3, 1], [1, 2, 1, 2])
    for rep in reps:
        for st, dt, layout in ((F32, F32, "cont"), (F32, F32, "perm"), (F16, F32, "cont"), (F32, F16, "cont"),
                               (F16, F16, "perm"), (I32, I32, "cont"), (I32, I32, "perm")):
            @case("repeat", f"x{'x'.join(map(str, rep))}-{TN[st]}-{TN[dt]}-{layout}")
            def _(g, rep=rep, st=st, dt=dt, layout=layout):
                sne = [5, 2, 2, 2]
                s = ints(74, sne) if st == I32 else values(75, sne, np.concatenate([EDGE, TO_F16]))
                return out_node(g, "REPEAT", dt, [sne[i] * rep[i] for i in range(4)], [lay(g, s, st, layout)])

    @case("repeat", "f32-dpad")
    def _(g):
        return out_node(g, "REPEAT", F32, [12, 4, 1, 1], [g.leaf(values(76, [6, 2], EDGE))], "dpad")


_concat_repeat_cases()


# ---- ROPE ------------------------------------------------------------------------------------------------------
def _rope_node(g, x, n_dims, mode, ff=None, freq_scale=1.0, attn=1.0, dst="cont", pos=(0, 1, 4095), ext=0.0,
               typ=F32, nb=None, base=10000.0):
    ne = ne_of(x)
    srcs = [x, g.leaf(np.asarray(pos, np.int32), typ=I32)]
    if ff is not None:
        srcs.append(g.leaf(ff))
    kw = dict(params=[0, n_dims, mode, 0, 4096], fparams={5: base, 6: freq_scale, 7: ext, 8: attn})
    if nb is not None:
        return g.node("ROPE", typ, ne, srcs, nb=nb, **kw)
    return out_node(g, "ROPE", typ, ne, srcs, dst, **kw)


def _rope_cases():
    for mode in (0, 2):
        for n0 in (64, 256):
            for nd_ in (n0, n0 // 2):
                for ffs in (False, True):
                    @case("rope", f"mode{mode}-ne0_{n0}-ndims{nd_}-{'ff' if ffs else 'noff'}", bar="ulp1")
                    def _(g, mode=mode, n0=n0, nd_=nd_, ffs=ffs):
                        x = lay(g, values(80, [n0, 3, 3, 2]))
                        ff = np.linspace(1.0, 8.0, nd_ // 2).astype(np.float32) if ffs else None
                        return _rope_node(g, x, nd_, mode, ff)
        for name, kw, layout in (("freq_scale", dict(freq_scale=0.5), "cont"), ("attn_factor", dict(attn=1.25), "cont"),
                                 ("both", dict(freq_scale=0.5, attn=1.25, base=500000.0), "cont"), ("perm", {}, "perm"),
                                 ("pad", {}, "pad"), ("off4", {}, "off4"), ("inplace", dict(dst="inplace"), "cont"),
                                 ("perm-inplace", dict(dst="inplace"), "perm"), ("dpad", dict(dst="dpad"), "cont")):
            @case("rope", f"mode{mode}-{name}", bar="ulp1")
            def _(g, mode=mode, kw=kw, layout=layout):
                x = lay(g, values(81, [64, 3, 3, 2]), F32, layout)
                return _rope_node(g, x, 32, mode, np.linspace(1.0, 4.0, 16).astype(np.float32), **kw)


_rope_cases()


# ---- past the grid caps ----------------------------------------------------------------------------------------
N_BIG = 65536 * 256 + 1025        # = 3609 * 4649: past grid_for's 65536 blocks of 256
N_MID = 4096 * 256                # k_cpy_multi and k_repeat_interleave1 cap at 4096 blocks of 256


@case("big", "ADD-cont")
def _(g):
    a = values(90, [N_BIG])
    return g.node("ADD", F32, [N_BIG], [g.leaf(a), g.leaf(a[::-1].copy())])


@case("big", "CPY-transposed")
def _(g):
    s = g.transpose(g.leaf(values(91, [3609, 4649])))
    cache = g.leaf(np.zeros(N_BIG, np.float32))
    dv = g.view(cache, [4649, 3609, 1, 1], [4, 4 * 4649, 4 * N_BIG, 4 * N_BIG])
    return g.node("CPY", F32, [4649, 3609, 1, 1], [s, dv], on=(dv, 0))


@case("big", "MCPY-chain")
def _(g):       # hd * nkv = 1048592 > N_MID source elements into two interleaved cache views
    return chains.mcpy(g, hd=65537, nkv=16, rep=2)


@case("big", "RINT-chain")
def _(g):       # n0 * n1 * r * n2 = 1048640 > N_MID destination elements
    return chains.rint(g, n0=16385, n1=4, n2=4, r=4)


# ---- what supports_op must refuse (never run) --------------------------------------------------------------------
def _quant(g, typ, ne):
    n = ttship.TYPE_SIZE[typ] * (ne[0] // ttship.BLCK_SIZE[typ]) * int(np.prod(ne[1:]))
    return g.leaf(raw=np.zeros(n, np.uint8), typ=typ, ne=ne)


def _refusals():
    R = "refuse"
    for qt, qn in ((Q8_0, "q8_0"), (Q4_K, "q4_K")):
        ne = [256, 4]
        for op in ("ADD", "SUB", "MUL", "DIV"):
            @case(R, f"{op}-src0-{qn}", expect=R)
            def _(g, op=op, qt=qt):
                return g.node(op, F32, ne, [_quant(g, qt, ne), g.leaf(values(1, ne))])

            @case(R, f"{op}-src1-{qn}", expect=R)
            def _(g, op=op, qt=qt):
                return g.node(op, F32, ne, [g.leaf(values(1, ne)), _quant(g, qt, ne)])

            @case(R, f"{op}-dst-{qn}", expect=R)
            def _(g, op=op, qt=qt):
                return g.node(op, qt, ne, [g.leaf(values(1, ne)), g.leaf(values(2, ne))])
        for name in [m for m, _ in MAPS] + list(U):
            @case(R, f"{name}-src-{qn}", expect=R)
            def _(g, name=name, qt=qt):
                return _unary_node(g, name, _quant(g, qt, ne), F32, "cont")
        @case(R, f"CONCAT-src0-{qn}", expect=R)
        def _(g, qt=qt):
            return g.node("CONCAT", F32, [256, 8], [_quant(g, qt, ne), g.leaf(values(1, ne))], params=[1])

        @case(R, f"CONCAT-src1-{qn}", expect=R)
        def _(g, qt=qt):
            return g.node("CONCAT", F32, [256, 8], [g.leaf(values(1, ne)), _quant(g, qt, ne)], params=[1])

        @case(R, f"REPEAT-src-{qn}", expect=R)
        def _(g, qt=qt):
            return g.node("REPEAT", F32, [256, 8], [_quant(g, qt, ne)])

        @case(R, f"SUM_ROWS-src-{qn}", expect=R)
        def _(g, qt=qt):
            return g.node("SUM_ROWS", F32, [1, 4], [_quant(g, qt, ne)])

    x_ne = [64, 3, 3, 2]
    @case(R, "ROPE-ext_factor", expect=R)
    def _(g):
        return _rope_node(g, g.leaf(values(1, x_ne)), 64, 2, ext=1.0)
    for mode in (1, 4, 8, 10, 24):       # bits outside {0, 2}: GLM's bit 0, mrope 8, vision 24 ...
        @case(R, f"ROPE-mode{mode}", expect=R)
        def _(g, mode=mode):
            return _rope_node(g, g.leaf(values(1, x_ne)), 64, mode)

    @case(R, "SOFT_MAX-max_bias", expect=R)
    def _(g):
        return g.node("SOFT_MAX", F32, [77, 4], [g.leaf(values(1, [77, 4])), g.leaf(_mask(2, [77, 4]))], fparams={0: 1.0, 1: 8.0})
    for layout in ("perm", "transpose", "pad"):
        @case(R, f"SOFT_MAX-src-{layout}", expect=R)
        def _(g, layout=layout):
            s = lay(g, values(1, [64, 4, 3, 2]), F32, layout)
            return g.node("SOFT_MAX", F32, ne_of(s), [s], fparams={0: 1.0, 1: 0.0})

    @case(R, "SOFT_MAX-dst-padded", expect=R)
    def _(g):     # k_soft_max takes row r at r * nb[1] of the destination too
        return out_node(g, "SOFT_MAX", F32, [64, 4, 3, 2], [g.leaf(values(1, [64, 4, 3, 2]))], "dpad", fparams={0: 1.0, 1: 0.0})

    def row_op(g, op, typ, nb):
        ne = [64, 3, 3, 2]
        x = g.leaf(values(1, ne))
        if op == "GET_ROWS":
            return g.node(op, typ, [64, 3], [g.leaf(values(1, [64, 7])), g.leaf(np.array([0, 6, 3], np.int32), typ=I32)], nb=nb)
        if op == "ROPE":
            return _rope_node(g, x, 64, 2, typ=typ, nb=nb)
        if op == "SOFT_MAX":
            return g.node(op, typ, ne, [x], nb=nb, fparams={0: 1.0, 1: 0.0})
        return g.node(op, typ, ne, [x], nb=nb, fparams={0: 1e-5})
    for op in ("GET_ROWS", "NORM", "RMS_NORM", "SOFT_MAX", "ROPE"):
        @case(R, f"{op}-dst-f16", expect=R)
        def _(g, op=op):
            return row_op(g, op, F16, None)

        @case(R, f"{op}-dst-nb0_8", expect=R)
        def _(g, op=op):
            return row_op(g, op, F32, [8, 512, 1536, 4608])
    for op in ("CONCAT", "REPEAT"):
        for ts in ((I32, F32, F32), (F32, I32, F32), (I32, I32, F32), (F32, F32, I32)):
            if op == "REPEAT" and ts[1] != ts[0]:
                continue
            @case(R, f"{op}-{'-'.join(TN[t] for t in ts)}", expect=R)
            def _(g, op=op, ts=ts):
                def leaf(t):
                    return g.leaf(ints(1, [4, 2]) if t == I32 else values(1, [4, 2]), typ=t)
                if op == "CONCAT":
                    return g.node(op, ts[2], [4, 4], [leaf(ts[0]), leaf(ts[1])], params=[1])
                return g.node(op, ts[2], [4, 4], [leaf(ts[0])])


_refusals()

assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"
GROUPS = sorted({c.group for c in CASES if c.expect == "run"})


def by_group(group):
    return [c for c in CASES if c.group == group]
