"""Host side of the split-fp16 (hi + lo) kernel tests: the number format, a case table, and per operation one fp64 reference and one
fp32 emulation.  Nothing here needs a GPU (test_split_planes_cpu.py runs it all); test_split_planes_gpu.py uploads the same inputs.

A split map stores value = hi + lo in two fp16 planes (csrc/elementwise.hip, ld_split / st_split).  Every operation below is written
once, generic in the dtype: run in fp64 on the uploaded values (hi + lo) it is the reference, run in fp32 it is the emulation -- the
same operations as the kernel in one fixed order, each a single IEEE fp32 operation (no fused multiply-add).  For max pool, the layout
conversion, axpby with unit coefficients and sum_act the kernel has no freedom (no reduction tree, no contraction that changes a
result), so the emulation is bit-exact; for the others E_op = max |emulation before the store - reference| measures the fp32
arithmetic error and the GPU assertion is |got - ref| <= |ref| 2^-22 + 2^-25 + MARGIN E_op (the kernel's summation order and
contraction are not the emulation's: MARGIN = 4).

Mutants (what a subtly wrong kernel would compute, run through the emulation): "load" ignores the lo plane of every split input,
"store" leaves the output's lo plane at 0, "argmax" picks the max-pool winner from the hi plane alone.
"""
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

FMT_REL, FMT_ABS = 2.0 ** -22, 2.0 ** -25       # |split_load64(split_store(v)) - v| <= |v| FMT_REL + FMT_ABS  (test_split_format_bound)
MARGIN = 4.0
CANARY = 0x6B5A                                   # bit pattern of every element no launch may touch (fp16 3764.0)
SLICE_EXTRA, SLICE_C0 = 24, 8                     # the slice layout: channels [8, 8 + c) of a split buffer c + 24 channels wide

SP = namedtuple("SP", "hi lo")                    # one uploaded map, NCHW fp16 planes; lo None: a plain fp16 map
Case = namedtuple("Case", "id op kind out p mutants")   # kind: "exact" | "bounded"; out: "split" | "plain" | "f32"


def pad8(c):
    return (c + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------- the format
def split_store(v32):
    """st_split: hi = fp16(v), lo = fp16(v - fp32(hi))"""
    assert v32.dtype == torch.float32
    hi = v32.half()
    return hi, (v32 - hi.float()).half()


def split_load(hi, lo):
    """ld_split: fp32(hi) + fp32(lo)"""
    return hi.float() + lo.float()


def split_load64(hi, lo):
    return hi.double() + lo.double()


def fmt_bound(ref64):
    return ref64.abs() * FMT_REL + FMT_ABS


def load(p, dtype, drop_lo=False):
    return p.hi.to(dtype) if p.lo is None or drop_lo else p.hi.to(dtype) + p.lo.to(dtype)


def draw(shape, seed):
    """unit scale, 2^-6 <= |v| <= 2^3: the lo plane of such values is a normal fp16 number almost everywhere"""
    v = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return torch.where(v < 0, -1.0, 1.0) * v.abs().clamp(2.0 ** -6, 8.0)


def split_pair(v32):
    return SP(*split_store(v32))


def plain_pair(v32):
    return SP(v32.half(), None)


def tie_pair(shape, seed):
    """max-pool tie set: hi on a coarse grid g or one fp16 step above it, lo a multiple of a quarter step in [-1, 1] steps.  Windows hold
    several pixels with equal hi that differ only in lo, pixels whose larger hi carries a negative lo next to a smaller hi with a positive
    one (the hi plane alone picks the wrong winner), and different (hi, lo) pairs of EQUAL value (first-in-scan decides)."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.tensor([-1.0, 1.0, 1.5, 1.5, 1.5, 1.5])[torch.randint(0, 6, shape, generator=g)]      # a window's top level is shared by most of its pixels
    step = torch.where(grid.abs() >= 1.0, 2.0 ** -10, 2.0 ** -11)
    hi = grid + step * torch.randint(0, 2, shape, generator=g)
    lo = step * (torch.randint(-4, 5, shape, generator=g) / 4.0)
    assert torch.equal(hi.half().float(), hi) and torch.equal(lo.half().float(), lo)
    return SP(hi.half(), lo.half())


def grid_dy(shape, seed):
    """fp16 gradients on a 2^-8 grid, 0.25 <= |dy| < 4: any sum of four is exact in fp32, so the kernel's fp32 sums round like fp64 ones"""
    v = draw(shape, seed).clamp(-3.9, 3.9)
    v = torch.where(v < 0, -1.0, 1.0) * v.abs().clamp(min=0.25)
    return ((v * 256).round() / 256).half()


# ------------------------------------------------------------------------------------------------- the operations, dtype-generic
def op_convert(src, mean, invstd):
    """nchw32_to_nhwc16_kernel: (v - mean[n, c]) * invstd[n, c], a subtraction and a multiplication"""
    if mean is None:
        return src
    return (src - mean[:, :, None, None]) * invstd[:, :, None, None]


def op_maxpool(x):
    return F.max_pool2d(x, 3, 2, 1)


def op_maxpool_idx(x):
    """first maximum in scan order (torch's CPU rule, strict >), as flat indices into H*W"""
    return F.max_pool2d(x, 3, 2, 1, return_indices=True)[1]


def op_maxpool_bwd(idx, dy, hw):
    dx = torch.zeros(dy.shape[0], dy.shape[1], hw[0] * hw[1], dtype=dy.dtype)
    return dx.scatter_add_(2, idx.flatten(2), dy.flatten(2)).view(dy.shape[0], dy.shape[1], *hw)


def op_axpby(x, z, a, b):
    if z is None:
        return x * a
    if a == 1.0 and b == 1.0:
        return x + z
    return x * a + z * b


def op_sum_act(terms, relu):
    acc = torch.zeros_like(terms[0])
    for t in terms:                       # t = 0 .. n-1, the kernel's order
        acc = acc + t
    return torch.where(acc < 0, torch.zeros_like(acc), acc) if relu else acc


def op_bn(x, res, mean, invstd, gamma, beta, act, slope, drop):
    """bn_apply_kernel: ((x - mean) * (invstd * gamma) + beta) + res, activation, dropout scale"""
    b = lambda t: t[None, :, None, None]
    v = (x - b(mean)) * b(invstd * gamma) + b(beta)
    if res is not None:
        v = v + res
    if act == "relu":
        v = torch.where(v > 0, v, torch.zeros_like(v))
    elif act == "prelu":
        v = torch.where(v > 0, v, v * slope)
    return v if drop is None else v * drop[:, :, None, None]


def aap_bins(n_in, n_out):
    return [((o * n_in) // n_out, ((o + 1) * n_in + n_out - 1) // n_out) for o in range(n_out)]


def op_aap(x, OH, OW, block):
    """aap_fwd_kernel: the bin's pixels added in scan order, times 1 / count.  aap_fwd_block_kernel: pixel i goes to lane i % 32, the 32
    lanes are added in lane order, the sum is divided by the count."""
    N, C, H, W = x.shape
    out = torch.zeros(N, C, OH, OW, dtype=x.dtype)
    for oy, (y0, y1) in enumerate(aap_bins(H, OH)):
        for ox, (x0, x1) in enumerate(aap_bins(W, OW)):
            v = x[:, :, y0:y1, x0:x1].reshape(N, C, -1)
            cnt = v.shape[2]
            if block:
                v = F.pad(v, (0, -cnt % 32)).view(N, C, -1, 32)
                lanes = torch.zeros(N, C, 32, dtype=x.dtype)
                for k in range(v.shape[2]):
                    lanes = lanes + v[:, :, k]
                s = torch.zeros(N, C, dtype=x.dtype)
                for q in range(32):
                    s = s + lanes[:, :, q]
                out[:, :, oy, ox] = s / cnt
            else:
                s = torch.zeros(N, C, dtype=x.dtype)
                for k in range(cnt):
                    s = s + v[:, :, k]
                out[:, :, oy, ox] = s * (torch.ones((), dtype=x.dtype) / cnt)
    return out


def bil_axis(n_in, n_out, align, dtype):
    """bil_src: source index pair and weight of every output index, computed in ``dtype``"""
    o = torch.arange(n_out, dtype=dtype)
    if align:
        src = o * float(n_in - 1) / float(n_out - 1) if n_out > 1 else torch.zeros(n_out, dtype=dtype)
    else:
        src = ((o + 0.5) * (torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0.to(dtype)


def op_bilinear(x, OH, OW, align, drop):
    """bilinear_fwd_kernel / bilinear_fwd_cols_kernel (one arithmetic): weights in the working precision from bil_src"""
    y0, y1, wy = bil_axis(x.shape[2], OH, align, x.dtype)
    x0, x1, wx = bil_axis(x.shape[3], OW, align, x.dtype)
    wy, wx = wy[:, None], wx[None, :]
    g = lambda yi, xi: x[:, :, yi][:, :, :, xi]
    v = (1 - wy) * ((1 - wx) * g(y0, x0) + wx * g(y0, x1)) + wy * ((1 - wx) * g(y1, x0) + wx * g(y1, x1))
    return v if drop is None else v * drop[:, :, None, None]


def ref_bilinear(x64, OH, OW, align, drop64):
    """torch's own fp64 bilinear (its index rule, fp64 weights)"""
    v = F.interpolate(x64, size=(OH, OW), mode="bilinear", align_corners=align)
    return v if drop64 is None else v * drop64[:, :, None, None]


def op_wpool(x, w):
    """wpool_fwd_kernel: out[n][c] = sum_p w[n][p] x[n][p][c].  1024-pixel chunks; in a chunk pixel group pg takes pixels pg, pg + groups, ...
    (groups = 256 / c8), the groups are added in order, then the chunks (csbsr_sum_partials)."""
    N, C, H, W = x.shape
    hw, groups = H * W, 256 // (C // 8)
    xs = x.reshape(N, C, hw)
    out = torch.zeros(N, C, dtype=x.dtype)
    for p0 in range(0, hw, 1024):
        p1 = min(hw, p0 + 1024)
        t = xs[:, :, p0:p1] * w[:, None, p0:p1]
        t = F.pad(t, (0, -(p1 - p0) % groups)).view(N, C, -1, groups)
        acc = torch.zeros(N, C, groups, dtype=x.dtype)
        for k in range(t.shape[2]):
            acc = acc + t[:, :, k]
        part = torch.zeros(N, C, dtype=x.dtype)
        for q in range(groups):
            part = part + acc[:, :, q]
        out = out + part
    return out


# ------------------------------------------------------------------------------------------------- the case table
def _cases():
    rows = []

    def add(id_, op, kind, out, mutants, **p):
        rows.append(Case(id_, op, kind, out, p, tuple(mutants)))

    for C in (3, 20):
        for norm in (False, True):
            add(f"convert-C{C}-{'norm' if norm else 'raw'}", "convert", "exact", "split", ["store"], shape=(2, C, 7, 9), norm=norm)
    for shape in ((2, 16, 11, 14), (1, 8, 7, 9), (1, 8, 1, 5), (2, 24, 16, 12)):
        for tie in (False, True):
            tag = "x".join(map(str, shape)) + ("-tie" if tie else "")
            add("maxpool-" + tag, "maxpool", "exact", "split", ["load", "store"] + (["argmax"] if tie else []), shape=shape, tie=tie)
            # (random inputs: two pixels of one window never share hi, so neither mutant moves a gradient -- the tie sets are the test)
            add("maxpool_bwd-" + tag, "maxpool_bwd", "exact", "plain", ["load", "argmax"] if tie else [], shape=shape, tie=tie)
    for v in ("unit", "znone", "mixed", "toplain", "scaled"):
        add("axpby-" + v, "axpby", "bounded" if v == "scaled" else "exact", "plain" if v == "toplain" else "split",
            [] if v == "toplain" else ["load", "store"], shape=(2, 24, 7, 9), variant=v)
    for n, split_terms in ((1, (1,)), (3, (1, 0, 1)), (4, (1, 1, 0, 0))):
        for relu in (False, True):
            add(f"sum_act-n{n}-relu{int(relu)}", "sum_act", "exact", "split", ["load", "store"], shape=(2, 24, 7, 9), split_terms=split_terms,
                relu=relu)
    for shape in ((3, 16, 9, 10), (2, 40, 5, 7)):          # c8 = 5: grid_for_c8 rounds the grid up to a multiple of 5
        for act in ("none", "relu", "prelu"):
            for drop in (False, True):
                add(f"bn-{'x'.join(map(str, shape))}-{act}-drop{int(drop)}", "bn", "bounded", "split", ["load", "store"], shape=shape, act=act,
                    drop=drop, cancel=False)
    # the same with a residual that cancels a quarter of the elements down to rounding distance of z = 0: the rows for the backward's mask
    for shape, act, drop in (((3, 16, 9, 10), "relu", False), ((3, 16, 9, 10), "prelu", True), ((2, 40, 5, 7), "relu", True), ((2, 40, 5, 7), "prelu", False)):
        add(f"bn-{'x'.join(map(str, shape))}-{act}-drop{int(drop)}-cancel", "bn", "bounded", "split", ["load", "store"], shape=shape, act=act,
            drop=drop, cancel=True)
    # adaptive average pool; ``block``: the launcher takes aap_fwd_block_kernel ((H / OH) * (W / OW) >= 64).  8x8 -> 1 is exactly 64.
    for size in (1, 2, 3, 6):
        add(f"aap-8x8-{size}-c24", "aap", "bounded", "split", ["load", "store"], shape=(2, 24, 8, 8), osize=(size, size), block=size == 1)
    add("aap-11x14-3x5-c24", "aap", "bounded", "split", ["load", "store"], shape=(2, 24, 11, 14), osize=(3, 5), block=False)
    for c in (24, 136):                                    # c8 = 3: channel lanes 3 .. 7 idle; c8 = 17: the third group has one lane
        for (H, W), s in (((20, 20), 2), ((17, 19), 2), ((24, 24), 3), ((16, 16), 1)):
            add(f"aap-{H}x{W}-{s}-c{c}", "aap", "bounded", "split", ["load", "store"], shape=(2, c, H, W), osize=(s, s), block=True)
    # bilinear; ``cols``: the launcher takes bilinear_fwd_cols_kernel
    for align in (False, True):
        a = f"-align{int(align)}"
        add("bilinear-8x8-16x16" + a, "bilinear", "bounded", "split", ["load", "store"], shape=(2, 24, 8, 8), osize=(16, 16), align=align,
            drop=False, cols=False)
        add("bilinear-5x7-20x21-drop" + a, "bilinear", "bounded", "split", ["load", "store"], shape=(2, 24, 5, 7), osize=(20, 21), align=align,
            drop=True, cols=False)
        add("bilinear-6x6-1x1" + a, "bilinear", "bounded", "split", ["load", "store"], shape=(2, 24, 6, 6), osize=(1, 1), align=align,
            drop=False, cols=False)
        add("bilinear-23x31-50x70-drop" + a, "bilinear", "bounded", "split", ["load", "store"], shape=(2, 240, 23, 31), osize=(50, 70),
            align=align, drop=True, cols=True)
        add("bilinear-32x32-64x64" + a, "bilinear", "bounded", "split", ["load", "store"], shape=(2, 256, 32, 32), osize=(64, 64), align=align,
            drop=False, cols=True)
    for hw in ((33, 31), (42, 50)):                        # 1023 pixels: one ragged chunk; 2100: three
        for c in (64, 320):                                # c8 = 40: 256 % 40 = 16 idle tail threads
            add(f"wpool-{hw[0] * hw[1]}-c{c}", "wpool", "bounded", "f32", ["load"], shape=(2, c, *hw))
    return rows


CASES = _cases()


def _seed(case):
    return zlib.crc32(case.id.encode())            # (a row keeps its inputs when rows are added)


def _f32(x):
    return x.float().contiguous()


def make_inputs(case):
    """the uploaded inputs of a case, a dict; SP pairs are NCHW.  Deterministic: the CPU and the GPU tests see the same numbers."""
    p, s = case.p, _seed(case)
    N, C, H, W = p["shape"]
    op = case.op
    if op == "convert":
        d = {"src": draw(p["shape"], s), "mean": None, "invstd": None}
        if p["norm"]:
            d["mean"] = _f32(d["src"].double().mean((2, 3)))
            d["invstd"] = _f32(1.0 / (d["src"].double().var((2, 3), unbiased=False) + 1e-5).sqrt())
        return d
    if op in ("maxpool", "maxpool_bwd"):
        d = {"x": tie_pair(p["shape"], s) if p["tie"] else split_pair(draw(p["shape"], s))}
        if op == "maxpool_bwd":
            d["dy"] = grid_dy((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), s + 500)
        return d
    if op == "axpby":
        v = p["variant"]
        return {"x": split_pair(draw(p["shape"], s)),
                "z": None if v == "znone" else (plain_pair if v == "mixed" else split_pair)(draw(p["shape"], s + 500)),
                "a": float(torch.tensor(0.7)) if v == "scaled" else 1.0, "b": float(torch.tensor(-1.3)) if v == "scaled" else 1.0}
    if op == "sum_act":
        return {"terms": [(split_pair if sp else plain_pair)(draw(p["shape"], s + 100 * t)) for t, sp in enumerate(p["split_terms"])]}
    if op == "bn":
        g = torch.Generator().manual_seed(s)
        x = split_pair(draw(p["shape"], s))
        x64 = load(x, torch.float64)
        d = {"x": x, "mean": _f32(x64.mean((0, 2, 3))), "invstd": _f32(1.0 / (x64.var((0, 2, 3), unbiased=False) + 1e-5).sqrt()),
             "gamma": 1 + 0.2 * torch.randn(C, generator=g), "beta": 0.1 * torch.randn(C, generator=g), "slope": 0.25,
             "drop": (torch.rand(N, C, generator=g) > 0.3).float() / 0.7 if p["drop"] else None}
        res = draw(p["shape"], s + 500)
        if p["cancel"]:
            # a quarter of the elements cancel the normalised value down to rounding distance (|z| ~ 2^-23 |x|): the sign of z there
            # depends on how z is computed -- the elements at which a backward mask can disagree with the forward
            z0 = op_bn(load(x, torch.float32), None, d["mean"], d["invstd"], d["gamma"], d["beta"], "none", 0.0, None)
            res = torch.where(torch.rand(p["shape"], generator=g) < 0.25, -z0, res)
        d["res"] = split_pair(res)
        d["dy"] = grid_dy(p["shape"], s + 700)
        return d
    if op == "aap":
        return {"x": split_pair(draw(p["shape"], s))}
    if op == "bilinear":
        g = torch.Generator().manual_seed(s)
        # The kernel's fp32 source position is off by ~2^-24 W, and the weight error times the difference of two neighbours is the bulk of
        # E_op: 1.1e-5 for 31 -> 70 columns of independent unit-scale pixels, more than a dropped lo plane costs (2^-12 |v|).  A map around
        # 2 whose neighbours differ by ~0.35 keeps E_op near 1e-6 and lo-plane errors where they were (they scale with |v|, not with
        # differences); a wrong index still moves a result by ~0.35, 1e5 times the bound.
        return {"x": split_pair(2 + 0.25 * torch.randn(p["shape"], generator=g)), "drop": (torch.rand(N, C, generator=g) > 0.3).float() * 1.25 if p["drop"] else None}
    if op == "wpool":
        g = torch.Generator().manual_seed(s)
        return {"x": split_pair(draw(p["shape"], s)), "w": torch.softmax(2 * torch.randn(N, H * W, generator=g), 1)}
    raise KeyError(op)


def compute(case, ins, dtype, mutate=None):
    """the case's operation in ``dtype`` on the uploaded values: fp64 = the reference, fp32 = the emulation before the store"""
    p, op = case.p, case.op
    ld = lambda q: load(q, dtype, drop_lo=mutate == "load")
    cast = lambda t: None if t is None else t.to(dtype)
    if op == "convert":
        return op_convert(cast(ins["src"]), cast(ins["mean"]), cast(ins["invstd"]))
    if op == "maxpool":
        x = ld(ins["x"])
        if mutate == "argmax":          # the winner chosen on the hi plane, its full value stored
            return x.flatten(2).gather(2, op_maxpool_idx(ins["x"].hi.to(dtype)).flatten(2)).view_as(op_maxpool(x))
        return op_maxpool(x)
    if op == "maxpool_bwd":
        idx = op_maxpool_idx(ins["x"].hi.to(dtype) if mutate == "argmax" else ld(ins["x"]))
        return op_maxpool_bwd(idx, cast(ins["dy"]), p["shape"][2:])
    if op == "axpby":
        return op_axpby(ld(ins["x"]), None if ins["z"] is None else ld(ins["z"]), ins["a"], ins["b"])
    if op == "sum_act":
        return op_sum_act([ld(t) for t in ins["terms"]], p["relu"])
    if op == "bn":
        return op_bn(ld(ins["x"]), ld(ins["res"]), cast(ins["mean"]), cast(ins["invstd"]), cast(ins["gamma"]), cast(ins["beta"]), p["act"],
                     ins["slope"], cast(ins["drop"]))
    if op == "aap":
        return op_aap(ld(ins["x"]), *p["osize"], p["block"])
    if op == "bilinear":
        if dtype == torch.float64:
            return ref_bilinear(ld(ins["x"]), *p["osize"], p["align"], cast(ins["drop"]))
        return op_bilinear(ld(ins["x"]), *p["osize"], p["align"], cast(ins["drop"]))
    if op == "wpool":
        return op_wpool(ld(ins["x"]), cast(ins["w"]))
    raise KeyError(op)


def stored64(case, out32, mutate=None):
    """the fp64 value a kernel leaves behind for the fp32 result ``out32``"""
    if case.out == "f32":
        return out32.double()
    if case.out == "plain":
        return out32.half().double()
    hi, lo = split_store(out32)
    return hi.double() if mutate == "store" else split_load64(hi, lo)


Host = namedtuple("Host", "ins ref64 out32 e_op bound")
_HOST = {}


def host(case):
    """inputs, reference, emulation, E_op and the elementwise bound of a case (computed once per process, never modified)"""
    if case.id not in _HOST:
        ins = make_inputs(case)
        ref64, out32 = compute(case, ins, torch.float64), compute(case, ins, torch.float32)
        e_op = float((out32.double() - ref64).abs().max())
        fmt = ref64.abs() * 2.0 ** -24 if case.out == "f32" else fmt_bound(ref64)          # an fp32 output: one rounding of the result
        _HOST[case.id] = Host(ins, ref64, out32, e_op, fmt + MARGIN * e_op)
    return _HOST[case.id]


def mutant64(case, mutate):
    ins = host(case).ins
    out32 = compute(case, ins, torch.float32, mutate if mutate != "store" else None)
    return stored64(case, out32, mutate)


# ------------------------------------------------------------------------------------------------- the composed chain
CHAIN_SHAPE, CHAIN_CP = (1, 3, 33, 41), 8


def chain_host(hi_only=False):
    """PSPNet stem-to-pyramid path in split mode: layout conversion -> BN (relu) -> max pool -> adaptive pool to 2 -> bilinear back -> axpby
    onto the pooled map.  Returns the inputs, the fp64 chain, the emulated chain (every stage stored as a split pair and loaded again;
    ``hi_only``: every lo plane forced to 0) and the bound on |device - fp64| of the last stage.

    The bound: stage s computes f_s; with d_s the device's stored result and r_s the fp64 chain's, e_s = max |d_s - r_s| obeys
    e_s <= L_s e_(s-1) + B_s, where L_s is the stage's Lipschitz constant in the max norm (max |invstd gamma| for BN, 1 for the pools and
    the resize, whose weights are convex, |a| and |b| for the two inputs of axpby) and B_s = max |r_s| 2^-22 + 2^-25 + MARGIN E_op_s is the
    stage's own bound, E_op_s measured on the emulated chain's input to that stage."""
    N, C, H, W = CHAIN_SHAPE
    src = torch.zeros(N, CHAIN_CP, H, W)
    src[:, :C] = draw(CHAIN_SHAPE, 77)
    g = torch.Generator().manual_seed(77)
    ins = {"src": src[:, :C].contiguous(), "gamma": 1 + 0.2 * torch.randn(CHAIN_CP, generator=g), "beta": 0.1 * torch.randn(CHAIN_CP, generator=g)}
    x1 = split_load64(*split_store(src))
    mean, var = x1.mean((0, 2, 3)), x1.var((0, 2, 3), unbiased=False)
    ins["mean"], ins["invstd"] = _f32(mean), _f32(1.0 / (var + 1e-5).sqrt())
    ins["mean"][C:], ins["invstd"][C:] = 0.0, 1.0              # padding channels: x = 0 passes through
    bnp = [ins[k] for k in ("mean", "invstd", "gamma", "beta")]
    PH, PW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    stages = [("convert", lambda T, a: a["src"], 0.0),
              ("bn", lambda T, a: op_bn(a["convert"], None, *[t.to(T) for t in bnp], "relu", 0.0, None), float((ins["invstd"] * ins["gamma"]).abs().max())),
              ("maxpool", lambda T, a: op_maxpool(a["bn"]), 1.0),
              ("aap", lambda T, a: op_aap(a["maxpool"], 2, 2, True), 1.0),
              ("bilinear", lambda T, a: (ref_bilinear(a["aap"], PH, PW, False, None) if T == torch.float64 else op_bilinear(a["aap"], PH, PW, False, None)), 1.0),
              ("axpby", lambda T, a: op_axpby(a["bilinear"], a["maxpool"], 1.0, 1.0), None)]
    r, em, e, e_op = {"src": src.double()}, {"src": src}, {}, {}        # fp64 chain; emulated chain (loaded fp32 values); error bounds; E_op
    for name, f, lip in stages:
        r[name] = f(torch.float64, r)
        out32 = f(torch.float32, em)
        e_op[name] = float((out32.double() - f(torch.float64, {k: v.double() for k, v in em.items()})).abs().max())
        hi, lo = split_store(out32)
        em[name] = hi.float() if hi_only else split_load(hi, lo)
        b_s = float(r[name].abs().max()) * FMT_REL + FMT_ABS + MARGIN * e_op[name]
        prev = {"convert": 0.0, "bn": e.get("convert"), "maxpool": e.get("bn"), "aap": e.get("maxpool"), "bilinear": e.get("aap")}.get(name)
        e[name] = (e["bilinear"] + e["maxpool"] if name == "axpby" else lip * prev) + b_s
    return ins, r, em, e_op, e


# ------------------------------------------------------------------------------------------------- device maps with canaries
def _canary_buf(N, H, W, width):
    return torch.full((N, H, W, width), CANARY, dtype=torch.int16).view(torch.float16)


def _fm(eng, buf, c, cpt, c0, split):
    from csbsr_amd.engine import FM
    return FM(buf.to(eng.device)[..., c0:c0 + pad8(c)], c, lo=cpt if split else 0)


def _geometry(c, c_total, c0):
    return (pad8(c), 0) if c_total is None else (pad8(c_total), c0)


def empty_split_fm(eng, N, H, W, c, c_total=None, c0=0, split=True):
    """an output map: every element -- both planes, the padding channels, the rest of a wider buffer -- holds the canary"""
    cpt, c0 = _geometry(c, c_total, c0)
    assert c0 % 8 == 0 and c0 + pad8(c) <= cpt
    return _fm(eng, _canary_buf(N, H, W, (2 if split else 1) * cpt), c, cpt, c0, split)


def to_split_fm(eng, x, c_total=None, c0=0):
    """upload an SP pair (or fp32 values, split here) as a whole [hi | lo] map (lo == cp) or as channels [c0, c0 + c) of a split buffer
    pad8(c_total) channels wide (ld = 2 pad8(c_total), lo = pad8(c_total)); a pair without lo becomes a plain map.  Everything outside the
    slice holds the canary; the slice's own padding channels are 0, as in any map."""
    if not isinstance(x, SP):
        x = split_pair(x)
    N, c, H, W = x.hi.shape
    cpt, c0 = _geometry(c, c_total, c0)
    split = x.lo is not None
    buf = _canary_buf(N, H, W, (2 if split else 1) * cpt)
    for plane, off in ((x.hi, c0), (x.lo, cpt + c0)) if split else ((x.hi, c0),):
        buf[..., off:off + pad8(c)] = 0
        buf[..., off:off + c] = plane.permute(0, 2, 3, 1)
    return _fm(eng, buf, c, cpt, c0, split)


def _base(fm):
    base = fm.t if fm.t._base is None else fm.t._base
    return base, fm.t.storage_offset() - base.storage_offset()


def planes(fm, padded=False):
    """(hi, lo) of a device map as NCHW fp16 CPU tensors (lo None for a plain map); ``padded``: with the padding channels"""
    c = fm.cp if padded else fm.c
    hi = fm.t[..., :c].cpu().permute(0, 3, 1, 2).contiguous()
    if not fm.lo:
        return hi, None
    lo = torch.as_strided(fm.t, fm.t.shape, fm.t.stride(), fm.t.storage_offset() + fm.lo)
    return hi, lo[..., :c].cpu().permute(0, 3, 1, 2).contiguous()


def from_split_fm(fm):
    """fp64 hi + lo of a device map, NCHW, real channels"""
    hi, lo = planes(fm)
    return hi.double() if lo is None else split_load64(hi, lo)


def canary_damage(fm):
    """number of elements outside the map's own channels (both planes) that no longer hold the canary bit pattern"""
    base, c0 = _base(fm)
    keep = torch.ones(base.shape[-1], dtype=torch.bool)
    keep[c0:c0 + fm.cp] = False
    if fm.lo:
        keep[c0 + fm.lo:c0 + fm.lo + fm.cp] = False
    return int((base.cpu().view(torch.int16)[..., keep] != CANARY).sum())


def assert_canaries(*fms):
    for i, fm in enumerate(fms):
        n = canary_damage(fm)
        assert n == 0, f"map {i}: {n} elements outside the slice were overwritten"
