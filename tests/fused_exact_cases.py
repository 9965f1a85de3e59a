"""The case table of tests/test_fused_exact_gpu.py: exact-lattice rows for the paths that write more than one output -- the dgrads that
take over the epilogue-backward pass of the layer below (conv_tp's TP/14 and TP/13, the thin-input DACT kernel), the one-pass backward of
kb.up_conv1 (csrc/conv_kbup.hip), the folded constant segment (Conv.fwd_folded / bwd_weights_folded / fwd_const_1x1), ShuffleConv, and
the kernel predictor's backward (csbsr_amd/modeling/kp_bwd.py: csrc/conv_pair.hip, the masked fill with class sums and its fold).

Plain torch on the CPU, importable without a GPU: every ``build_*`` draws the operands of one row on the lattice of
tests/test_conv_exact_gpu.py (activations and gradients i / 4, weights j / 8, bias / old gradient / residual k / 32, every slope 0.25 --
the kernels divide by the slope, exact only for a power of two) and PROVES the bounds on the reference before anything is compared with
it: every reference is on its lattice and fits the output format, and every fp32 sum a kernel forms has sum |terms| / unit < 2^24 on the
actual values, so no summation order, no split into tiles or workgroups and no number of partial rows can round.  The share of 2^24 the
largest sum of a case uses is kept in ``case.share`` (tests/test_fused_exact_cases_cpu.py prints it).

Row fields: name; entry (the engine / kp_bwd entry point the row covers); group (the builder and runner); args (the builder's arguments);
kid / var (csbsr_debug_last_conv_kernel() & 255 / >> 8, None where the path records none; ShuffleConv: per launch); budget (run again under CU budgets); why."""
from collections import namedtuple
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import exact_lattice as XL

SLOPE = 0.25
QX, QW, QB = 2, 3, 5
UNIT = 2.0 ** -(QX + QW)          # a product of an activation and a weight
BUDGETS = (1, 3, 7)

FRow = namedtuple("FRow", "name entry group args kid var budget why")


def FR(name, entry, group, args, kid=None, var=None, budget=False, why=""):
    return FRow(name, entry, group, dict(args), kid, var, budget, why)


X3 = (("conv_x3", 2),)
X3N = (("conv_x3n", 2),)
X3W = (("conv_x3w", 2), ("eng.use_x3w", 2))

FUSED_ROWS = [
    # ---- conv_tp's dgrad with the bias / PReLU-slope sums of the layer below (csrc/conv_tp.hip, HAS_STAT): var bits 2 acc, 4 mask, 8 sums, 1 res
    FR("tp_dact", "Conv.bwd_input", "tp_dact", dict(res=None), kid=9, var=14, budget=True,
       why="accumulating dgrad + mask + sums of the layer below: two whole 8 x 32 tiles per sample"),
    FR("tp_dact_res_sub", "Conv.bwd_input", "tp_dact", dict(res="sub"), kid=9, var=13, budget=True,
       why="the layer below was act(pre) - res: activation rebuilt as saved + res, d(res) = -tot the second output"),
    FR("tp_dact_res_add", "Conv.bwd_input", "tp_dact", dict(res="add"), kid=9, var=13, budget=True,
       why="the layer below was act(pre) + res: activation rebuilt as saved - res, d(res) = +tot"),
    # ---- the thin-input accumulating dgrad with the epilogue-backward of the PReLU + residual layer below (csrc/conv_thin.hip, DACT)
    FR("thin_dact_128_add", "Conv.bwd_input", "thin_dact", dict(cout=128, H=9, W=70, res="add"), kid=13,
       why="conv_thin_cin2_kernel<true>: 128 features, ragged tiles, more than one workgroup partial"),
    FR("thin_dact_128_sub", "Conv.bwd_input", "thin_dact", dict(cout=128, H=9, W=70, res="sub"), kid=13, why="the same, RES_SUB: d(res) = -tot"),
    FR("thin_dact_64_add", "Conv.bwd_input", "thin_dact", dict(cout=64, H=16, W=32, res="add"), kid=13, why="64 features: two cout tiles per lane ring"),
    FR("thin_dact_64_sub", "Conv.bwd_input", "thin_dact", dict(cout=64, H=16, W=32, res="sub"), kid=13, why="the same, RES_SUB"),
    # ---- one-pass backward of kb.up_conv1 (csrc/conv_kbup.hip): dPre, weight gradient slabs, slope partials
    FR("kbup_128", "Conv.bwd_thin_tp_fused", "kbup", dict(cout=128, h=9, w=33), why="ragged against the 4-row blocks and the pixel lanes"),
    FR("kbup_64", "Conv.bwd_thin_tp_fused", "kbup", dict(cout=64, h=5, w=8), why="8 octets: eight pixels per wave pass, two row blocks"),
    FR("kbup_8", "Conv.bwd_thin_tp_fused", "kbup", dict(cout=8, h=4, w=7), why="one octet: 64 pixel lanes, most of them dead"),
    # ---- Conv.fwd_folded: the constant segment as a 16-class bias table, one row per kernel family the models reach it on
    FR("folded_glds", "Conv.fwd_folded", "folded_fwd", dict(cout=100, H=12, W=20, modes=()), kid=3, var=0, why="the general LDS-DMA kernel"),
    FR("folded_x3", "Conv.fwd_folded", "folded_fwd", dict(cout=100, H=12, W=20, modes=X3), kid=17, var=0, budget=True, why="conv_x3, straight-line rows"),
    FR("folded_x3w", "Conv.fwd_folded", "folded_fwd", dict(cout=100, H=12, W=20, modes=X3W), kid=19, var=1, budget=True, why="conv_x3w, straight-line rows"),
    FR("folded_x3n_lean", "Conv.fwd_folded", "folded_fwd", dict(cout=200, H=27, W=100, modes=X3N), kid=20, var=13, budget=True,
       why="wide lean conv_x3n: interior tiles (class row through LDS) next to border tiles"),
    # ---- Conv.bwd_weights_folded: feature half on the MFMA, constant half and dL/dk from the 16 border-class sums of dPre
    # (``prelu_out`` -- the slope gradient from the same pass -- exists from 1024 pixels on, csbsr_border_class_sums_prelu; the callers test that)
    FR("folded_bwd_12x20", "Conv.bwd_weights_folded", "folded_bwd", dict(H=12, W=20, prelu=False), why="every border class and an interior"),
    FR("folded_bwd_1x7", "Conv.bwd_weights_folded", "folded_bwd", dict(H=1, W=7, prelu=False), why="one row: first and last row classes coincide"),
    FR("folded_bwd_2x5", "Conv.bwd_weights_folded", "folded_bwd", dict(H=2, W=5, prelu=False), why="two rows: no interior row"),
    FR("folded_bwd_3x3", "Conv.bwd_weights_folded", "folded_bwd", dict(H=3, W=3, prelu=False), why="one interior pixel"),
    FR("folded_bwd_prelu_32x32", "Conv.bwd_weights_folded", "folded_bwd", dict(H=32, W=32, prelu=True),
       why="prelu_out: 1024 pixels, the first size of the total-minus-borders kernels that also take the slope sum"),
    FR("folded_bwd_prelu_40x33", "Conv.bwd_weights_folded", "folded_bwd", dict(H=40, W=33, prelu=True), why="prelu_out, ragged chunks"),
    # ---- Conv.fwd_const_1x1 (plain input): the constant segment as a per-sample bias row
    FR("const_1x1", "Conv.fwd_const_1x1", "const_1x1", dict(stat=False), kid=3, var=0, why="1x1, 128 -> 100: the general kernels"),
    FR("const_1x1_bn", "Conv.fwd_const_1x1", "const_1x1", dict(stat=True), kid=3, var=0, why="with BatchNorm sums (HRNet's fuse layer)"),
    # ---- ShuffleConv: conv3x3 + pixel shuffle as a transposed conv with a permuted weight; kid = (forward, dgrad, wgrad) kernel IDs.
    # 3s x 3s taps at stride s are three taps per phase and axis: not conv_tp's 2 x 2, so the general kernels take forward and dgrad
    FR("shuffle_s2", "ShuffleConv", "shuffle", dict(s=2, cin=128, C=128, H=9, W=11), kid=(3, 3, 5), var=(0, 0),
       why="6x6 stride 2, 128 -> 128: LDS-DMA 128 tile forward and dgrad (36 taps), LDS-DMA 128 x 128 wgrad"),
    FR("shuffle_s4", "ShuffleConv", "shuffle", dict(s=4, cin=128, C=128, H=5, W=7), kid=(3, 2, 6), var=(0, 0),
       why="12x12 stride 4: the dgrad's 144 taps exceed the LDS-DMA kernels' 64-bit tap mask -> register-staged 128; wgrad 128 x 256"),
    FR("shuffle_s4_thin", "ShuffleConv", "shuffle", dict(s=4, cin=3, C=64, H=6, W=9), kid=(1, 0, 3), var=(0, 0),
       why="3 -> 64: register-staged 64 forward (8 padded input channels), 32-row dgrad into 8 padded channels, 32-row wgrad"),
    # ---- kp_bwd.pair1x1_backward (csrc/conv_pair.hip): dgrad + mask and the weight gradient from one pass
    FR("pair_19x45", "kp_bwd.pair1x1_backward", "pair", dict(N=3, H=19, W=45, cin_tot=49), budget=True, why="ragged tiles, the ring of tile buffers walked"),
    FR("pair_1x7", "kp_bwd.pair1x1_backward", "pair", dict(N=3, H=1, W=7, cin_tot=49), budget=True,
       why="21 pixels: the transposing LDS reads run past the last pixel"),
    FR("pair_8x32_98", "kp_bwd.pair1x1_backward", "pair", dict(N=3, H=8, W=32, cin_tot=98), budget=True,
       why="fe_cat.0's form: the first 49 of 98 columns only"),
    # ---- kp_bwd.fold_const_wgrad on the class sums of csbsr_border_class_fill_masked_sums
    FR("fillsums_1x7", "kp_bwd.fold_const_wgrad", "fillsums", dict(H=1, W=7), why="small-map route, one row"),
    FR("fillsums_2x5", "kp_bwd.fold_const_wgrad", "fillsums", dict(H=2, W=5), why="small-map route, no interior row"),
    FR("fillsums_3x3", "kp_bwd.fold_const_wgrad", "fillsums", dict(H=3, W=3), why="small-map route, one interior pixel"),
    FR("fillsums_32x32", "kp_bwd.fold_const_wgrad", "fillsums", dict(H=32, W=32), why="1024 pixels: the first size of the one-pass kernel"),
    FR("fillsums_40x33", "kp_bwd.fold_const_wgrad", "fillsums", dict(H=40, W=33), why="one-pass kernel, ragged chunks"),
]


# ---------------------------------------------------------------------------------------------------------------- helpers

def _gen(name):
    return torch.Generator().manual_seed(sum(map(ord, name)) + 7)


def draw_gate(shape, gen, neg=1.0 / 32, zero=1.0 / 64):
    """an activation map that pins the gate convention: positives j / 4 (j = 1..4), negatives -j / 16, and a few exact zeros
    (``y > 0`` against ``y >= 0``: at y == 0 the gradient is multiplied by the slope and adds a zero term to the slope sum)"""
    u = torch.rand(tuple(shape), generator=gen)
    j = torch.randint(1, 5, tuple(shape), generator=gen).to(torch.float32)
    return torch.where(u < neg, -j / 16, torch.where(u < neg + zero, torch.zeros(()), j / 4))


def share(terms, unit, dims=None):
    """largest sum |terms| / unit over ``dims`` (None: everything) as a share of 2^24"""
    a = terms.double().abs() / unit
    return float((a.sum() if dims is None else a.sum(dims).max())) / XL.FP32_EXACT


def assert_share(case, what, terms, unit, dims=None):
    s = share(terms, unit, dims)
    assert s < 1.0, f"{case.name}: {what}: sum |terms| = {s:.3g} x 2^24 units: the fp32 sum is not order-free; use a sparser draw"
    case.share[what] = s


def assert_k_bound(case, what, n_terms, unit=None):
    """a K-term sum of activation x weight products: K x max|a| x max|b| < 2^24 units (XL.assert_sum_bound), its share recorded"""
    unit = UNIT if unit is None else unit
    XL.assert_sum_bound(n_terms, 2.0 ** (1 - QX), 2.0 ** (1 - QW), unit, f"{case.name} {what}")
    case.share[what + " (bound)"] = n_terms * 2.0 ** (1 - QX) * 2.0 ** (1 - QW) / unit / XL.FP32_EXACT


def class_index(H, W):
    """border class of every pixel: (first row) 8 + (last row) 4 + (first column) 2 + (last column)"""
    y, x = torch.arange(H)[:, None], torch.arange(W)[None, :]
    return (y == 0) * 8 + (y == H - 1) * 4 + (x == 0) * 2 + (x == W - 1)


def class_sums(t, drop=None):
    """[N, 16, C] sums of an NCHW map per border class (``drop``: a class left out -- the mutant of the CPU test)"""
    cls = class_index(*t.shape[2:])
    return torch.stack([(t * ((cls == k) & (k != drop))).sum((2, 3)) for k in range(16)], 1)


def border_tap_mask():
    m = torch.ones(4, 3)
    m[2, 0] = m[3, 0] = 0.0
    m[1, 2] = m[3, 2] = 0.0
    return m


def gate(y, strict=True):
    """True where the PReLU passed its input through: ``y > 0`` (strict=False: the ``>=`` mutant)"""
    return (y > 0) if strict else (y >= 0)


def _case(row, **kw):
    return SimpleNamespace(name=row.name, row=row, share={}, **kw)


# ---------------------------------------------------------------------------------------------------------------- conv_tp + dact

TP_TILE = (8, 32)          # TP_TH x TP_TW pixels of dPre (csrc/conv_tp.hip)


def tp_dact_ref(c, strict=True, dres_sign=None, skip_tile=None):
    """(dz, db, da, dres) of the issue's reference; the keyword arguments build the CPU test's mutants"""
    a = SLOPE
    neg = ~gate(c.y, strict)
    dz = torch.where(neg, c.tot * a, c.tot)
    terms = torch.where(neg, c.tot * c.y, torch.zeros(()))
    dzs = dz
    if skip_tile is not None:          # one tile's partial left out of the sums
        keep = torch.ones_like(dz)
        n, ty, tx = skip_tile
        keep[n, :, 4 * TP_TILE[0] * ty:4 * TP_TILE[0] * (ty + 1), 4 * TP_TILE[1] * tx:4 * TP_TILE[1] * (tx + 1)] = 0
        dzs, terms = dz * keep, terms * keep
    db = dzs.sum((0, 2, 3))
    da = terms.sum() / a
    sign = dres_sign if dres_sign is not None else {None: 0.0, "sub": -1.0, "add": 1.0}[c.res_mode]
    return dz, db, da, sign * c.tot


def build_tp_dact(row, H=8, W=64, N=2, C=128, neg=1.0 / 32):
    g = _gen(row.name)
    k, s, p = 8, 4, 2
    res_mode = row.args.get("res")
    c = _case(row, N=N, C=C, H=H, W=W, IH=s * H, IW=s * W, res_mode=res_mode, acc=res_mode is None)
    K = 4 * C
    dens = XL.density_for(K)
    c.w = XL.draw((C, C, k, k), QW, amp=2, density=dens, gen=g)
    c.dpre = XL.draw((N, C, H, W), QX, amp=2, density=dens, gen=g)
    XL.assert_sum_bound(K, 2.0 ** (1 - QX), 2.0 ** (1 - QW), UNIT, row.name)
    xr = torch.zeros(N, C, c.IH, c.IW, requires_grad=True)
    F.conv2d(xr, c.w, None, s, p).backward(c.dpre)
    tot = xr.grad.detach()
    XL.assert_on_lattice(tot, UNIT, row.name + " dgrad")
    c.old = XL.draw(tot.shape, QB, amp=64, density=1.0, gen=g) if c.acc else None
    c.tot = tot + c.old if c.acc else tot
    XL.assert_fp16_exact(c.tot, row.name + " tot")
    c.y = draw_gate(tot.shape, g, neg=neg)
    c.bias0 = XL.draw((C,), QB, amp=64, density=1.0, gen=g)
    if res_mode is None:
        c.res, c.saved = None, c.y
    else:          # RES_SUB: out = act - res, the kernel rebuilds act = saved + res; RES_ADD: out = act + res, act = saved - res
        c.res = XL.draw(tot.shape, QB, amp=64, density=1.0, gen=g)
        c.saved = c.y - c.res if res_mode == "sub" else c.y + c.res
        XL.assert_fp16_exact(c.saved, row.name + " saved output")
    c.dz, c.db, c.da, c.dres = tp_dact_ref(c)
    XL.assert_on_lattice(c.dz, UNIT * SLOPE, row.name + " dz")
    XL.assert_fp16_exact(c.dz, row.name + " dz")
    assert_share(c, "bias sums", c.dz, UNIT * SLOPE, (0, 2, 3))
    assert_share(c, "slope sum", torch.where(c.y > 0, torch.zeros(()), c.tot * c.y), UNIT / 16)      # tot (2^-5) x y (2^-4)
    XL.assert_fp32_exact(c.db, row.name + " db")
    XL.assert_fp32_exact(c.da, row.name + " da")
    return c


# ---------------------------------------------------------------------------------------------------------------- thin DACT

def thin_dact_ref(c, strict=True, dres_sign=None):
    neg = ~gate(c.y, strict)
    dz = torch.where(neg, c.tot * SLOPE, c.tot)
    da = torch.where(neg, c.tot * c.y, torch.zeros(())).sum() / SLOPE
    return dz, da, (dres_sign if dres_sign is not None else (1.0 if c.res_mode == "add" else -1.0)) * c.tot


def build_thin_dact(row):
    g = _gen(row.name)
    a = row.args
    cout, H, W, N = a["cout"], a["H"], a["W"], 2
    c = _case(row, N=N, cout=cout, H=H, W=W, res_mode=a["res"])
    c.w = XL.draw((3, cout, 3, 3), QW, amp=2, density=0.5, gen=g)          # the head conv: cout features -> 3 image channels
    c.dimg = XL.draw((N, 3, H, W), QX, amp=2, density=0.5, gen=g)
    c.old = XL.draw((N, cout, H, W), QB, amp=64, density=1.0, gen=g)
    XL.assert_sum_bound(27, 2.0 ** (1 - QX), 2.0 ** (1 - QW), UNIT, row.name)
    c.tot = c.old + F.conv_transpose2d(c.dimg, c.w, None, 1, 1)              # dgrad of conv2d(x, w[3, cout]) wrt x
    XL.assert_on_lattice(c.tot, UNIT, row.name + " tot")
    XL.assert_fp16_exact(c.tot, row.name + " tot")
    c.y = draw_gate(c.tot.shape, g, neg=1.0 / 8, zero=1.0 / 32)
    c.res = XL.draw(c.tot.shape, QB, amp=64, density=1.0, gen=g)
    c.saved = c.y + c.res if c.res_mode == "add" else c.y - c.res
    XL.assert_fp16_exact(c.saved, row.name + " saved output")
    c.dz, c.da, c.dres = thin_dact_ref(c)
    XL.assert_fp16_exact(c.dz, row.name + " dz")
    assert_share(c, "slope sum", torch.where(c.y > 0, torch.zeros(()), c.tot * c.y), UNIT / 16)
    XL.assert_fp32_exact(c.da, row.name + " da")
    return c


# ---------------------------------------------------------------------------------------------------------------- conv_kbup

def kbup_ref(c, strict=True):
    """(dPre, da) of the layer's backward; the weight gradient is autograd's under dPre"""
    pos = gate(c.pre, strict)
    dpre = torch.where(pos, c.dout, c.dout * SLOPE)
    da = (c.dout * torch.where(pos, torch.zeros(()), c.pre)).sum()
    return dpre, da


def build_kbup(row):
    g = _gen(row.name)
    a = row.args
    cout, h, w, N = a["cout"], a["h"], a["w"], 2
    c = _case(row, N=N, cout=cout, h=h, w=w)
    # sparse operands: a 12-term pre-activation is then exactly zero on many pixels, which pins the sign convention at pre == 0
    c.x = XL.draw((N, 3, h, w), QX, amp=2, density=0.4, gen=g)
    c.wt = XL.draw((3, cout, 8, 8), QW, amp=2, density=0.4, gen=g)
    c.dout = XL.draw((N, cout, 4 * h, 4 * w), QX, amp=2, density=0.75, gen=g)
    XL.assert_sum_bound(12, 2.0 ** (1 - QX), 2.0 ** (1 - QW), UNIT, row.name)
    c.pre = F.conv_transpose2d(c.x, c.wt, None, 4, 2)
    XL.assert_on_lattice(c.pre, UNIT, row.name + " pre-activation")
    c.dpre, c.da = kbup_ref(c)
    XL.assert_on_lattice(c.dpre, 2.0 ** -QX * SLOPE, row.name + " dPre")
    XL.assert_fp16_exact(c.dpre, row.name + " dPre")
    wr = c.wt.clone().requires_grad_(True)
    F.conv_transpose2d(c.x, wr, None, 4, 2).backward(c.dpre)
    c.dw = wr.grad.detach()
    ugw = 2.0 ** -QX * 2.0 ** -QX * SLOPE          # x (2^-2) x dPre (2^-4)
    XL.assert_on_lattice(c.dw, ugw, row.name + " weight gradient")
    XL.assert_fp32_exact(c.dw, row.name + " weight gradient")
    wa = torch.ones_like(c.wt).requires_grad_(True)          # sum |x| |dPre| per weight element: the terms of the kernel's sums
    F.conv_transpose2d(c.x.abs(), wa, None, 4, 2).backward(c.dpre.abs())
    assert_share(c, "weight gradient", wa.grad.detach().max().reshape(1), ugw)
    assert_share(c, "slope sum", c.dout * torch.clamp(c.pre, max=0.0), 2.0 ** -QX * UNIT)
    XL.assert_fp32_exact(c.da, row.name + " da")
    return c


# ---------------------------------------------------------------------------------------------------------------- folded constant segment

def _act(t, act):
    return t if act == "none" else torch.where(t > 0, t, t * SLOPE)


def build_folded_fwd(row, cf=128, cc=21, N=2):
    g = _gen(row.name)
    a = row.args
    cout, H, W = a["cout"], a["H"], a["W"]
    c = _case(row, N=N, cf=cf, cc=cc, cout=cout, H=H, W=W, modes=tuple(a["modes"]))
    K = 9 * (cf + cc)
    dens = XL.density_for(K)
    c.x = XL.draw((N, cf, H, W), QX, amp=2, density=dens, gen=g)
    c.kvec = XL.draw((N, cc), QX, amp=2, density=1.0, gen=g)
    c.w = XL.draw((cout, cf + cc, 3, 3), QW, amp=2, density=dens, gen=g)
    c.b = XL.draw((cout,), QB, amp=64, density=1.0, gen=g)
    XL.assert_sum_bound(K, 2.0 ** (1 - QX), 2.0 ** (1 - QW), UNIT, row.name)
    pre = F.conv2d(torch.cat([c.x, c.kvec[:, :, None, None].expand(N, cc, H, W)], 1), c.w, c.b, 1, 1)
    XL.assert_on_lattice(pre, UNIT, row.name + " pre-activation")
    c.pre, c.ref = pre, _act(pre, "lrelu")
    XL.assert_on_lattice(c.ref, UNIT * SLOPE, row.name)
    XL.assert_fp16_exact(c.ref, row.name)
    kx = torch.cat([c.x, c.kvec[:, :, None, None].expand(N, cc, H, W)], 1).abs()
    assert_share(c, "pre-activation", F.conv2d(kx, c.w.abs(), c.b.abs(), 1, 1).max().reshape(1), UNIT)
    return c


def folded_bwd_ref(c, strict=True, drop=None):
    """(dk, dprelu): the parts that depend on the border classes / the gate (``drop``: one border class left out of the sums)"""
    S = class_sums(c.dpre, drop).reshape(c.N, 4, 4, c.cout)
    m = border_tap_mask()
    St = torch.einsum("nabo,ay,bx->noyx", S, m, m)
    dk = torch.einsum("ocyx,noyx->nc", c.w[:, c.cf:], St)
    dwc = torch.einsum("noyx,nc->ocyx", St, c.kvec)
    da = torch.where(gate(c.out, strict), torch.zeros(()), c.dpre * c.out).sum() / (SLOPE * SLOPE)
    return dk, dwc, da


def build_folded_bwd(row, cf=128, cc=21, cout=100, N=2):
    g = _gen(row.name)
    H, W = row.args["H"], row.args["W"]
    c = _case(row, N=N, cf=cf, cc=cc, cout=cout, H=H, W=W, prelu=row.args["prelu"])
    c.x = XL.draw((N, cf, H, W), QX, amp=2, density=0.5, gen=g)
    c.kvec = XL.draw((N, cc), QX, amp=2, density=1.0, gen=g)
    c.w = XL.draw((cout, cf + cc, 3, 3), QW, amp=2, density=0.5, gen=g)
    # (sparser on the large maps: dL/dk contracts the class sums of |dPre| with every weight of the constant half)
    c.dpre = XL.draw((N, cout, H, W), QW, amp=2, density=0.5 if H * W < 1024 else 0.25, gen=g)
    c.out = draw_gate((N, cout, H, W), g, neg=1.0 / 4, zero=1.0 / 16)          # the layer's saved output
    ug = 2.0 ** -(QX + QW)
    XL.assert_sum_bound(N * H * W, 2.0 ** (1 - QX), 2.0 ** (1 - QW), ug, row.name)
    wr = c.w.clone().requires_grad_(True)
    kb = c.kvec[:, :, None, None].expand(N, cc, H, W).clone().requires_grad_(True)
    F.conv2d(torch.cat([c.x, kb], 1), wr, None, 1, 1).backward(c.dpre)
    c.dw, c.dk = wr.grad.detach(), kb.grad.detach().sum((2, 3))
    c.db = c.dpre.sum((0, 2, 3))
    XL.assert_on_lattice(c.dw, ug, row.name + " weight gradient")
    XL.assert_fp32_exact(c.dw, row.name + " weight gradient")
    XL.assert_on_lattice(c.dk, 2.0 ** -(QW + QW), row.name + " dL/dk")
    XL.assert_fp32_exact(c.dk, row.name + " dL/dk")
    dk, dwc, c.da = folded_bwd_ref(c)
    assert torch.equal(dk, c.dk) and torch.equal(dwc, c.dw[:, cf:]), f"{row.name}: the class-sum form is not autograd's"
    assert_share(c, "class sums of dPre", c.dpre, 2.0 ** -QW, (0, 2, 3))
    assert_share(c, "dL/dk", torch.einsum("ocyx,no->nc", c.w[:, cf:].abs(), c.dpre.abs().sum((2, 3))), 2.0 ** -(QW + QW), None)
    assert_share(c, "slope sum", torch.where(c.out > 0, torch.zeros(()), c.dpre * c.out), 2.0 ** -(QW + 4))
    XL.assert_fp32_exact(c.da, row.name + " da")
    c.classes = sorted(set(class_index(H, W).reshape(-1).tolist()))
    return c


def build_const_1x1(row, c0=16, c1=128, cout=100, N=2, H=9, W=11):
    g = _gen(row.name)
    c = _case(row, N=N, c0=c0, c1=c1, cout=cout, H=H, W=W, stat=row.args["stat"])
    K = c0 + c1
    c.x = XL.draw((N, c1, H, W), QX, amp=2, density=0.5, gen=g)
    c.cvec = XL.draw((N, c0), QX, amp=2, density=1.0, gen=g)
    c.w = XL.draw((cout, K, 1, 1), QW, amp=2, density=0.5, gen=g)
    c.b = None if c.stat else XL.draw((cout,), QB, amp=64, density=1.0, gen=g)          # (conv + BatchNorm carries no bias or activation)
    assert_k_bound(c, "K sum", K)
    pre = F.conv2d(torch.cat([c.cvec[:, :, None, None].expand(N, c0, H, W), c.x], 1), c.w, c.b, 1, 0)
    XL.assert_on_lattice(pre, UNIT, row.name + " pre-activation")
    c.pre, c.ref = pre, _act(pre, "none" if c.stat else "lrelu")
    XL.assert_fp16_exact(c.ref, row.name)
    if c.stat:
        XL.assert_sq_sum_bound(pre, UNIT, (0, 2, 3), row.name)
        assert_share(c, "BatchNorm sums of squares", pre * pre, UNIT * UNIT, (0, 2, 3))
        c.ref_stat = torch.stack([pre.sum((0, 2, 3)), (pre * pre).sum((0, 2, 3))])
    return c


# ---------------------------------------------------------------------------------------------------------------- ShuffleConv

def shuffle_fwd(x, W, s):
    return _act(F.pixel_shuffle(F.conv2d(x, W, None, 1, 1), s), "prelu")


def build_shuffle(row, N=2):
    g = _gen(row.name)
    a = row.args
    s, cin, C, H, W = a["s"], a["cin"], a["C"], a["H"], a["W"]
    c = _case(row, N=N, s=s, cin=cin, C=C, H=H, W=W)
    Kf, Kd = 9 * cin, 9 * C * s * s
    c.x = XL.draw((N, cin, H, W), QX, amp=2, density=XL.density_for(Kf), gen=g)
    c.Wm = XL.draw((C * s * s, cin, 3, 3), QW, amp=2, density=XL.density_for(Kf), gen=g)
    c.Wm2 = XL.draw((C * s * s, cin, 3, 3), QW, amp=2, density=XL.density_for(Kf), gen=g)          # the weights after an optimiser step
    assert_k_bound(c, "forward K sum", Kf)
    c.ref, c.ref2 = shuffle_fwd(c.x, c.Wm, s), shuffle_fwd(c.x, c.Wm2, s)
    for t in (c.ref, c.ref2):
        XL.assert_on_lattice(t, UNIT * SLOPE, row.name + " forward")
        XL.assert_fp16_exact(t, row.name + " forward")
    assert not torch.equal(c.ref, c.ref2)
    # dgrad: its own, sparser operands (9 C s^2 terms per input pixel)
    dd = XL.density_for(Kd)
    c.Wd = XL.draw(c.Wm.shape, QW, amp=2, density=dd, gen=g)
    c.dpre = XL.draw((N, C, s * H, s * W), QX, amp=2, density=dd, gen=g)
    assert_k_bound(c, "dgrad K sum", Kd)
    xr = torch.zeros(N, cin, H, W, requires_grad=True)
    F.pixel_shuffle(F.conv2d(xr, c.Wd, None, 1, 1), s).backward(c.dpre)
    c.dx = xr.grad.detach()
    XL.assert_on_lattice(c.dx, UNIT, row.name + " dgrad")
    XL.assert_fp16_exact(c.dx, row.name + " dgrad")
    # wgrad in the master layout [C s^2, cin, 3, 3]
    c.dpre_w = XL.draw((N, C, s * H, s * W), QW, amp=2, density=0.5, gen=g)
    assert_k_bound(c, "wgrad pixel sum", N * H * W)
    wr = c.Wm.clone().requires_grad_(True)
    F.pixel_shuffle(F.conv2d(c.x, wr, None, 1, 1), s).backward(c.dpre_w)
    c.dW = wr.grad.detach()
    XL.assert_on_lattice(c.dW, UNIT, row.name + " wgrad")
    XL.assert_fp32_exact(c.dW, row.name + " wgrad")
    return c


# ---------------------------------------------------------------------------------------------------------------- kp_bwd

def pair_ref(c, strict=True):
    din = F.conv_transpose2d(c.dpre, c.w[:, :c.cin], None, 1, 0)
    return torch.where(gate(c.x, strict), din, din * SLOPE)


def build_pair(row, cin=49, cout=32):
    g = _gen(row.name)
    a = row.args
    N, H, W, cin_tot = a["N"], a["H"], a["W"], a["cin_tot"]
    c = _case(row, N=N, H=H, W=W, cin=cin, cout=cout, cin_tot=cin_tot)
    c.w = XL.draw((cout, cin_tot, 1, 1), QW, amp=2, density=0.75, gen=g)
    c.dpre = XL.draw((N, cout, H, W), QX, amp=2, density=0.75, gen=g)
    # the layer's saved input = the activation of the layer below: i / 4 with zeros and negatives (the gate and the wgrad operand)
    c.x = XL.draw((N, cin, H, W), QX, amp=2, density=0.8, gen=g)
    XL.assert_sum_bound(cout, 2.0 ** (1 - QX), 2.0 ** (1 - QW), UNIT, row.name)
    c.din = pair_ref(c)
    XL.assert_on_lattice(c.din, UNIT * SLOPE, row.name + " dIn")
    XL.assert_fp16_exact(c.din, row.name + " dIn")
    wr = c.w.clone().requires_grad_(True)
    F.conv2d(torch.cat((c.x, torch.zeros(N, cin_tot - cin, H, W)), 1), wr, None, 1, 0).backward(c.dpre)
    c.dw = wr.grad.detach()
    ug = 2.0 ** -(QX + QX)
    XL.assert_on_lattice(c.dw, ug, row.name + " wgrad")
    XL.assert_fp32_exact(c.dw, row.name + " wgrad")
    assert_share(c, "weight gradient", torch.einsum("nohw,nchw->oc", c.dpre.abs(), c.x.abs()).max().reshape(1), ug)
    return c


def fillsums_ref(c, strict=True, drop=None):
    """(class sums of the layer's input, folded weight gradient, masked dgrad fill)"""
    sums = class_sums(c.x, drop)
    mf = border_tap_mask().flip(1)
    S = torch.einsum("nabc,ay,bx->ncyx", sums.reshape(c.N, 4, 4, c.cin), mf, mf)
    dw = torch.einsum("no,ncyx->ocyx", c.g, S)
    xr = torch.zeros_like(c.x).requires_grad_(True)
    F.conv2d(xr, c.w, None, 1, 1).backward(c.g[:, :, None, None].expand(c.N, c.cout, c.H, c.W))
    din = xr.grad.detach()
    return sums, dw, torch.where(gate(c.x, strict), din, din * SLOPE)


def build_fillsums(row, N=2, cin=32, cout=49):
    g = _gen(row.name)
    H, W = row.args["H"], row.args["W"]
    c = _case(row, N=N, cin=cin, cout=cout, H=H, W=W)
    c.w = XL.draw((cout, cin, 3, 3), QW, amp=2, density=0.75, gen=g)
    c.g = XL.draw((N, cout), QX, amp=2, density=1.0, gen=g)          # dPre: one vector per sample (fp16-exact: the fold rounds it to fp16)
    c.x = XL.draw((N, cin, H, W), QX, amp=2, density=0.8, gen=g)      # the layer's input = the mask map of its dgrad
    XL.assert_sum_bound(9 * cout, 2.0 ** (1 - QX), 2.0 ** (1 - QW), UNIT, row.name)
    c.sums, c.dw, c.din = fillsums_ref(c)
    wr = c.w.clone().requires_grad_(True)
    F.conv2d(c.x, wr, None, 1, 1).backward(c.g[:, :, None, None].expand(N, cout, H, W))
    assert torch.equal(c.dw, wr.grad), f"{row.name}: the fold of the class sums is not autograd's weight gradient"
    XL.assert_fp32_exact(c.sums, row.name + " class sums")
    XL.assert_fp32_exact(c.dw, row.name + " wgrad")
    XL.assert_on_lattice(c.din, UNIT * SLOPE, row.name + " dIn")
    XL.assert_fp16_exact(c.din, row.name + " dIn")
    assert_share(c, "class sums", c.x, 2.0 ** -QX, (0, 2, 3))
    assert_share(c, "folded weight gradient", torch.einsum("no,nc->oc", c.g.abs(), c.x.abs().sum((2, 3))).max().reshape(1), 2.0 ** -(QX + QX))
    c.classes = sorted(set(class_index(H, W).reshape(-1).tolist()))
    return c


BUILDERS = {"tp_dact": build_tp_dact, "thin_dact": build_thin_dact, "kbup": build_kbup, "folded_fwd": build_folded_fwd,
            "folded_bwd": build_folded_bwd, "const_1x1": build_const_1x1, "shuffle": build_shuffle, "pair": build_pair,
            "fillsums": build_fillsums}

_CACHE = {}


def build(row):
    """the row's operands and reference: built once, shared by the tests of a session, never modified"""
    if row.name not in _CACHE:
        _CACHE[row.name] = BUILDERS[row.group](row)
    return _CACHE[row.name]
