"""The case table and the CPU reference of tests/test_split_conv_exact_gpu.py: the split-fp16 (hi + lo) convolution paths of the detector
precision mode on exact-lattice operands.  Plain data and CPU code, importable without a GPU: tests/test_split_conv_cases_cpu.py proves
every row's bounds and that every mutant of the reference (a dropped product, a forgotten out_scale, a lo plane rounded twice, ...)
changes the expected planes; tests/test_conv_exact_coverage_cpu.py counts the rows next to tests/conv_exact_cases.py's.

The lattice (tests/exact_lattice.py: draw_split_planes / draw_split_weights).  A forward conv of a split map sums
x_hi w_hi + x_lo w_hi + x_hi w_lo in ONE fp32 accumulator, so all three products must be whole multiples of one unit and the sum of their
magnitudes must stay below 2^24 units:
  x_hi = i 2^a, x_lo = j 2^(a - 13), |i|, |j| <= 2, the two planes drawn independently (plane arithmetic, not canonical pairs);
  scaled weights v = v_hi + v_lo, v_hi = k, v_lo = m 2^-13 where k != 0; the master weight is v / Conv.WSCALE, exact in fp32, and
  csbsr_pack_weights_split's fp16(v) / fp16(v - fp16(v)) give back exactly (v_hi, v_lo) -- asserted on a CPU emulation of the pack;
  density sqrt(150 / K): about 150 nonzero terms per product and output.
The largest product is 2^15 units (x_hi w_hi = 4 x 2^9 against the unit 2^-4), so a dense draw would break the bound (K = 1152 gives
2^25.2): the reference COUNTS the nonzero terms of every output on the drawn operands (a convolution of the nonzero masks) and proves
K_max x max|a| x max|b| summed over the products < 2^24 (XL.assert_products_bound: 2^20.1 to 2^22.26 units on these rows, around a
largest sum of |terms| of 2^19.5 to 2^21.35 units, which tests/test_split_conv_cases_cpu.py prints per row).  The mutants of the
reference change these shares of the expected elements (the same test prints them; a ReLU row halves each): a dropped x_lo w_hi or
x_hi w_lo 92 - 96 %, x_lo w_lo added 12 - 13 %, out_scale left out 98 - 100 %, a zero lo plane 92 - 96 % (8.6 % on the plan-1 row), a
lo plane rounded twice 27 - 52 %, the lo plane of the input shifted by 32 channels 96 %; on the dgrad rows no w_lo 19 %, rounded twice 6 %.  With a = 9
the output lattice is 2^-12 (2^-14 under the slope 0.25), so every nonzero value of both output planes is a normal fp16 number
(asserted: a unit input scale leaves most of the lo plane subnormal).

Row fields:
  op / entry  "fwd" Conv.fwd, "folded" Conv.fwd_folded, "const" Conv.fwd_const_1x1 (split feature input), "dgrad" Conv.bwd_input with
              hp_dgrad (a plain fp16 gradient against [w_hi | w_lo], plain fp16 output rounded once)
  shape       cin, cout, k, stride, pad, dilation and the layer's INPUT size N x H x W; ``segs``: folded (feature, constant) channels,
              const (constant, feature) channels, dgrad (segment 0, segment 1) channels of a two-segment layer + ``seg`` the one computed
  epi         fwd: activation (none / relu / lrelu / prelu, slope 0.25) + residual (_add / _sub / _fma: split pairs) or "bn" (BatchNorm sums);
              dgrad: "" / "acc"
  blocks      Conv.fwd_blocks of the layer (3 / 2 / 1);  ``fused``: Engine.split_fused
  plan        the plan whose products the reference sums: 3 / 4 = x_hi w_hi + x_lo w_hi + x_hi w_lo, 2 / 5 = (x_hi + x_lo) w_hi (the drawn
              v_lo must not appear), 1 = x_hi fp16(w) on plain operands.  4 / 5 are the fused stages of csrc/conv_igemm_glds.hip
              (csbsr_conv_desc_t::split_fused 1 / 2); 5 is also what csrc/conv_x3n.hip runs as 2 x Cp plain channels against [w | w]
  modes       as tests/conv_exact_cases.py
  kid / var   csbsr_debug_last_conv_kernel() & 255 / >> 8 (None where the dispatcher encodes no instance)
  budget      a conv_x3n row: run again under the CU budgets BUDGETS["default"], bit-identical
  out_c0      the output as channels [c0, c0 + coutp) of a wider split buffer, once per listed c0
  draw        overrides of DRAW (the BatchNorm rows: a narrow span, see there)
"""
import math
import os
import re
from collections import namedtuple
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import exact_lattice as XL

SLOPE = 0.25
QB = 5                       # bias, class-bias operands, old gradient: k / 32
DRAW = dict(a=9, shift=13, amp=2, target=150.0)
A_DGRAD = 8                  # hp dgrad: the plain gradient is i 2^8, so the scaled sum's lattice 2^(8 - 13 - 8) = 2^-13 is fp16-normal


def wscale():
    """Conv.WSCALE, read from csbsr_amd/engine.py (no GPU library needed)"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csbsr_amd", "engine.py")) as f:
        return float(re.search(r"^    WSCALE = ([0-9.]+)\s*$", f.read(), re.M).group(1))


WSCALE = wscale()

SRow = namedtuple("SRow", "name op entry mode cin cout k s p dil N H W epi blocks fused plan modes kid var budget out_c0 draw segs seg why")
ENTRY = {"fwd": "Conv.fwd", "folded": "Conv.fwd_folded", "const": "Conv.fwd_const_1x1", "dgrad": "Conv.bwd_input"}


def S(name, op, cin, cout, k, s, p, dil, N, H, W, epi="none", blocks=3, fused=1, plan=4, modes=(), kid=-1, var=None, budget=False,
      out_c0=(0,), draw=(), segs=(), seg=0, why=""):
    mode = "Conv.hp_dgrad" if op == "dgrad" else "split"
    return SRow(name, op, ENTRY[op], mode, cin, cout, k, s, p, dil, N, H, W, epi, blocks, fused, plan, tuple(modes), kid, var, budget,
                tuple(out_c0), tuple(dict(draw).items()), tuple(segs), seg, why)


X3N = (("conv_x3n", 2),)
# BatchNorm rows: the sums of squares must stay below 2^24 units^2, which a 2^13-wide pair of planes cannot (one output is ~2^20 units): the
# planes sit 2 bits apart, amplitude 1 -- the sums, not the lo plane, are what these rows are about (plan 5 multiplies no v_lo anyway)
NARROW = dict(shift=2, amp=1)
SPLIT_ROWS = [
    # ---- the fused three-product stage (plan 4, csrc/conv_igemm_glds.hip FS = true): instance bit 1; bit 2 = the general K walk.  A split
    # launch is offered no other family (csbsr_amd/engine.py FAMILIES: conv_hr / x3 / x3w / tp refuse ``sp``, conv_x3n takes plan 5 alone)
    S("fs_glds64", "fwd", 64, 64, 3, 1, 1, 1, 2, 40, 70, "lrelu", kid=14, var=1, why="33..64 couts: the 64-cout tile; 64-channel planes = whole 32-channel slices"),
    S("fs_glds128", "fwd", 128, 128, 3, 1, 1, 1, 2, 16, 16, "lrelu_sub", kid=3, var=1, why="128 couts, 512 pixels (< 65536): the 128 x 128 tile; split residual"),
    S("fs_glds256", "fwd", 128, 128, 3, 1, 1, 1, 1, 256, 256, "none", kid=4, var=1,
      why="[hi | lo] = 256 channels: Kp = 9 x 256 = 2304 and 65536 pixels reach the 256-row tile from 128-channel planes"),
    S("fs_glds256w", "fwd", 128, 256, 3, 1, 1, 1, 1, 256, 256, "relu", kid=7, var=1, why="as above, 256 couts: the 256 px x 256 cout tile"),
    S("fs_glds64_gk", "fwd", 48, 64, 3, 1, 1, 1, 2, 40, 44, "none", kid=14, var=3, why="48-channel planes: (ctot / 2) % 32 != 0, a 32-channel slice straddles taps"),
    S("fs_glds128_gk", "fwd", 48, 96, 3, 1, 1, 1, 2, 24, 40, "relu", kid=3, var=3, why="HRNet-W48 widths: general K walk on the 128 tile"),
    S("fs_glds256_gk", "fwd", 136, 128, 3, 1, 1, 1, 1, 256, 256, "relu", kid=4, var=3,
      why="136-channel planes (4 slices + 8: the ragged tail 264 has, at half the reference's cost): Kp = 2448 >= 2304, 65536 pixels"),
    S("fs_glds256w_gk", "fwd", 136, 256, 3, 1, 1, 1, 1, 256, 256, "lrelu", kid=7, var=3, why="as above, 256 couts"),
    S("fs_strided", "fwd", 64, 128, 3, 2, 1, 1, 2, 32, 32, "lrelu", kid=3, var=1, why="64 -> 128 stride 2, 16 x 16 out"),
    S("fs_dilated", "fwd", 64, 128, 3, 1, 2, 2, 2, 17, 19, "none", kid=3, var=1, why="dilation 2, pad 2 (PSPNet's dilated stages)"),
    S("fs_pad", "fwd", 128, 100, 3, 1, 1, 1, 2, 16, 16, "lrelu_add", kid=3, var=1, why="100 -> 104 padded couts: the pads of BOTH planes must be zero"),
    S("fs_1x1", "fwd", 128, 128, 1, 1, 0, 1, 2, 9, 11, "prelu", kid=3, var=1, why="1x1 (the PSP bottleneck's form): one tap, Kp = 256"),
    # ---- a split output slice, the way PSPNet's last block writes into the concat buffer (cat.slice(c0, c1): lo stays the buffer's plane pitch)
    S("fs_out_slice", "fwd", 64, 128, 3, 1, 1, 1, 2, 10, 12, "relu", kid=3, var=1, out_c0=(0, 128), why="output at c0 = 0 and c0 = 128 of a wider split buffer"),
    # ---- the fused two-product stage (plan 5): fwd_blocks = 2
    S("fs2_glds128", "fwd", 128, 128, 3, 1, 1, 1, 2, 16, 16, "lrelu", blocks=2, plan=5, kid=3, var=1,
      why="split_fused = 2 on the 128 tile (conv_x3n's default mode refuses a launch of 512 pixels)"),
    S("fs2_x3n_narrow", "fwd", 64, 64, 3, 1, 1, 1, 2, 19, 70, "lrelu", blocks=2, plan=5, modes=X3N, kid=20, var=1, budget=True,
      why="conv_x3n narrow: [hi | lo] as 128 plain channels against [w | w], straight-line rows"),
    S("fs2_x3n_wide", "fwd", 64, 200, 3, 1, 1, 1, 2, 19, 70, "relu", blocks=2, plan=5, modes=X3N, kid=20, var=13, budget=True,
      why="conv_x3n wide (200 > 64 couts), no residual: the lean instance"),
    S("fs2_x3n_bn", "fwd", 64, 64, 3, 1, 1, 1, 2, 19, 70, "bn", blocks=2, plan=5, modes=X3N, kid=20, var=3, budget=True, draw=NARROW,
      why="conv_x3n narrow + fused BatchNorm sums (the PSPNet decoder's up_2 / up_3 form)"),
    S("fs2_x3n_fma", "fwd", 64, 64, 3, 1, 1, 1, 2, 19, 70, "none_fma", blocks=2, plan=5, modes=X3N, kid=20, var=0, budget=True,
      why="BlurSkip's conv_shift.1: y = conv + q x scale, both residual operands split pairs: r_lo keeps it off the straight-line rows"),
    S("fs2_glds128_bn", "fwd", 128, 128, 3, 1, 1, 1, 2, 16, 16, "bn", blocks=2, plan=5, kid=3, var=1, draw=NARROW, why="BatchNorm sums from the fused stage of the 128 tile"),
    # ---- the unfused forms (Engine.split_fused = 0): K blocks [hi | lo] + hi against [w_hi | w_hi | w_lo], or [hi | lo] against [w_hi | w_hi]
    S("blocks3_glds128", "fwd", 128, 128, 3, 1, 1, 1, 2, 16, 16, "lrelu", fused=0, plan=3, kid=3, var=0, why="segments 256 + 128 channels, whole 64-channel slices: the plain 128 tile"),
    S("blocks2_glds128", "fwd", 128, 128, 3, 1, 1, 1, 2, 16, 16, "relu", blocks=2, fused=0, plan=2, kid=3, var=0, why="one 256-channel segment, plan 2 (conv_x3n is asked for plan 5 alone)"),
    S("blocks3_igemm64", "fwd", 16, 64, 3, 1, 1, 1, 2, 12, 12, "lrelu", plan=3, kid=1, var=None,
      why="16-channel planes (cp < 32: never fused): segments 32 + 16, not whole slices: the register-staged kernel, two segments"),
    S("blocks1_glds128", "fwd", 128, 128, 3, 1, 1, 1, 2, 16, 16, "lrelu", blocks=1, plan=1, kid=3, var=0, why="fwd_blocks = 1: the hi plane alone against plain fp16 weights, hi + lo output"),
    # ---- the fallback: a plan-4 launch the library refuses (LDS-DMA kernels off) runs the three-block form
    S("fs_fallback", "fwd", 128, 128, 3, 1, 1, 1, 2, 16, 16, "lrelu", modes=(("conv_glds", 0),), plan=4, kid=2, var=None,
      why="csbsr_conv_split_fused_eligible says no: Conv._launch packs [w_hi | w_hi | w_lo] and reaches the register-staged 128 kernel"),
    # ---- the other entry points, at the shapes of their plain rows (tests/fused_exact_cases.py)
    S("fs_folded", "folded", 149, 100, 3, 1, 1, 1, 2, 12, 20, "lrelu", kid=3, var=1, segs=(128, 21), why="Conv.fwd_folded, split feature segment: conv_x3 / x3w withhold themselves, the fused 128 tile"),
    S("fs2_folded_x3n", "folded", 149, 200, 3, 1, 1, 1, 2, 12, 20, "lrelu", blocks=2, plan=5, modes=X3N, kid=20, var=13, budget=True, segs=(128, 21),
      why="Conv.fwd_folded offers conv_x3n a split input under plan 5: the wide lean instance with the class-bias rows"),
    S("fs_const_1x1", "const", 144, 100, 1, 1, 0, 1, 2, 9, 11, "lrelu", kid=3, var=1, segs=(16, 128), why="Conv.fwd_const_1x1, split feature segment at k_off = 16"),
    # ---- high-precision dgrad (Conv.hp_dgrad): dY w_hi + dY w_lo, scaled, rounded once to fp16
    S("hp_dgrad", "dgrad", 128, 128, 3, 1, 1, 1, 2, 16, 16, "acc", plan=0, kid=3, var=0, out_c0=(0, 128),
      why="stride-1 3x3: the gradient passed twice, 128 + 128 channels, accumulating (again as channel slices of NaN / canary buffers)"),
    S("hp_dgrad_s2", "dgrad", 64, 128, 3, 2, 1, 1, 2, 32, 32, "", plan=0, kid=14, var=0, why="strided 3x3: the gather-form transposed launch into 64 channels"),
    S("hp_dgrad_seg1", "dgrad", 128, 128, 3, 1, 1, 1, 2, 16, 16, "", plan=0, kid=14, var=0, segs=(64, 64), seg=1, why="segment 1 of a two-segment layer: weight rows [64, 128)"),
]
BY_NAME = {r.name: r for r in SPLIT_ROWS}

MUTANTS = ("no_xlo_whi", "no_xhi_wlo", "plus_xlo_wlo", "no_out_scale", "lo_zero", "lo_rounded_twice", "xlo_shift32")
DGRAD_MUTANTS = ("no_wlo", "no_out_scale", "rounded_twice")


def mutants_of(row):
    """the mutants that change what this row's kernel must compute"""
    if row.op == "dgrad":
        return DGRAD_MUTANTS
    m = ["no_out_scale"]
    if row.plan != 1:
        m.append("no_xlo_whi")
    if row.plan in (3, 4):
        m += ["no_xhi_wlo", "plus_xlo_wlo"]
    if dict(row.draw).get("shift", DRAW["shift"]) >= 13:          # (the narrow-span rows' outputs fit the hi plane: their lo plane is zero)
        m.append("lo_zero")
        if row.plan != 1:           # (plan 1's values -- x_hi v_hi / WSCALE + bias, lattice 2^-5 -- have fewer than 16 bits: nothing to round twice)
            m.append("lo_rounded_twice")
    if row.var is not None and row.var & 2 and row.plan == 4:
        m.append("xlo_shift32")
    return tuple(m)


def _gen(name):
    return torch.Generator().manual_seed(sum(map(ord, name)) + 13)


def out_hw(r):
    return (r.H + 2 * r.p - r.dil * (r.k - 1) - 1) // r.s + 1, (r.W + 2 * r.p - r.dil * (r.k - 1) - 1) // r.s + 1


def split_pair(t):
    """value -> (hi, lo) as conv_common.h's split_store: hi = fp16(t), lo = fp16(t - hi)"""
    t = t.float()
    hi = t.half()
    return hi, (t - hi.float()).half()


def _exact(t64, what):
    XL.assert_fp32_exact(t64, what)
    return t64


def _act(t, act):
    return t if act == "none" else (torch.relu(t) if act == "relu" else torch.where(t > 0, t, t * SLOPE))


# ---------------------------------------------------------------------------------------------------------------- forward rows

def _conv(r, x, w):
    return F.conv2d(x, w, None, r.s, r.p, r.dil)


def _plan_operands(c, plan, mutant=None):
    """(input, weight) channel blocks of the plan's products, as lists to concatenate"""
    x_lo = torch.roll(c.x_lo, 32, 1) if mutant == "xlo_shift32" else c.x_lo
    xs, ws = [c.x_hi], [c.v_hi]
    if plan != 1 and mutant != "no_xlo_whi":
        xs.append(x_lo), ws.append(c.v_hi)
    if plan in (3, 4) and mutant != "no_xhi_wlo":
        xs.append(c.x_hi), ws.append(c.v_lo)
    return xs, ws


def _build_fwd(row):
    r, g = row, _gen(row.name)
    d = dict(DRAW, **dict(r.draw))
    a, sh, amp = d["a"], d["shift"], d["amp"]
    csp = {"fwd": r.cin, "folded": r.segs[0] if r.segs else 0, "const": r.segs[1] if r.segs else 0}[r.op]
    K = r.k * r.k * csp
    dens = XL.density_for(K, d["target"])
    c = SimpleNamespace(name=r.name, row=r, csp=csp, N=r.N)
    c.OH, c.OW = out_hw(r)
    c.x_hi, c.x_lo = XL.draw_split_planes((r.N, csp, r.H, r.W), a, amp, dens, sh, g)
    c.v_hi, c.v_lo = XL.draw_split_weights((r.cout, csp, r.k, r.k), amp, dens, 13, g)
    c.w_split = ((c.v_hi.double() + c.v_lo.double()) / WSCALE).float()
    assert torch.equal(c.w_split.double() * WSCALE, c.v_hi.double() + c.v_lo.double()), f"{r.name}: the master weight v / WSCALE is not fp32-exact"
    # 1. + 2. the pack on the CPU (csrc/pack.hip pack_weights_kernel: v = w * wscale, hi = fp16(v), lo = fp16(v - hi)) gives the drawn planes back
    v = c.w_split * WSCALE
    p_hi = v.half()
    p_lo = (v - p_hi.float()).half()
    assert torch.equal(p_hi.float(), c.v_hi) and torch.equal(p_lo.float(), c.v_lo), f"{r.name}: the emulated pack does not return the drawn (v_hi, v_lo)"
    assert torch.equal(c.w_split.half().float() * WSCALE, c.v_hi), f"{r.name}: fp16(w) is not v_hi / WSCALE (the plain operand of plan 1)"
    # the bound: nonzero terms per output and product, counted on the drawn operands
    ind = _conv(r, torch.cat([(c.x_hi != 0).float(), (c.x_lo != 0).float()], 0), (c.v_hi != 0).float())
    k_hh, k_lh = float(ind[:r.N].max()), float(ind[r.N:].max())
    ux, uw = 2.0 ** a, 2.0 ** (a - sh)
    products = [(k_hh, amp * ux, amp, ux)]
    if r.plan != 1:
        products.append((k_lh, amp * uw, amp, uw))
    if r.plan in (3, 4):
        products.append((k_hh, amp * ux, amp * 2.0 ** -13, 2.0 ** (a - 13)))      # (v_lo is nonzero only where v_hi is: K_hl <= K_hh)
    c.unit = min(u for *_, u in products)
    c.span = XL.assert_products_bound(products, c.unit, r.name)
    c.k_terms = (k_hh, k_lh)
    # 3. + 4. the plan's products as ONE fp32 convolution over concatenated channels; on the lattice (fp32-exact under the bound above: the CPU
    # test repeats the small rows in fp64)
    xs, ws = _plan_operands(c, r.plan)
    c.pre = _conv(r, torch.cat(xs, 1), torch.cat(ws, 1))
    XL.assert_on_lattice(c.pre, c.unit, r.name + " accumulator")
    # the epilogue's operands
    c.bn = r.epi == "bn"
    act, _, res = ("none", "", "") if c.bn else r.epi.partition("_")
    c.act, c.res = act, res
    c.b = None if c.bn else XL.draw((r.cout,), QB, amp=64, density=1.0, gen=g)
    c.cb_map = None
    if r.op == "folded":            # the constant segment: plain lattice operands, folded by the engine in fp32 (exact on the lattice)
        cc = r.segs[1]
        c.kvec = XL.draw((r.N, cc), 2, amp=2, density=1.0, gen=g)
        c.w_const = XL.draw((r.cout, cc, 3, 3), 3, amp=2, density=0.5, gen=g)
        c.cb_map = F.conv2d(c.kvec[:, :, None, None].expand(r.N, cc, r.H, r.W), c.w_const, None, 1, 1)
    if r.op == "const":
        c0 = r.segs[0]
        c.cvec = XL.draw((r.N, c0), 2, amp=2, density=1.0, gen=g)
        c.w_const = XL.draw((r.cout, c0, 1, 1), 3, amp=2, density=0.5, gen=g)
        c.cb_map = (c.cvec @ c.w_const[:, :, 0, 0].t())[:, :, None, None].expand(r.N, r.cout, c.OH, c.OW)
    c.r1 = c.r2 = None
    oshape = (r.N, r.cout, c.OH, c.OW)
    if res in ("add", "sub"):       # a split pair on the output lattice: hi = i / 4, lo = j 2^-12
        c.r1 = (XL.draw(oshape, 2, amp=8, density=1.0, gen=g), XL.draw(oshape, 12, amp=2, density=0.5, gen=g))
    if res == "fma":                # q x scale, both split pairs a few bits wide (their product must stay fp32-exact): hi = i, lo = j / 64
        c.r1 = (XL.draw(oshape, 0, amp=2, density=1.0, gen=g), XL.draw(oshape, 6, amp=2, density=0.5, gen=g))
        c.r2 = (XL.draw(oshape, 0, amp=2, density=1.0, gen=g), XL.draw(oshape, 6, amp=2, density=0.5, gen=g))
    c.hi, c.lo, c.t, c.stat = expected(c)
    # (the output lattice: the scaled accumulator's, the bias's / class bias's 2^-5, the residual pairs' 2^-12; times the slope)
    c.out_unit = min([c.unit / WSCALE] + ([2.0 ** -QB] if c.b is not None else []) + ([2.0 ** -12] if res else [])) * (1.0 if act == "none" else SLOPE)
    XL.assert_on_lattice(c.t, c.out_unit, r.name + " output")
    XL.assert_fp16_normal(c.hi, r.name + " hi plane")
    XL.assert_fp16_normal(c.lo, r.name + " lo plane")
    assert bool(torch.isfinite(c.hi.float()).all()), f"{r.name}: the hi plane overflows fp16"
    return c


def expected(c, mutant=None):
    """(hi, lo, t, stat) of a forward row: steps 3 - 6 of the reference; ``mutant`` changes one of them (the CPU test: each must show)"""
    r = c.row
    if mutant in ("no_xlo_whi", "no_xhi_wlo", "xlo_shift32"):
        xs, ws = _plan_operands(c, r.plan, mutant)
        pre = _conv(r, torch.cat(xs, 1), torch.cat(ws, 1)).double()
    elif mutant == "plus_xlo_wlo":  # the full (hi + lo)(hi + lo) product, in fp64
        pre = c.pre.double() + _conv(r, c.x_lo.double(), c.v_lo.double())
    else:
        pre = c.pre.double()
    strict = mutant is None
    step = (lambda t, what: _exact(t, f"{r.name} {what}")) if strict else (lambda t, what: t)
    # 5. out_scale, bias (+ the constant segment's class bias), activation, residual: each step exact in fp32
    t = step(pre if mutant == "no_out_scale" else pre / WSCALE, "out_scale")
    if c.b is not None:
        t = step(t + c.b.double()[None, :, None, None], "bias")
    if c.cb_map is not None:
        t = step(t + c.cb_map.double(), "class bias")
    t = step(_act(t, c.act), "activation")
    stat = None
    if c.bn:
        if strict:
            XL.assert_sq_sum_bound(t, c.unit / WSCALE, (0, 2, 3), r.name)
        stat = torch.stack([t.sum((0, 2, 3)), (t * t).sum((0, 2, 3))]).float()
    if c.res in ("add", "sub"):
        rv = step(c.r1[0].double() + c.r1[1].double(), "residual pair")
        t = step(t + rv if c.res == "add" else t - rv, "residual")
    elif c.res == "fma":
        rv, r2v = step(c.r1[0].double() + c.r1[1].double(), "residual pair"), step(c.r2[0].double() + c.r2[1].double(), "scale pair")
        t = step(t + step(rv * r2v, "q x scale"), "fma")
    # 6. the hi + lo store
    t32 = t.float()
    hi, lo = split_pair(t32)
    if mutant == "lo_zero":
        lo = torch.zeros_like(lo)
    if mutant == "lo_rounded_twice":        # t through a 16-bit significand before the split: the lo plane of a value rounded on the way
        m, e = torch.frexp(t32)
        lo = (torch.ldexp(torch.round(m * 65536.0) / 65536.0, e) - hi.float()).half()
    return hi, lo, t32, stat


# ---------------------------------------------------------------------------------------------------------------- hp dgrad rows

def _dgrad(r, dpre, w):
    xr = torch.zeros(r.N, w.shape[1], r.H, r.W, dtype=w.dtype, requires_grad=True)
    F.conv2d(xr, w, None, r.s, r.p, r.dil).backward(dpre.to(w.dtype))
    return xr.grad.detach()


def _build_dgrad(row):
    r, g = row, _gen(row.name)
    c = SimpleNamespace(name=r.name, row=r, N=r.N)
    c.OH, c.OW = out_hw(r)
    taps = r.k * r.k if r.s == 1 else ((r.k + r.s - 1) // r.s) ** 2
    dens = XL.density_for(taps * r.cout, DRAW["target"])
    c.v_hi, c.v_lo = XL.draw_split_weights((r.cout, r.cin, r.k, r.k), 2, dens, 13, g)
    c.w_split = ((c.v_hi.double() + c.v_lo.double()) / WSCALE).float()
    v = c.w_split * WSCALE
    p_hi = v.half()
    assert torch.equal(p_hi.float(), c.v_hi) and torch.equal((v - p_hi.float()).half().float(), c.v_lo), f"{r.name}: the emulated pack does not return (v_hi, v_lo)"
    c.dpre = XL.draw((r.N, r.cout, c.OH, c.OW), 0, amp=2, density=dens, gen=g) * 2.0 ** A_DGRAD
    c.c_lo, c.c_hi = (0, r.cin) if not r.segs else ((0, r.segs[0]) if r.seg == 0 else (r.segs[0], r.cin))
    c.cseg = c.c_hi - c.c_lo
    sl = slice(c.c_lo, c.c_hi)
    k_max = float(_dgrad(r, (c.dpre != 0).float(), (c.v_hi != 0).float()[:, sl]).max())
    u = 2.0 ** A_DGRAD
    c.unit = u * 2.0 ** -13
    c.span = XL.assert_products_bound([(k_max, 2 * u, 2, u), (k_max, 2 * u, 2 * 2.0 ** -13, c.unit)], c.unit, r.name)
    c.g_hi, c.g_lo = _dgrad(r, c.dpre, c.v_hi[:, sl]), _dgrad(r, c.dpre, c.v_lo[:, sl])
    XL.assert_on_lattice(c.g_hi, u, r.name + " dY w_hi")
    XL.assert_on_lattice(c.g_lo, c.unit, r.name + " dY w_lo")
    c.old = XL.draw(c.g_hi.shape, QB, amp=64, density=1.0, gen=g) if "acc" in r.epi else None
    c.ref, c.t = expected_dgrad(c)
    XL.assert_fp16_normal(c.ref, r.name + " gradient")
    return c


def expected_dgrad(c, mutant=None):
    """(fp16 gradient, exact fp32 value before the store) of an hp dgrad row"""
    r = c.row
    step = (lambda t, what: _exact(t, f"{r.name} {what}")) if mutant is None else (lambda t, what: t)
    t = step(c.g_hi.double() + (0 if mutant == "no_wlo" else c.g_lo.double()), "the two passes' sum")
    t = step(t if mutant == "no_out_scale" else t / WSCALE, "out_scale")
    if mutant == "rounded_twice":      # to 12 significant bits first: the second rounding then meets ties the exact value does not have
        m, e = torch.frexp(t)
        t = torch.ldexp(torch.round(m * 4096.0) / 4096.0, e)
    if c.old is not None:
        t = step(t + c.old.double(), "accumulate")
    return t.float().half(), t.float()


# ---------------------------------------------------------------------------------------------------------------- cache

_CACHE = {}


def build(row):
    """the operands and the reference of one row, computed once per process and shared (nothing writes to a built case)"""
    c = _CACHE.get(row.name)
    if c is None:
        c = _CACHE[row.name] = (_build_dgrad if row.op == "dgrad" else _build_fwd)(row)
    return c


def span_log2(c):
    return math.log2(c.span)
