"""Exact / bounded parity of the plain-fp16 kernels of csrc/elementwise.hip through the C ABI: the border-class and ring-class family
(fill, masked fill, sums, sums + PReLU dot, fill + sums of the mask; 11 kernels), the weighted pool and its adjoint, the adaptive average
pool both ways, the bilinear resize both ways (six kernels; and the fp32 pair csbsr_bilinear32_* of csrc/image_ops.hip), the epilogue
backward, batch norm (apply, backward, finalize), the instance-norm backward, the max pool's plain entry points and the small kernels
(axpby, sum_act, fill, the two layout converters, dc_bias, channel_mean_sub) -- at the smallest shapes that cross each dispatch
threshold, chunk seam and channel-group edge.  References, input builders, case tables and the mutants that show the inputs
discriminate: tests/elementwise_cases.py (validated without a GPU by tests/test_elementwise_cases_cpu.py).  The guarded call harness
is tests/abi_harness.py: NaN-refilled reduction scratch, NaN round every input (margins, and for an fp16 map the other channels of the
buffer it is a slice of), sentinels round every output, every row twice with identical bits.  fp16 maps run as a whole map (ld == c)
and as channels [8, 8 + c) of a buffer c + 24 channels wide.

"Bit for bit" below: the two runs of a row are compared as bit patterns; against the reference a row is compared by VALUE in the
output's own format (every element equal to the fp64 reference, which the format holds exactly) -- the sign of a zero is not asked.

What is exact, what carries a bound, and why:

  class sums      x on 2^-4 {-15 .. 15}, at most 4620 pixels per class: any order of summation is exact in fp32, and so is
                  interior = total - border.  Asked BIT FOR BIT on a zeroed ``sums`` and on one preset with lattice values (the
                  entry points accumulate), on both sides of the 1024-pixel threshold; negdot (products of two lattices) likewise.
  class fills     a copy of an fp16-exact V (x a power-of-two slope): bit for bit.  fill_masked_sums: out bit for bit fill_masked's,
                  sums bit for bit border_class_sums of the mask.
  weighted pool   w on 2^-6, x on 2^-4, hw <= 2100: out, dw and the accumulated fp16 dx bit for bit.
  adaptive pool   windows of 4, 16 or 64 pixels: the mean of lattice values is exact, forward and backward (stored and accumulated), bit
                  for bit.  Ragged windows: |got - ref| <= n 2^-24 sum|terms| + 2^-11 |ref| with n = count + 1 forward (count - 1
                  additions, the reciprocal, the product) and n = 13 backward (elementwise_cases.AAP_BWD_ROUNDINGS).  8 x 8 -> 6 has
                  overlapping windows of four pixels: exact too, and asked bit for bit.
  bilinear        dyadic source positions (x2, x4, x8 without align_corners; 5 -> 9, 9 -> 33, 129 -> 257, 33 -> 65 with): weights are
                  multiples of 1 / 16, x integers in {-7 .. 7}: forward and backward, with and without the dropout scale row (scales 0,
                  1 / 2, 1, 2), stored and accumulated, bit for bit through all six kernels.
  bilinear, other ratios (5x7 -> 20x21, 23x31 -> 50x70, the 6x6 -> 1x1 down-scale; fp16 and fp32 kernels): the kernels' fp32 source
                  position is off by at most 3 x 2^-24 x in per axis, which moves the result by at most 3 (H + W) 2^-24 T, T = the sum
                  of |x| over the 4 x 4 pixels round the position; plus 12 roundings of the arithmetic (backward: K + 8, K = the outputs
                  within two pixels of the input pixel); plus the fp16 store.  Written out at elementwise_cases.BIL_FWD_ROUNDINGS.
  epilogue bwd    pre on 2^-2, power-of-two slopes: dpre, dres, dres2 (stored and accumulated), dbias (one block, several, and the
                  1025 partial rows that take the fold's second level) and dprelu -- both accumulated onto lattice presets -- bit for
                  bit.  The derivative at pre == 0 is torch's: the negative side (its backward tests ``> 0``).  ACT_SIGMOID: y on
                  2^-6 {1 .. 63}: d = g y (1 - y) is exact in fp32, so dbias is bit for bit; dpre: 3 roundings + the fp16 store.
  instance norm   red bit for bit on both sides of the 65536-pixel chunk rule; dx (fp32): n = 8 (+ 1 accumulated) roundings of
                  invstd (|g| + |red0 / hw| + |xh red1 / hw|) (+ |dx0|).
  max pool        integers in {-2 .. 2}: ties in nearly every window, H = 1 and W = 1 included: y, and dx (each window's gradient to its
                  first maximum in scan order) bit for bit.
  batch norm      statistics GIVEN: mean on the lattice, invstd a power of two, gamma / beta on the lattice, a power-of-two pixel count:
                  y, red, dgamma / dbeta (accumulated), dprelu and dres bit for bit, one reduce block and several.  dx rounds (xh k2 needs
                  more than 24 bits): n = 7 roundings of |gamma invstd| (|dz| + |k1| + |xh k2|) plus the fp16 store; dy is drawn large
                  enough that no dx lands in fp16's subnormal range, where the store's 2^-11 |ref| model does not hold.
                  bn_finalize: mean and the running mean exact, invstd and the running variance within 2 fp32 ulp of fp64.
  small kernels   power-of-two coefficients on lattice values: bit for bit; the padded lanes of nchw32_to_nhwc16 are +0.

Measured on the MI355X: every bit-for-bit row identical.  Worst error / bound of the bounded rows:
  adaptive pool fwd   c = 8 / 24 / 136:  11x14->3x5 0.82 / 0.82 / 0.83   8x8->3 0.70 / 0.86 / 0.86   17x19->2 (block kernel) 0.77 / 0.88 / 0.90
  adaptive pool bwd   stored | accumulated, worst over c:  11x14->3x5 0.92 | 0.93   8x8->3 0.88 | 0.88   17x19->2 0.94 | 0.96
  bn_backward dx      worst over the 12 configurations:  2x32x8 0.997   2x2048x8 0.998   2x32x40 0.999   2x512x40 0.999
  bn_finalize         invstd 0.50 ulp, running variance 0.50 ulp (of the 2 allowed);  channel_mean_sub 9x9: 0.62 ulp
  bilinear fwd        align 0 / 1:  5x7->20x21 0.64 / 0.91   23x31->50x70 0.84 / 0.86 (c = 256, column kernel: 0.88)   6x6->1x1 0 / 0
  bilinear bwd        worst of stored / accumulated:  5x7->20x21 0.50 / 0.57   23x31->50x70 0.73 / 0.70 (c = 256: 0.83)   6x6->1x1 0 / 0
  bilinear32          fwd 0.093 at most, bwd 0.0085 at most (fp32 outputs: no store term; the position allowance is barely used)
  epilogue sigmoid    dpre 0.93 (the fp16 store);  instnorm_bwd dx 0.23 at most (hw = 65537), 0.15 at hw = 65536
The fp16 rows sit close to 1 because the store alone uses the whole 2^-11 |ref| term at the bottom of a binade (half an fp16 ulp IS
2^-11 of such a value) and thousands of elements are compared; the fp32 part of the bounds is used to less than a quarter
(tests/test_elementwise_cases_cpu.py).  Before the accumulation fix of bcs_fixup_kernel the 96 preset rows of the large border-class path
failed, in class 0 only (the first: got -10.1875, want -76.8125).

Wall time of this module on the MI355X: 7.3 s for its 1550 rows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import elementwise_cases as E
from abi_harness import In16, Out, Out16, _ptr, call, inp, same_bits, twice
from exact_lattice import mismatch

pytestmark = pytest.mark.gpu


def _id(r):
    return "x".join(str(v) for v in r)


def _exact(got, ref, what):
    got, ref = torch.as_tensor(np.ascontiguousarray(got)), torch.as_tensor(np.ascontiguousarray(ref))
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert torch.equal(got.double(), ref.double()), f"{what}: {mismatch(got, ref)}"


def _bounded(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    assert not np.isnan(err).any(), f"{what}: NaN in the result"
    assert (err[bound == 0] == 0).all(), f"{what}: an element with a zero bound is not exact"
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"MEASURED {what}: error / bound {r:.3g}")
    assert r <= 1.0, f"{what}: error {r:.3g} x its bound"


def _in16(x, lay):
    x = np.asarray(x)
    c = x.shape[-1]
    ld, c0 = E.layout(lay, c)
    return In16(x.reshape(-1, c), ld, c0)


def _out16(npix, c, lay, init=None):
    ld, c0 = E.layout(lay, c)
    return Out16(npix, c, ld, c0, None if init is None else np.asarray(init).reshape(npix, c))


# ------------------------------------------------------------------------------------------- border / ring class sums

def run_class_sums(entry, d, row, lay, preset, src="x"):
    N, H, W, c = row
    K = 25 if entry == "csbsr_ring_class_sums" else 16
    x = _in16(d[src], lay)
    sums = Out(N * K * c, init=d["sums0"] if preset else 0.0)
    out = {}
    if entry == "csbsr_border_class_sums_prelu":
        t, nd = _in16(d["t"], lay), Out(N * c, init=d["negdot0"] if preset else 0.0)
        call(entry, x.ptr, x.ld, t.ptr, t.ld, sums.ptr, nd.ptr, N, H, W, c)
        assert nd.margins_intact(), f"{entry} wrote outside negdot"
        out["negdot"] = nd.get(N, c)
    else:
        call(entry, x.ptr, x.ld, sums.ptr, N, H, W, c)
    assert sums.margins_intact(), f"{entry} wrote outside sums"
    out["sums"] = sums.get(N, K, c)
    return out


@pytest.mark.parametrize("preset", [False, True], ids=["zeroed", "preset"])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.BORDER_SHAPES, ids=_id)
def test_border_class_sums(row, lay, preset):
    """a zeroed ``sums`` and one preset with lattice values: the entry point accumulates (include/csbsr_hip.h)"""
    d = E.class_case(*row, ring=False)
    got = twice(lambda: run_class_sums("csbsr_border_class_sums", d, row, lay, preset))
    _exact(got["sums"], E.class_reference("sums", *row, preset), f"border_class_sums ({E.border_path(row[1], row[2])} path) {row} {lay} preset={preset}")


@pytest.mark.parametrize("preset", [False, True], ids=["zeroed", "preset"])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", [s for s in E.BORDER_SHAPES if E.border_path(s[1], s[2]) == "large"], ids=_id)
def test_border_class_sums_prelu(row, lay, preset):
    d = E.class_case(*row, ring=False)
    got = twice(lambda: run_class_sums("csbsr_border_class_sums_prelu", d, row, lay, preset))
    _exact(got["sums"], E.class_reference("sums", *row, preset), f"border_class_sums_prelu sums {row} {lay} preset={preset}")
    _exact(got["negdot"], E.class_reference("negdot", *row, preset), f"border_class_sums_prelu negdot {row} {lay} preset={preset}")


def test_border_class_sums_prelu_refuses_small_maps():
    from csbsr_amd import _lib as L
    row = (2, 31, 33, 8)
    d = E.class_case(*row, ring=False)
    x, t, sums, nd = _in16(d["x"], "whole"), _in16(d["t"], "whole"), Out(2 * 16 * 8, init=0.0), Out(2 * 8, init=0.0)
    with pytest.raises(L.CsbsrHipError, match="1024"):
        call("csbsr_border_class_sums_prelu", x.ptr, x.ld, t.ptr, t.ld, sums.ptr, nd.ptr, *row)
    assert (sums.get() == 0).all() and (nd.get() == 0).all() and sums.margins_intact()


@pytest.mark.parametrize("preset", [False, True], ids=["zeroed", "preset"])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.RING_SHAPES, ids=_id)
def test_ring_class_sums(row, lay, preset):
    d = E.class_case(*row, ring=True)
    got = twice(lambda: run_class_sums("csbsr_ring_class_sums", d, row, lay, preset))
    _exact(got["sums"], E.class_reference("ring", *row, preset), f"ring_class_sums {row} {lay} preset={preset}")


def test_ring_class_sums_refuses_small_maps():
    from csbsr_amd import _lib as L
    x, sums = _in16(np.ones((1, 4, 5, 8)), "whole"), Out(25 * 8, init=0.0)
    with pytest.raises(L.CsbsrHipError, match="ring_class_sums"):
        call("csbsr_ring_class_sums", x.ptr, x.ld, sums.ptr, 1, 4, 5, 8)
    assert (sums.get() == 0).all()


# ------------------------------------------------------------------------------------------- border class fills

def run_fill(entry, d, row, lay, preset=False):
    N, H, W, c = row
    V, out = inp(d["V"]), _out16(N * H * W, c, lay)
    res = {}
    if entry == "csbsr_border_class_fill":
        call(entry, _ptr(V), out.ptr, out.ld, N, H, W, c)
    else:
        m = _in16(d["mask"], lay)
        if entry == "csbsr_border_class_fill_masked":
            call(entry, _ptr(V), out.ptr, out.ld, m.ptr, m.ld, E.MASK_SLOPE, N, H, W, c)
        else:
            sums = Out(N * 16 * c, init=d["sums0"] if preset else 0.0)
            call(entry, _ptr(V), out.ptr, out.ld, m.ptr, m.ld, E.MASK_SLOPE, sums.ptr, N, H, W, c)
            assert sums.margins_intact(), f"{entry} wrote outside sums"
            res["sums"] = sums.get(N, 16, c)
    assert out.intact(), f"{entry} wrote outside its channel slice of out"
    res["out"] = out.get().reshape(N, H, W, c)
    return res


@pytest.mark.parametrize("masked", [0, 1], ids=["plain", "masked"])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.BORDER_SHAPES, ids=_id)
def test_border_class_fill(row, lay, masked):
    d = E.class_case(*row, ring=False)
    got = twice(lambda: run_fill("csbsr_border_class_fill_masked" if masked else "csbsr_border_class_fill", d, row, lay))
    _exact(got["out"], E.class_reference("fill_masked" if masked else "fill", *row), f"border_class_fill masked={masked} {row} {lay}")


@pytest.mark.parametrize("preset", [False, True], ids=["zeroed", "preset"])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.BORDER_SHAPES, ids=_id)
def test_border_class_fill_masked_sums(row, lay, preset):
    """out bit for bit fill_masked's, sums bit for bit border_class_sums of the mask map (both taken from the library, besides the
    references), either side of the 1024-pixel threshold"""
    d = E.class_case(*row, ring=False)
    got = twice(lambda: run_fill("csbsr_border_class_fill_masked_sums", d, row, lay, preset))
    what = f"border_class_fill_masked_sums ({E.border_path(row[1], row[2])} path) {row} {lay} preset={preset}"
    _exact(got["out"], E.class_reference("fill_masked", *row), what + " out")
    _exact(got["sums"], E.class_reference("mask_sums", *row, preset), what + " sums")
    assert same_bits(got["out"], run_fill("csbsr_border_class_fill_masked", d, row, lay)["out"]), what + ": out is not fill_masked's"
    alone = run_class_sums("csbsr_border_class_sums", d, row, lay, preset, src="mask")["sums"]
    assert same_bits(got["sums"], alone), what + ": sums are not border_class_sums'"


# ------------------------------------------------------------------------------------------- weighted pool

def run_wpool_fwd(d, row, lay):
    N, hw, c = row
    x, w, out = _in16(d["x"], lay), inp(d["w"]), Out(N * c, init=0.0)
    call("csbsr_weighted_pool_fwd", x.ptr, x.ld, _ptr(w), out.ptr, N, hw, c)
    assert out.margins_intact(), "csbsr_weighted_pool_fwd wrote outside out"
    return dict(out=out.get(N, c))


def run_wpool_bwd(d, row, lay):
    N, hw, c = row
    x, w, dout = _in16(d["x"], lay), inp(d["w"]), inp(d["dout"])
    dx, dw = _out16(N * hw, c, lay, init=d["dx0"]), Out(N * hw)
    call("csbsr_weighted_pool_bwd", x.ptr, x.ld, _ptr(w), _ptr(dout), dx.ptr, dx.ld, dw.ptr, N, hw, c)
    assert dx.intact() and dw.margins_intact(), "csbsr_weighted_pool_bwd wrote outside dx / dw"
    return dict(dx=dx.get().reshape(N, hw, c), dw=dw.get(N, hw))


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.WPOOL_SHAPES, ids=_id)
def test_weighted_pool(row, lay):
    d = E.wpool_case(*row)
    _exact(twice(lambda: run_wpool_fwd(d, row, lay))["out"], d["out"], f"weighted_pool_fwd {row} {lay}")
    got = twice(lambda: run_wpool_bwd(d, row, lay))
    _exact(got["dw"], d["dw"], f"weighted_pool_bwd dw {row} {lay}")
    _exact(got["dx"], d["dx"], f"weighted_pool_bwd dx {row} {lay}")


# ------------------------------------------------------------------------------------------- adaptive average pool

def run_aap_fwd(d, row, lay):
    N, H, W, OH, OW, c = row
    x, y = _in16(d["x"], lay), Out16(N * OH * OW, c)          # the plain entry point writes a dense y
    call("csbsr_adaptive_avgpool_fwd", x.ptr, x.ld, y.ptr, N, H, W, c, OH, OW)
    assert y.intact(), "csbsr_adaptive_avgpool_fwd wrote outside y"
    return dict(y=y.get().reshape(N, OH, OW, c))


def run_aap_bwd(d, row, lay, accumulate):
    N, H, W, OH, OW, c = row
    dy, dx = In16(d["dy"].reshape(-1, c)), _out16(N * H * W, c, lay, init=d["dx0"] if accumulate else None)
    call("csbsr_adaptive_avgpool_bwd", dy.ptr, dx.ptr, dx.ld, accumulate, N, H, W, c, OH, OW)
    assert dx.intact(), "csbsr_adaptive_avgpool_bwd wrote outside its channel slice of dx"
    return dict(dx=dx.get().reshape(N, H, W, c))


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.AAP_EXACT + E.AAP_RAGGED, ids=_id)
def test_adaptive_avgpool_fwd(row, lay):
    d = E.aap_case(*row)
    got = twice(lambda: run_aap_fwd(d, row, lay))["y"]
    what = f"{E.aap_kernel_for(*row[1:5])} {_id(row)} {lay}"
    if d["exact"]:
        _exact(got, d["y"], what)
    else:
        _bounded(got, d["y"], E.aap_fwd_roundings(d["cnt"])[None, :, :, None] * E.U * d["y_abs"] + E.H16 * np.abs(d["y"]), "aap fwd " + what)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.AAP_EXACT + E.AAP_RAGGED, ids=_id)
def test_adaptive_avgpool_bwd(row, lay, accumulate):
    d = E.aap_case(*row)
    got = twice(lambda: run_aap_bwd(d, row, lay, accumulate))["dx"]
    ref = d["dx"] + d["dx0"] if accumulate else d["dx"]
    what = f"aap_bwd_kernel {_id(row)} {lay} accumulate={accumulate}"
    if d["exact"]:
        _exact(got, ref, what)
    else:
        ab = d["dx_abs"] + (np.abs(d["dx0"]) if accumulate else 0.0)
        _bounded(got, ref, E.AAP_BWD_ROUNDINGS * E.U * ab + E.H16 * np.abs(ref), "aap bwd " + what)


# ------------------------------------------------------------------------------------------- bilinear

def run_bilinear_fwd(d, row, lay, drop):
    N, H, W, OH, OW, al, c = row
    x, y, dr = _in16(d["x"], lay), _out16(N * OH * OW, c, lay), inp(d["drop"]) if drop else None
    call("csbsr_bilinear_fwd", x.ptr, x.ld, y.ptr, y.ld, N, H, W, c, OH, OW, al, _ptr(dr))
    assert y.intact(), "csbsr_bilinear_fwd wrote outside its channel slice of y"
    return dict(y=y.get().reshape(N, OH, OW, c))


def run_bilinear_bwd(d, row, lay, drop, accumulate):
    N, H, W, OH, OW, al, c = row
    dy, dr = _in16(d["dy"], lay), inp(d["drop"]) if drop else None
    dx = _out16(N * H * W, c, lay, init=d["dx0"] if accumulate else None)
    call("csbsr_bilinear_bwd", dy.ptr, dy.ld, dx.ptr, dx.ld, accumulate, N, H, W, c, OH, OW, al, _ptr(dr))
    assert dx.intact(), "csbsr_bilinear_bwd wrote outside its channel slice of dx"
    return dict(dx=dx.get().reshape(N, H, W, c))


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.BIL_EXACT, ids=_id)
def test_bilinear_fwd_exact(row, lay, drop):
    d = E.bilinear_case(*row)
    got = twice(lambda: run_bilinear_fwd(d, row, lay, drop))["y"]
    _exact(got, d["y"] * d["drop"][:, None, None, :] if drop else d["y"], f"{E.bilinear_kernel_for('fwd', *row[:5], row[6])[0]} {row} {lay} drop={drop}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.BIL_EXACT, ids=_id)
def test_bilinear_bwd_exact(row, lay, drop, accumulate):
    d = E.bilinear_case(*row)
    got = twice(lambda: run_bilinear_bwd(d, row, lay, drop, accumulate))["dx"]
    ref = (d["dx"] * d["drop"][:, None, None, :] if drop else d["dx"]) + (d["dx0"] if accumulate else 0.0)
    _exact(got, ref, f"{E.bilinear_kernel_for('bwd', *row[:5], row[6])[-1]} {row} {lay} drop={drop} accumulate={accumulate}")


# ------------------------------------------------------------------------------------------- epilogue backward

def run_epilogue(d, ref, row, lay):
    from csbsr_amd import _lib as L
    npix, c, act, res_mode, dres, dres2 = row
    g, out = _in16(d["g"], lay), _in16(d["out"], lay)
    res = _in16(d["res"], lay) if res_mode else None
    res2 = _in16(d["res2"], lay) if res_mode == E.RES_FMA else None
    prelu = inp(np.array([d["slope"]])) if act == E.ACT_PRELU else None
    dpre = _out16(npix, c, lay)
    o_dres = _out16(npix, c, lay, init=d["dres0"] if dres == 2 else None) if dres else None
    o_dres2 = _out16(npix, c, lay, init=d["dres20"] if dres2 == 2 else None) if dres2 else None
    dbias, dprelu = Out(c, init=d["dbias0"]), Out(1, init=d["dprelu0"]) if act == E.ACT_PRELU else None          # += outputs: lattice presets
    k = L.EpiBwdDesc(npix=npix, c=c, creal=c, dout=g.ptr, dout_ld=g.ld, out=out.ptr, out_ld=out.ld, act=act, act_slope=d["slope"], res_mode=res_mode,
                     dpre=dpre.ptr, dpre_ld=dpre.ld, dbias=dbias.ptr)
    if res:
        k.res, k.res_ld = res.ptr, res.ld
    if res2:
        k.res2, k.res2_ld = res2.ptr, res2.ld
    if prelu is not None:
        k.prelu, k.dprelu = _ptr(prelu), dprelu.ptr
    if o_dres:
        k.dres, k.dres_ld, k.dres_accumulate = o_dres.ptr, o_dres.ld, int(dres == 2)
    if o_dres2:
        k.dres2, k.dres2_ld, k.dres2_accumulate = o_dres2.ptr, o_dres2.ld, int(dres2 == 2)
    call("csbsr_epilogue_backward", C.byref(k))
    r = dict(dpre=dpre.get(), dbias=dbias.get())
    assert dpre.intact() and dbias.margins_intact(), "csbsr_epilogue_backward wrote outside dpre / dbias"
    for name, o in (("dres", o_dres), ("dres2", o_dres2)):
        if o:
            assert o.intact(), f"csbsr_epilogue_backward wrote outside its channel slice of {name}"
            r[name] = o.get()
    if dprelu:
        assert dprelu.margins_intact(), "csbsr_epilogue_backward wrote outside dprelu"
        r["dprelu"] = dprelu.get()
    return r


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("cfg", E.EPI_CONFIGS, ids=_id)
@pytest.mark.parametrize("shape", E.EPI_SHAPES, ids=_id)
def test_epilogue_backward(shape, cfg, lay):
    row = shape + cfg
    d, ref = E.epi_case(*row), E.epi_ref(*row)
    got = twice(lambda: run_epilogue(d, ref, row, lay))
    assert set(got) == set(ref) - {"dpre_abs"}
    for k in got:
        if k == "dpre" and cfg[0] == E.ACT_SIGMOID:
            bound = E.EPI_SIGMOID_ROUNDINGS * E.U * ref["dpre_abs"] + E.H16 * np.abs(ref[k])
            _bounded(got[k], ref[k], bound, f"epilogue_backward sigmoid dpre {_id(row)} {lay}")
            continue
        _exact(got[k], ref[k], f"epilogue_backward {k} npix={shape[0]} c={shape[1]} (act, res_mode, dres, dres2)={cfg} "
                               f"blocks={E.epi_blocks(*shape)[1]} {lay}")


def test_epilogue_backward_two_level_fold():
    """1025 partial rows: dbias through both levels of the fold (the second level reads the scratch tail), onto a preset"""
    row = E.EPI_FOLD2
    d, ref = E.epi_case(*row), E.epi_ref(*row)
    got = twice(lambda: run_epilogue(d, ref, row, "whole"))
    for k in got:
        _exact(got[k], ref[k], f"epilogue_backward {k} {row} blocks={E.epi_blocks(*row[:2])[1]}")


# ------------------------------------------------------------------------------------------- small kernels

@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.AXPBY, ids=_id)
def test_axpby(row, lay):
    npix, c, a, b, z = row
    d = E.small_case("axpby", *row)

    def run():
        x, zz, y = _in16(d["x"], lay), _in16(d["z"], lay) if z else None, _out16(npix, c, lay)
        call("csbsr_axpby", npix, c, x.ptr, x.ld, a, zz.ptr if zz else None, zz.ld if zz else 0, b, y.ptr, y.ld)
        assert y.intact(), "csbsr_axpby wrote outside its channel slice of y"
        return dict(y=y.get())
    _exact(twice(run)["y"], d["ref"], f"axpby {row} {lay}")


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.SUM_ACT, ids=_id)
def test_sum_act(row, lay):
    npix, c, n, relu = row
    d = E.small_case("sum_act", *row)

    def run():
        xs, y = [_in16(x, lay) for x in d["xs"]], _out16(npix, c, lay)
        ptrs, lds = (C.c_void_p * n)(*[x.ptr for x in xs]), (C.c_int64 * n)(*[x.ld for x in xs])
        call("csbsr_sum_act", npix, c, n, ptrs, lds, y.ptr, y.ld, relu)
        assert y.intact(), "csbsr_sum_act wrote outside its channel slice of y"
        return dict(y=y.get())
    _exact(twice(run)["y"], d["ref"], f"sum_act {row} {lay}")


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.FILL, ids=_id)
def test_fill_f16(row, lay):
    npix, c, v = row

    def run():
        p = _out16(npix, c, lay)
        call("csbsr_fill_f16", p.ptr, npix, c, p.ld, v)
        assert p.intact(), "csbsr_fill_f16 wrote outside its channel slice"
        return dict(p=p.get())
    _exact(twice(run)["p"], np.full((npix, c), v), f"fill_f16 {row} {lay}")


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.TO_NCHW, ids=_id)
def test_nhwc16_to_nchw32(row, lay):
    """beta == 0: dst is not read (it holds NaN)"""
    N, Cc, H, W, a, b = row
    d = E.small_case("to_nchw", *row)

    def run():
        src, dst = _in16(d["src"], lay), Out(N * Cc * H * W, init=d["dst0"] if b else float("nan"))
        call("csbsr_nhwc16_to_nchw32", src.ptr, src.ld, dst.ptr, N, Cc, H, W, a, b)
        assert dst.margins_intact(), "csbsr_nhwc16_to_nchw32 wrote outside dst"
        return dict(dst=dst.get(N, Cc, H, W))
    _exact(twice(run)["dst"], d["ref"], f"nhwc16_to_nchw32 {row} {lay}")


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.TO_NHWC, ids=_id)
def test_nchw32_to_nhwc16(row, lay):
    N, Cc, H, W, cp, norm = row
    d = E.small_case("to_nhwc", *row)

    def run():
        src, mean, istd = inp(d["src"]), inp(d["mean"]) if norm else None, inp(d["invstd"]) if norm else None
        dst = _out16(N * H * W, cp, lay)
        call("csbsr_nchw32_to_nhwc16", _ptr(src), dst.ptr, N, Cc, H, W, cp, dst.ld, _ptr(mean), _ptr(istd))
        assert dst.intact(), "csbsr_nchw32_to_nhwc16 wrote outside its channel slice of dst"
        return dict(dst=dst.get().reshape(N, H, W, cp))
    got = twice(run)["dst"]
    _exact(got, d["ref"], f"nchw32_to_nhwc16 {row} {lay}")
    assert (got[..., Cc:].view(np.uint16) == 0).all(), "a padded lane is not +0"


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("row", E.DC_BIAS, ids=_id)
def test_dc_bias(row, bias):
    N, cout, cin, c0, c1 = row
    d = E.small_case("dc_bias", *row)

    def run():
        S, m0, m1, bv, out = inp(d["S"]), inp(d["m0"]), inp(d["m1"]) if c1 else None, inp(d["bias"]) if bias else None, Out(N * cout)
        call("csbsr_dc_bias", _ptr(S), cout, cin, _ptr(m0), d["m0"].shape[1], c0, _ptr(m1), d["m1"].shape[1], c1, _ptr(bv), N, _ptr(out.v))
        assert out.margins_intact(), "csbsr_dc_bias wrote outside out"
        return dict(out=out.get(N, cout))
    _exact(twice(run)["out"], d["ref"] if bias else d["ref_nobias"], f"dc_bias {row} bias={bias}")


# ------------------------------------------------------------------------------------------- batch norm, plain path

def _bn_desc(d, row, lay, backward):
    """(descriptor, outputs, inputs kept alive) of one csbsr_bn_apply / csbsr_bn_backward call"""
    from csbsr_amd import _lib as L
    N, hw, c, act, res, drop, dres = row
    npix = N * hw
    x, mean, istd, ga, be = _in16(d["x"], lay), inp(d["mean"]), inp(d["invstd"]), inp(d["gamma"]), inp(d["beta"])
    keep = [x, mean, istd, ga, be]
    k = L.BnDesc(npix=npix, hw=hw, c=c, creal=c, x=x.ptr, x_ld=x.ld, mean=_ptr(mean), invstd=_ptr(istd), gamma=_ptr(ga), beta=_ptr(be), act=act)
    if res:
        r = _in16(d["res"], lay)
        keep.append(r)
        k.res, k.res_ld = r.ptr, r.ld
    if drop:
        dr = inp(d["drop"])
        keep.append(dr)
        k.drop = _ptr(dr)
    if act == E.ACT_PRELU:
        sl = inp(np.array([E.BN_SLOPE]))
        keep.append(sl)
        k.prelu = _ptr(sl)
    outs = {}
    if not backward:
        outs["y"] = _out16(npix, c, lay)
        k.y, k.y_ld = outs["y"].ptr, outs["y"].ld
        return k, outs, keep
    dy = _in16(d["dy"], lay)
    keep.append(dy)
    outs.update(red=Out(2 * c, init=0.0), dx=_out16(npix, c, lay), dgamma=Out(c, init=d["dgamma0"]), dbeta=Out(c, init=d["dbeta0"]))
    k.dy, k.dy_ld, k.red, k.dx, k.dx_ld = dy.ptr, dy.ld, outs["red"].ptr, outs["dx"].ptr, outs["dx"].ld
    k.dgamma, k.dbeta = outs["dgamma"].ptr, outs["dbeta"].ptr
    if act == E.ACT_PRELU:
        outs["dprelu"] = Out(1, init=0.0)
        k.dprelu = outs["dprelu"].ptr
    if dres:
        outs["dres"] = _out16(npix, c, lay, init=d["dres0"] if dres == 2 else None)
        k.dres, k.dres_ld, k.dres_accumulate = outs["dres"].ptr, outs["dres"].ld, int(dres == 2)
    return k, outs, keep


def run_bn(d, row, lay, backward):
    k, outs, _keep = _bn_desc(d, row, lay, backward)
    call("csbsr_bn_backward" if backward else "csbsr_bn_apply", C.byref(k))
    for name, o in outs.items():
        assert o.intact() if isinstance(o, Out16) else o.margins_intact(), f"batch norm wrote outside {name}"
    return {name: o.get() for name, o in outs.items()}


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("cfg", E.BN_CONFIGS, ids=_id)
@pytest.mark.parametrize("shape", E.BN_SHAPES, ids=_id)
def test_bn_apply(shape, cfg, lay):
    row = shape + cfg
    d = E.bn_case(*row)
    _exact(twice(lambda: run_bn(d, row, lay, False))["y"], d["y"], f"bn_apply {row} {lay}")


@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("cfg", E.BN_CONFIGS, ids=_id)
@pytest.mark.parametrize("shape", E.BN_SHAPES, ids=_id)
def test_bn_backward(shape, cfg, lay):
    """red, dgamma, dbeta (accumulated onto lattice values), dprelu and dres bit for bit; dx bit for bit where the reference is
    fp16-exact, else within BN_DX_ROUNDINGS roundings of its terms plus the fp16 store"""
    row = shape + cfg
    d = E.bn_case(*row)
    got = twice(lambda: run_bn(d, row, lay, True))
    what = f"bn_backward {row} blocks={E.bn_blocks(shape[0] * shape[1], shape[2])} {lay}"
    for k in ("red", "dgamma", "dbeta") + (("dprelu",) if cfg[0] == E.ACT_PRELU else ()) + (("dres",) if cfg[3] else ()):
        _exact(got[k], d[k], what + " " + k)
    if d["dx_exact"]:
        _exact(got["dx"], d["dx"], what + " dx")
    else:
        _bounded(got["dx"], d["dx"], E.BN_DX_ROUNDINGS * E.U * d["dx_abs"] + E.H16 * np.abs(d["dx"]), what + " dx")


@pytest.mark.parametrize("running", [0, 1])
@pytest.mark.parametrize("row", E.BN_FINALIZE, ids=_id)
def test_bn_finalize(row, running):
    c, cstride, count, momentum = row
    d = E.bn_finalize_case(*row)

    def run():
        stat, mean, istd = inp(d["stat"]), Out(c), Out(c)
        rm, rv = (Out(c, init=d["rmean0"]), Out(c, init=d["rvar0"])) if running else (None, None)
        call("csbsr_bn_finalize", _ptr(stat), count, c, cstride, d["eps"], momentum, mean.ptr, istd.ptr, rm.ptr if rm else None, rv.ptr if rv else None)
        assert mean.margins_intact() and istd.margins_intact() and (not rm or (rm.margins_intact() and rv.margins_intact()))
        r = dict(mean=mean.get(), invstd=istd.get())
        if running:
            r.update(rmean=rm.get(), rvar=rv.get())
        return r
    got = twice(run)
    _exact(got["mean"], d["mean"], f"bn_finalize {row} mean")
    for k in ("invstd",) + (("rvar",) if running else ()):
        ulp = np.spacing(np.abs(d[k]).astype(np.float32)).astype(np.float64)
        worst = float((np.abs(got[k].astype(np.float64) - d[k]) / ulp).max())
        print(f"MEASURED bn_finalize {_id(row)} {k}: {worst:.3g} ulp")
        assert worst <= 2.0, f"bn_finalize {row} {k}: {worst:.3g} fp32 ulp from fp64"
    if running:
        _exact(got["rmean"], d["rmean"], f"bn_finalize {row} running mean")


# ------------------------------------------------------------------------------------------- channel_mean_sub

@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.CMEAN, ids=_id)
def test_channel_mean_sub(row, lay):
    """power-of-two sample counts bit for bit (one slice and the partial-row path); 81 samples within 2 fp32 ulp; out is overwritten"""
    N, H, W, cp, step = row
    d = E.cmean_case(*row)

    def run():
        x, out = _in16(d["x"], lay), Out(N * cp)
        call("csbsr_channel_mean_sub", x.ptr, H * W * x.ld, W * x.ld, x.ld, N, H, W, cp, step, out.ptr)
        assert out.margins_intact(), "csbsr_channel_mean_sub wrote outside out"
        return dict(out=out.get(N, cp))
    got = twice(run)["out"]
    if d["exact"]:
        _exact(got, d["ref"], f"channel_mean_sub {row} slices={E.cmean_slices(*row[1:])[1]} {lay}")
    else:
        ulp = np.spacing(np.abs(d["ref"]).astype(np.float32)).astype(np.float64)
        worst = float((np.abs(got.astype(np.float64) - d["ref"]) / ulp).max())
        print(f"MEASURED channel_mean_sub {_id(row)} {lay}: {worst:.3g} ulp")
        assert worst <= 2.0, f"channel_mean_sub {row}: {worst:.3g} fp32 ulp from fp64"



# ------------------------------------------------------------------------------------------- bilinear, ratios that round

@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.BIL_BOUNDED, ids=_id)
def test_bilinear_fwd_bounded(row, lay, drop):
    N, H, W, OH, OW, al, c = row
    d = E.bilinear_bounded_case(*row)
    got = twice(lambda: run_bilinear_fwd(d, row, lay, drop))["y"]
    ref, b32 = E.bilinear_bounds(d, "fwd", drop, 0, H, W)
    _bounded(got, ref, b32 + E.H16 * np.abs(ref), f"bilinear fwd {E.bilinear_kernel_for('fwd', *row[:5], c)[0]} {_id(row)} {lay} drop={drop}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.BIL_BOUNDED, ids=_id)
def test_bilinear_bwd_bounded(row, lay, drop, accumulate):
    N, H, W, OH, OW, al, c = row
    d = E.bilinear_bounded_case(*row)
    got = twice(lambda: run_bilinear_bwd(d, row, lay, drop, accumulate))["dx"]
    ref, b32 = E.bilinear_bounds(d, "bwd", drop, accumulate, H, W)
    kernel = E.bilinear_kernel_for("bwd", *row[:5], c)[-1]
    _bounded(got, ref, b32 + E.H16 * np.abs(ref), f"bilinear bwd {kernel} {_id(row)} {lay} drop={drop} accumulate={accumulate}")


# ------------------------------------------------------------------------------------------- bilinear32 (csrc/image_ops.hip)

def run_bilinear32(d, row, backward):
    planes, H, W, OH, OW, al = row
    if backward:
        src, out = inp(d["dy"]), Out(planes * H * W)
        call("csbsr_bilinear32_bwd", _ptr(src), out.ptr, planes, H, W, OH, OW, al)
    else:
        src, out = inp(d["x"]), Out(planes * OH * OW)
        call("csbsr_bilinear32_fwd", _ptr(src), out.ptr, planes, H, W, OH, OW, al)
    assert out.margins_intact(), "csbsr_bilinear32 wrote outside its output"
    return dict(out=out.get(planes, H, W) if backward else out.get(planes, OH, OW))


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("row", E.BIL32_EXACT + E.BIL32_BOUNDED, ids=_id)
def test_bilinear32(row, backward):
    d = E.bilinear32_case(*row)
    got = twice(lambda: run_bilinear32(d, row, backward))["out"]
    ref = d["dx"] if backward else d["y"]
    if d["exact"]:
        _exact(got, ref, f"bilinear32 {'bwd' if backward else 'fwd'} {row}")
    else:
        _bounded(got, ref, d["dx_bound"] if backward else d["y_bound"], f"bilinear32 {'bwd' if backward else 'fwd'} {_id(row)}")


# ------------------------------------------------------------------------------------------- max pool, plain entry points

@pytest.mark.parametrize("row", E.MAXPOOL, ids=_id)
def test_maxpool_plain(row):
    """dense maps through the plain wrappers; ties everywhere; the gradient of a window goes to its first maximum in scan order"""
    N, H, W, c = row
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = E.maxpool_case(*row)

    def run():
        x, y = In16(d["x"].reshape(-1, c)), Out16(N * OH * OW, c)
        call("csbsr_maxpool3x3s2_fwd", x.ptr, y.ptr, N, H, W, c)
        assert y.intact(), "csbsr_maxpool3x3s2_fwd wrote outside y"
        ys, dy, dx = In16(d["y"].reshape(-1, c)), In16(d["dy"].reshape(-1, c)), Out16(N * H * W, c)
        call("csbsr_maxpool3x3s2_bwd", x.ptr, ys.ptr, dy.ptr, dx.ptr, N, H, W, c)
        assert dx.intact(), "csbsr_maxpool3x3s2_bwd wrote outside dx"
        return dict(y=y.get().reshape(N, OH, OW, c), dx=dx.get().reshape(N, H, W, c))
    got = twice(run)
    _exact(got["y"], d["y"], f"maxpool fwd {row}")
    _exact(got["dx"], d["dx"], f"maxpool bwd {row}")


# ------------------------------------------------------------------------------------------- instance-norm backward

@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("lay", E.LAYOUTS)
@pytest.mark.parametrize("row", E.INSTNORM, ids=_id)
def test_instnorm_bwd(row, lay, accumulate):
    """red bit for bit (one partial row per plane and two); dx within INSTNORM_ROUNDINGS roundings of its terms"""
    N, Cc, hw = row
    d = E.instnorm_case(*row)

    def run():
        dy, x, mean, istd = _in16(d["dy8"], lay), inp(d["x"]), inp(d["mean"]), inp(d["invstd"])
        dx, red = Out(N * Cc * hw, init=d["dx0"] if accumulate else None), Out(N * Cc * 2, init=0.0)
        call("csbsr_instnorm_bwd", dy.ptr, dy.ld, _ptr(x), _ptr(mean), _ptr(istd), dx.ptr, accumulate, N, Cc, hw, red.ptr)
        assert dx.margins_intact() and red.margins_intact(), "csbsr_instnorm_bwd wrote outside dx / red"
        return dict(dx=dx.get(N, Cc, hw), red=red.get(N, Cc, 2))
    got = twice(run)
    what = f"instnorm_bwd {_id(row)} {lay} accumulate={accumulate}"
    _exact(got["red"], d["red"], what + " red")
    _bounded(got["dx"], d["dx"] + (d["dx0"] if accumulate else 0.0), E.instnorm_bound(d, accumulate), what + " dx")
