"""Exact / bounded parity of the per-sample blur and the bicubic resizes of csrc/image_ops.hip -- csbsr_blur_fwd, csbsr_blur_bwd_input,
csbsr_blur_bwd_kernel (seven kernels), csbsr_aa_bicubic_down_fwd / _bwd and csbsr_bicubic_up_add (five kernels) -- through the C ABI,
at the smallest shapes that cross each tile seam, dispatch threshold and grid wrap.  References, input builders, case tables and the
mutants that show the inputs discriminate: tests/image_cases.py (validated without a GPU by tests/test_image_cases_cpu.py).  The
guarded call harness is tests/abi_harness.py: NaN-refilled reduction scratch, NaN margins round every input, sentinel margins round
every output, every row twice with identical bits.

What is exact, what carries a bound, and why:

  blur            operands are integers x 2^-8 (|x| <= 255 units, |k| <= 64, K^2 x 255 x 64 < 2^24 units), so a sum of products in any
                  order is exact in fp32: y32, y32 - sub, dx (stored and accumulated onto a lattice dx0) and dk (integers |dy|, |x| <= 3
                  over up to 1 035 450 pixels, both levels of the fold) are asked BIT FOR BIT on every row.  The fp16 NHWC output:
                  x in {-1, 0, 1}, k in {-4 .. 4}, every value an integer below 2048, asked bit for bit; lanes 3 .. 7 of every pixel
                  keep their sentinel.
  down, aa = 0    f in {2, 4, 8}: weights exactly {-3, 19, 19, -3} / 32, x on 2^-4 {-15 .. 15}: forward, backward and the accumulating
                  backward bit for bit.
  up_add          s = 2 (integers in {-15 .. 15}) and s = 4 (ternary x, out0 in {-2 .. 2}): bit for bit.  s = 8: per element
                  |got - ref| <= 17 x 2^-24 (|M_y| |x| |M_x|^T + |out0|): a 4-term dot product per axis is 4 products + 4 additions, the
                  weights are exact multiples of 2^-14, one more rounding for the add into out.
  down, aa = 1    per element |got - ref| <= n 2^-24 |M_y| |x| |M_x|^T with n = image_cases.aa_roundings(f, border): per axis at most
                  4 f + 1 additions and as many products (2 (4 f + 1)); in the interior (outputs 2 .. n / f - 3, and the inputs only
                  they touch) that is all, because the fp32 weights equal the fp64 ones bit for bit: n = 36 / 68 / 132 for f = 2 / 4 / 8.
                  A weight of a cut tap set adds 4 f + 9 per axis (its normalising sum, the reciprocal, the product, the cubic):
                  n = 70 / 118 / 214.  One more for the accumulating backward.  The per-pixel backward (no scratch registered) is held
                  to the same bound.

Measured on the MI355X: every bit-for-bit row identical.  Worst error / bound of the bounded rows, interior | border ("-": the row has
no interior; planes x H x W x f):
  down fwd            6x32x40x4 0.024 | 0.020   3x12x20x2 0.035 | 0.028   3x48x24x8 - | 0.0021   2x8x4x4 - | 0.0021   1x2x2x2 - | 0.0065
                      3x1024x768x4 0.036 | 0.017   1x24x28x2 0.036 | 0.017   1x80x88x8 0.0037 | 0.0037
  down bwd (tables)   stored / accumulated:  6x32x40x4 0.038 | 0.030 / 0.014 | 0.019   3x12x20x2 - | 0.044 / - | 0.021
                      3x48x24x8 - | 0.015 / - | 0.0078   2x8x4x4 - | 0.014 / - | 0.0073   1x2x2x2 - | 0 / - | 0.0066
                      3x1024x768x4 0.060 | 0.035 / 0.043 | 0.024   1x24x28x2 0.050 | 0.035 / 0.028 | 0.028   1x80x88x8 0.025 | 0.017 / 0.016 | 0.0084
  down bwd per-pixel  6x32x40x4 0.042 | 0.033 / 0.022 | 0.024   2x8x4x4 - | 0.015 / - | 0.0074  (not the tables' bits: the other kernel ran)
  up_add s = 8        2x5x6x8 0.16
The counted bounds are 16 to 50 times what the kernels need (an honest fp32 evaluation sits near 2 .. 4 x 2^-24 of |M_y| |x| |M_x|^T);
every mutant of tests/image_cases.py is more than 10 bounds away (tests/test_image_cases_cpu.py).

Wall time of this module on the MI355X: 1.9 s for its 125 rows.
"""
import numpy as np
import pytest
import torch

import image_cases as I
from abi_harness import SENT, Out, _dev, _ptr, call, inp, twice
from exact_lattice import mismatch

pytestmark = pytest.mark.gpu


def _id(r):
    return "x".join(str(v) for v in r)


def _exact(got, ref, what):
    got, ref = torch.as_tensor(got), torch.as_tensor(np.array(ref) if isinstance(ref, np.ndarray) else ref)
    assert got.shape == ref.shape and torch.equal(got.double(), ref.double()), f"{what}: {mismatch(got, ref)}"


# ------------------------------------------------------------------------------------------- blur forward

def run_blur_fwd(case, row, want32, want16, with_sub):
    N, C, H, W, K, s = row
    OH, OW = I.out_size(H, K, s), I.out_size(W, K, s)
    x, k, sub = inp(case["x"]), inp(case["k"]), inp(case["sub"]) if with_sub else None
    y32 = Out(N * C * OH * OW) if want32 else None
    y16 = Out(N * OH * OW * I.Y16_LD, torch.float16) if want16 else None
    call("csbsr_blur_fwd", _ptr(x), _ptr(k), N, C, H, W, K, s, _ptr(sub), y32.ptr if y32 else None, y16.ptr if y16 else None, I.Y16_LD)
    out = {}
    if y32:
        assert y32.margins_intact(), "csbsr_blur_fwd wrote outside y32"
        out["y32"] = y32.get(N, C, OH, OW)
    if y16:
        assert y16.margins_intact(), "csbsr_blur_fwd wrote outside y16"
        out["y16"] = y16.get(N, OH, OW, I.Y16_LD)
    return out


@pytest.mark.parametrize("variant", I.FWD_VARIANTS)
@pytest.mark.parametrize("row", I.BLUR_FWD, ids=_id)
def test_blur_fwd_exact(row, variant):
    """y32 / y32 - sub on the rich lattice; the fp16 NHWC output alone and together with y32 (and sub) on the fp16 lattice"""
    N, C, H, W, K, s = row
    c, h, ref = I.blur_fwd_reference(*row)
    kernel = I.blur_kernel_for("fwd", K, s, H, W, C)[0]
    case = h if variant in ("y16", "both") else c
    got = twice(lambda: run_blur_fwd(case, row, variant != "y16", variant in ("y16", "both"), variant in ("y32_sub", "both")))
    if "y32" in got:
        _exact(got["y32"], ref[variant], f"{kernel} {row} {variant} y32")
    if "y16" in got:
        y16 = torch.from_numpy(got["y16"])
        _exact(y16[..., :C].permute(0, 3, 1, 2), ref[variant], f"{kernel} {row} {variant} y16")
        assert bool((y16[..., C:] == SENT).all()), f"{kernel} {row}: a padding lane of a y16 pixel was written"


# ------------------------------------------------------------------------------------------- blur input gradient

def run_blur_dx(case, row, accumulate):
    N, C, H, W, K, s = row
    dy, k = inp(case["dy"]), inp(case["k"])
    dx = Out(N * C * H * W, init=case["dx0"] if accumulate else None)
    call("csbsr_blur_bwd_input", _ptr(dy), _ptr(k), dx.ptr, accumulate, N, C, H, W, K, s)
    assert dx.margins_intact(), "csbsr_blur_bwd_input wrote outside dx"
    return dict(dx=dx.get(N, C, H, W))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("row", I.BLUR_BWD_INPUT, ids=_id)
def test_blur_bwd_input_exact(row, accumulate):
    N, C, H, W, K, s = row
    c, dx = I.blur_dx_reference(*row)
    kernel = I.blur_kernel_for("bwd_input", K, s, H, W, C)[0]
    got = twice(lambda: run_blur_dx(c, row, accumulate))
    _exact(got["dx"], dx + c["dx0"].double() if accumulate else dx, f"{kernel} {row} accumulate={accumulate}")


# ------------------------------------------------------------------------------------------- blur kernel gradient

def run_blur_dk(case, row):
    N, C, H, W, K, s = row
    dy, x = inp(case["dy"]), inp(case["x"])
    dk = Out(N * K * K, init=0.0)
    call("csbsr_blur_bwd_kernel", _ptr(dy), _ptr(x), dk.ptr, N, C, H, W, K, s)
    assert dk.margins_intact(), "csbsr_blur_bwd_kernel wrote outside dk"
    return dict(dk=dk.get(N, K, K))


@pytest.mark.parametrize("row", I.BLUR_BWD_KERNEL, ids=_id)
def test_blur_bwd_kernel_exact(row):
    N, C, H, W, K, s = row
    c, dk = I.blur_dk_reference(*row)
    kernel, tpw = I.blur_kernel_for("bwd_kernel", K, s, H, W, C)
    got = twice(lambda: run_blur_dk(c, row))
    _exact(got["dk"], dk, f"{kernel} {row} tiles_per_wg={tpw}")


# ------------------------------------------------------------------------------------------- blur refusals

def _refusal_calls(K, null):
    """(name, args, outputs, inputs kept alive) of one call per blur entry point at kernel size K; ``null``: the first pointer is missing"""
    N, C, H, W = 1, 3, 8, 8
    a, b, kv = inp(np.ones(N * C * H * W)), inp(np.ones(N * C * H * W)), inp(np.ones(N * K * K))
    first = None if null else _ptr(a)
    y32, y16, dx, dk = Out(N * C * H * W), Out(N * H * W * I.Y16_LD, torch.float16), Out(N * C * H * W), Out(N * K * K)
    keep = (a, b, kv)
    return [("csbsr_blur_fwd", (first, _ptr(kv), N, C, H, W, K, 1, None, y32.ptr, y16.ptr, I.Y16_LD), [y32, y16], keep),
            ("csbsr_blur_bwd_input", (first, _ptr(kv), dx.ptr, 0, N, C, H, W, K, 1), [dx], keep),
            ("csbsr_blur_bwd_kernel", (first, _ptr(b), dk.ptr, N, C, H, W, K, 1), [dk], keep)]


def test_blur_refuses_other_kernel_sizes():
    from csbsr_amd import _lib as L
    for name, args, outs, _keep in _refusal_calls(I.REFUSED_K, null=False):
        with pytest.raises(L.CsbsrHipError, match="unsupported kernel size 9"):
            call(name, *args)
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs), f"{name}: the refused call wrote to an output"


def test_blur_refuses_null():
    from csbsr_amd import _lib as L
    calls = _refusal_calls(21, null=True)
    N, C, H, W = 1, 3, 8, 8
    x, kv = inp(np.ones(N * C * H * W)), inp(np.ones(N * 441))
    calls.append(("csbsr_blur_fwd", (_ptr(x), _ptr(kv), N, C, H, W, 21, 1, None, None, None, 0), [], (x, kv)))          # neither output
    for name, args, outs, _keep in calls:
        with pytest.raises(L.CsbsrHipError, match="null"):
            call(name, *args)
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs), f"{name}: the refused call wrote to an output"


# ------------------------------------------------------------------------------------------- bicubic down-scale

def _ratio(got, ref, bound):
    """worst |got - ref| / bound; where the bound is 0 the result has to be exact"""
    err = np.abs(got.astype(np.float64) - ref)
    assert not np.isnan(err).any(), "NaN in the result"
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _check_bounded(got, ref, ab, My, Mx, f, adjoint, accumulate, what):
    """interior and border separately, each against its own count of roundings"""
    inner = I.interior_mask(My, adjoint)[:, None] & I.interior_mask(Mx, adjoint)[None, :]
    n_in, n_bd = I.aa_roundings(f, False, accumulate) * I.U, I.aa_roundings(f, True, accumulate) * I.U
    r_in = _ratio(got[:, inner], ref[:, inner], n_in * ab[:, inner]) if inner.any() else float("nan")
    r_bd = _ratio(got[:, ~inner], ref[:, ~inner], n_bd * ab[:, ~inner])
    print(f"MEASURED {what}: error / bound  interior {'none' if not inner.any() else format(r_in, '.3g')} (n = {n_in / I.U:.0f})  "
          f"border {r_bd:.3g} (n = {n_bd / I.U:.0f})")
    assert not (r_in > 1.0), f"{what}: interior error {r_in:.3g} x its bound"
    assert r_bd <= 1.0, f"{what}: border error {r_bd:.3g} x its bound"


def run_down_fwd(d, row, aa):
    planes, H, W, f = row
    x, y = inp(d["x"]), Out(planes * (H // f) * (W // f))
    call("csbsr_aa_bicubic_down_fwd", _ptr(x), y.ptr, planes, H, W, f, aa)
    assert y.margins_intact(), "csbsr_aa_bicubic_down_fwd wrote outside y"
    return dict(y=y.get(planes, H // f, W // f))


def run_down_bwd(d, row, aa, accumulate):
    planes, H, W, f = row
    dy, dx = inp(d["dy"]), Out(planes * H * W, init=d["dx0"] if accumulate else None)
    call("csbsr_aa_bicubic_down_bwd", _ptr(dy), dx.ptr, accumulate, planes, H, W, f, aa)
    assert dx.margins_intact(), "csbsr_aa_bicubic_down_bwd wrote outside dx"
    return dict(dx=dx.get(planes, H, W))


@pytest.mark.parametrize("aa", [1, 0])
@pytest.mark.parametrize("row", I.DOWN_CASES, ids=_id)
def test_bicubic_down_fwd(row, aa):
    planes, H, W, f = row
    d = I.down_case(planes, H, W, f, aa)
    got = twice(lambda: run_down_fwd(d, row, aa))["y"]
    if d["exact"]:
        _exact(got, d["y"], f"aa_down_fwd_kernel {row} aa=0")
    else:
        _check_bounded(got, d["y"], d["y_abs"], d["My"], d["Mx"], f, False, 0, f"down fwd {_id(row)}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("aa", [1, 0])
@pytest.mark.parametrize("row", I.DOWN_CASES, ids=_id)
def test_bicubic_down_bwd(row, aa, accumulate):
    """aa = 1: the table kernels (aa_weight_tables_kernel + aa_down_bwd_tab_kernel); aa = 0: the per-pixel kernel's clamped-tap rule"""
    planes, H, W, f = row
    d = I.down_case(planes, H, W, f, aa)
    got = twice(lambda: run_down_bwd(d, row, aa, accumulate))["dx"]
    ref = d["dx"] + d["dx0"].astype(np.float64) if accumulate else d["dx"]
    if d["exact"]:
        _exact(got, ref, f"aa_down_bwd_kernel {row} aa=0 accumulate={accumulate}")
    else:
        ab = d["dx_abs"] + (np.abs(d["dx0"].astype(np.float64)) if accumulate else 0.0)
        _check_bounded(got, ref, ab, d["My"], d["Mx"], f, True, accumulate, f"down bwd {_id(row)} accumulate={accumulate}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("row", I.FALLBACK_CASES, ids=_id)
def test_aa_down_bwd_without_scratch(row, accumulate):
    """no reduction scratch registered: csbsr_aa_bicubic_down_bwd has no room for its weight tables and takes the per-pixel antialiased
    kernel (aa_down_bwd_kernel with antialias = 1); the same bound"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import _reduction_scratch
    planes, H, W, f = row
    d = I.down_case(planes, H, W, f, 1)
    buf = _reduction_scratch(_dev())
    try:
        L.call("csbsr_set_reduction_scratch", None, 0)
        got = twice(lambda: run_down_bwd(d, row, 1, accumulate))["dx"]
    finally:
        L.call("csbsr_set_reduction_scratch", _ptr(buf), buf.numel())
    ref = d["dx"] + d["dx0"].astype(np.float64) if accumulate else d["dx"]
    ab = d["dx_abs"] + (np.abs(d["dx0"].astype(np.float64)) if accumulate else 0.0)
    _check_bounded(got, ref, ab, d["My"], d["Mx"], f, True, accumulate, f"down bwd per-pixel {_id(row)} accumulate={accumulate}")
    again = run_down_bwd(d, row, 1, accumulate)["dx"]          # the scratch is back: the table path runs, within the same bound
    _check_bounded(again, ref, ab, d["My"], d["Mx"], f, True, accumulate, f"down bwd after re-registering {_id(row)}")


# ------------------------------------------------------------------------------------------- bicubic up-scale

def run_up_add(d, row):
    planes, H, W, s = row
    x, out = inp(d["x"]), Out(planes * H * s * W * s, init=d["out0"])
    call("csbsr_bicubic_up_add", _ptr(x), out.ptr, planes, H, W, s)
    assert out.margins_intact(), "csbsr_bicubic_up_add wrote outside out"
    return dict(out=out.get(planes, H * s, W * s))


@pytest.mark.parametrize("row", I.UP_CASES, ids=_id)
def test_bicubic_up_add(row):
    d = I.up_case(*row)
    got = twice(lambda: run_up_add(d, row))["out"]
    if d["exact"]:
        _exact(got, d["out"], f"bicubic_up_add_kernel {row}")
    else:
        r = _ratio(got, d["out"], I.UP8_ROUNDINGS * I.U * d["out_abs"])
        print(f"MEASURED up_add {_id(row)}: error / bound {r:.3g} (n = {I.UP8_ROUNDINGS})")
        assert r <= 1.0
