"""Exact / fp64 parity of the kernels behind the numbers this project reports -- all of csrc/data_ops.hip (csbsr_iou_sweep,
csbsr_psnr_ssim, csbsr_gaussian_kernels) -- and of the loss reductions that share its 65536-element chunk rule (csbsr_l1_fwd_bwd,
csbsr_plane_reduce, csbsr_segloss_reduce / _finish), through the C ABI, at the smallest shapes that cross each tiling, chunking and
folding boundary.  References and input builders: tests/metric_cases.py (validated without a GPU by tests/test_metric_cases_cpu.py).

Every row: the shared reduction scratch is refilled with NaN before the call (a fold that reads a slot nobody wrote turns the result
into NaN); every input sits inside a NaN-filled allocation (a read outside the slice poisons the result instead of faulting); every
output sits inside a sentinel-filled allocation whose two margins are checked afterwards; the call runs twice and the two results
must be bit-identical.

What is exact, what carries a tolerance, and why:

  IoU sweep     ``inter`` / ``union`` and the histogram total are integers: equality with the count of (pred - t > 0) in fp32, ties,
                fp32 neighbours of every threshold, +-inf and NaN included.  ``iou``: 1 fp32 ulp of (inter + 1e-5) / (union + 1e-5)
                in fp64 -- the kernel adds fp32(1e-5) (2.7e-9 relative away from 1e-5, tests/test_metric_cases_cpu.py) in fp64 and
                rounds once.  Measured: at most 0.5 ulp on every row (the correctly rounded value).
  PSNR          inputs on the 2^-8 lattice with |a - b| <= 7 * 2^-8: the sum of squared errors is exact in fp32 in any order, so
                sums[n][0] is asked bit for bit; the PSNR itself within 1e-4 dB of fp64 (the project's tolerance; fp32 division and
                log10f on an exact sum).  Measured: at most 3.4e-6 dB.  a == b gives +inf as in the reference.
  SSIM          1e-5 of the fp64 restatement (the project's tolerance) on noise pairs and smooth pairs; a plain fp32 evaluation of the
                same formulas stays within 1.6e-7 of fp64 on these inputs (asserted < 1e-6 on the CPU), so the bound is about the
                kernel.  Measured on the MI355X, noise / smooth:  2x1x1x1 4.4e-8 / 1.4e-7,  2x3x5x5 6.2e-8 / 1.4e-8,
                4x1x21x21 5.7e-8 / 5.4e-8,  2x3x8x32 3.9e-8 / 7.9e-8,  2x3x9x33 1.4e-7 / 1.6e-8,  1x2x40x52 8.0e-8 / 3.9e-8,
                2x3x93x925 (the two-level fold) 9.7e-8 / 3.0e-8; the PSNR of the same calls within 4.4e-6 dB.
  blur kernels  every element within max(1 fp32 ulp, 2^-126) of the fp64 restatement: the kernel evaluates in fp64 (error ~1e-15
                relative, far below half an ulp) and rounds once; the floor admits a subnormal flushed on conversion.  Each kernel's
                fp64 sum within 1e-6 of 1.  Measured: at most 0.5 ulp, sums within 3.3e-8.
  L1            a - b on 2^-8 {-15 .. 15}, wmap on 2^-2 {2 .. 6}, power-of-two gradient scales: sums and gradients bit for bit,
                stored and accumulated, with and without wmap, at C * hw = 66789 (two chunks, the boundary inside plane 1).
  plane sums    values on 2^-8 {0 .. 12} at hw = 66065 (two chunks): sum a, sum a^2 and sum a b bit for bit.
  seg. loss     N = 2, hw = 66065 against the oracle's boundary_combo_loss on fp64 inputs: loss 1e-5, gradient 1e-4, relative to
                the maximum (the tolerances of test_segloss_and_l1), with p == 0 pixels on both sides of the chunk boundary and an
                empty target; sum t^2 (column 3 of the sums) is an integer and asked exactly.  Measured: loss 2.1e-8, gradient 8.6e-8.

Wall time of this module on the MI355X: about 3 s for its 43 rows (5.7 s together with tests/test_aux_rows_gpu.py).
"""
import numpy as np
import pytest
import torch

import metric_cases as M
from abi_harness import Out, _ptr, call, inp, same_bits, twice

pytestmark = pytest.mark.gpu

THRESHOLDS = [i * 0.01 for i in range(1, 100)]


# ------------------------------------------------------------------------------------------- IoU sweep

def run_iou(pred, mask, th, smooth=1e-5):
    B, hw = pred.shape
    T = len(th)
    p, m, t = inp(pred), inp(mask), inp(th)
    hist = Out(B * 2 * (T + 1), torch.int32, init=0)
    iou, inter, uni = Out(B * T), Out(B * T), Out(B * T)
    call("csbsr_iou_sweep", _ptr(p), _ptr(m), _ptr(t), B, hw, T, float(smooth), hist.ptr, iou.ptr, inter.ptr, uni.ptr)
    for o in (hist, iou, inter, uni):
        assert o.margins_intact(), "csbsr_iou_sweep wrote outside an output"
    return dict(hist=hist.get(B, 2 * (T + 1)), iou=iou.get(B, T), inter=inter.get(B, T), union=uni.get(B, T))


def check_iou(pred, mask, th):
    B, hw = pred.shape
    got = twice(lambda: run_iou(pred, mask, th))
    ri, ru = M.ref_iou_counts(pred, mask, th)
    assert np.array_equal(got["hist"].astype(np.int64).sum(1), np.full(B, hw)), "a sample's histogram does not hold hw pixels"
    bad = np.argwhere(got["inter"].astype(np.int64) != ri)
    assert bad.size == 0, f"inter differs at (sample, threshold) {bad[:4].tolist()}: {got['inter'][tuple(bad[0])]} vs {ri[tuple(bad[0])]}"
    bad = np.argwhere(got["union"].astype(np.int64) != ru)
    assert bad.size == 0, f"union differs at (sample, threshold) {bad[:4].tolist()}: {got['union'][tuple(bad[0])]} vs {ru[tuple(bad[0])]}"
    ref = M.ref_iou(ri, ru)
    err = np.abs(got["iou"].astype(np.float64) - ref) / M.ulp32(ref)
    print(f"iou B={B} hw={hw} T={len(th)}: {err.max():.3g} ulp")
    assert err.max() <= 1.0
    return got, ref


@pytest.mark.parametrize("B,hw", M.IOU_SHAPES)
def test_iou_counts_exact(B, hw):
    th = M.thresholds32(THRESHOLDS)
    pred, mask = M.iou_tie_inputs(B, hw, th, seed=hw + 99)
    check_iou(pred, mask, th)


@pytest.mark.parametrize("B,hw,T", M.IOU_EXTRA_T)
def test_iou_threshold_counts(B, hw, T):
    """T = 1 (the IoU class), T = 2, and T = 1024 -- the largest accepted: 2 * 1025 + 1024 words of LDS"""
    th = M.many_thresholds(T)
    pred, mask = M.iou_tie_inputs(B, hw, th, seed=hw + T)
    check_iou(pred, mask, th)


def test_iou_all_background_sample():
    """no foreground and nothing above the lowest threshold (ties with it included): 0 / 0 pixels, iou == 1 at every threshold"""
    th = M.thresholds32(THRESHOLDS)
    pred, mask = M.iou_tie_inputs(2, 65537, th, seed=5, background_sample=1)
    got, ref = check_iou(pred, mask, th)
    assert (got["iou"][1] == 1.0).all() and (got["inter"][1] == 0).all() and (got["union"][1] == 0).all()
    assert (got["union"][0] > 0).all()


def test_iou_refuses_1025_thresholds():
    from csbsr_amd import _lib as L
    th = M.many_thresholds(1025)
    pred, mask = M.iou_tie_inputs(1, 257, th[:99], seed=1)
    p, m, t = inp(pred), inp(mask), inp(th)
    outs = [Out(2 * 1026, torch.int32), Out(1025), Out(1025), Out(1025)]
    with pytest.raises(L.CsbsrHipError, match="iou_sweep"):
        call("csbsr_iou_sweep", _ptr(p), _ptr(m), _ptr(t), 1, 257, 1025, 1e-5, *(o.ptr for o in outs))
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), "the refused call wrote to an output"


# ------------------------------------------------------------------------------------------- PSNR / SSIM

def run_psnr_ssim(a, b):
    N, Cc, H, W = a.shape
    da, db = inp(a), inp(b)
    sums, ps, ss = Out(N * 2, init=0.0), Out(N), Out(N)
    call("csbsr_psnr_ssim", _ptr(da), _ptr(db), N, Cc, H, W, sums.ptr, ps.ptr, ss.ptr)
    for o in (sums, ps, ss):
        assert o.margins_intact(), "csbsr_psnr_ssim wrote outside an output"
    return dict(sums=sums.get(N, 2), psnr=ps.get(), ssim=ss.get())


@pytest.mark.parametrize("N,C,H,W", M.IMG_SHAPES)
def test_psnr_exact(N, C, H, W):
    eq = N - 1 if N > 1 else None
    a, b, sum_sq = M.psnr_lattice(N, C, H, W, seed=H * W, equal_sample=eq)
    got = twice(lambda: run_psnr_ssim(a, b))
    want = (sum_sq / 65536.0).astype(np.float32)
    assert np.array_equal(got["sums"][:, 0], want), f"sum of squared errors: got {got['sums'][:, 0].tolist()}, want {want.tolist()}"
    ref = M.psnr_from_sum_sq(sum_sq, C * H * W)
    live = np.isfinite(ref)
    assert np.array_equal(got["psnr"][~live].astype(np.float64), ref[~live]), "a == b must give +inf"
    if eq is not None:
        assert np.isposinf(got["psnr"][eq])
    if live.any():
        dev = np.abs(got["psnr"][live] - ref[live]).max()
        print(f"psnr {N}x{C}x{H}x{W}: {dev:.3g} dB")
        assert dev < 1e-4


@pytest.mark.parametrize("family", ["noise", "smooth"])
@pytest.mark.parametrize("N,C,H,W", M.IMG_SHAPES)
def test_ssim_fp64(N, C, H, W, family):
    a, b = M.ssim_pair(family, N, C, H, W, seed=H + W)
    got = twice(lambda: run_psnr_ssim(a, b))
    psnr, ssim = M.ref_psnr_ssim(a, b)
    dev = np.abs(got["ssim"] - ssim).max()
    print(f"ssim {family} {N}x{C}x{H}x{W}: {dev:.3g}   psnr {np.abs(got['psnr'] - psnr).max():.3g} dB")
    assert dev < 1e-5
    assert np.abs(got["psnr"] - psnr).max() < 1e-4


# ------------------------------------------------------------------------------------------- Gaussian blur kernels

def run_gauss(params, K):
    N = len(params)
    p = inp(params)
    out = Out(N * K * K)
    call("csbsr_gaussian_kernels", _ptr(p), out.ptr, N, K)
    assert out.margins_intact(), "csbsr_gaussian_kernels wrote outside its output"
    return dict(k=out.get(N, K, K))


@pytest.mark.parametrize("K", M.GAUSS_K)
def test_gaussian_kernels(K):
    from csbsr_amd.data.degrade import DeviceDegradation
    draws = DeviceDegradation(scale=4, ksize=K, seed=11).draw_params(32).numpy().astype(np.float32)
    params = np.concatenate([M.GAUSS_CORNERS, draws])
    assert len(params) == 37
    got = twice(lambda: run_gauss(params, K))["k"]
    ref = M.ref_gaussian_kernels(params, K)
    tol = np.maximum(M.ulp32(ref), 2.0 ** -126)
    err = np.abs(got.astype(np.float64) - ref) / tol
    print(f"gauss K={K}: {err.max():.3g} of the tolerance, sums within {np.abs(got.astype(np.float64).sum((1, 2)) - 1).max():.3g}")
    assert err.max() <= 1.0, f"element {np.unravel_index(err.argmax(), err.shape)}: {got.flat[err.argmax()]!r} vs {ref.flat[err.argmax()]!r}"
    assert np.abs(got.astype(np.float64).sum((1, 2)) - 1).max() < 1e-6
    for n in range(5):          # N = 1: one workgroup, the same bits as row n of the batch
        one = twice(lambda: run_gauss(params[n:n + 1], K))["k"]
        assert same_bits(one[0], got[n]), f"corner {n}: the N = 1 launch differs from the batch"


# ------------------------------------------------------------------------------------------- chunked loss reductions

def run_l1(c, wmap, want_sums, da_mode, gs_n=True, gscale=None):
    """da_mode: None (no gradient), 'store' (the slice starts as the sentinel) or 'acc' (starts as da0)"""
    N, Cc, hw = M.L1_SHAPE
    a, b, w = inp(c["a"]), inp(c["b"]), inp(c["wmap"] if wmap else None)
    g = inp(c["gs_n"]) if gs_n else None
    sums = Out(N, init=0.0) if want_sums else None
    da = None if da_mode is None else Out(N * Cc * hw, init=c["da0"] if da_mode == "acc" else None)
    call("csbsr_l1_fwd_bwd", _ptr(a), _ptr(b), _ptr(w), N, Cc, hw, sums.ptr if sums else None, c["gscale"] if gscale is None else gscale,
         _ptr(g), da.ptr if da else None, int(da_mode == "acc"))
    out = {}
    for name, o in (("sums", sums), ("da", da)):
        if o is not None:
            assert o.margins_intact(), f"csbsr_l1_fwd_bwd wrote outside {name}"
            out[name] = o.get(N, -1)
    return out


def test_l1_two_chunks_exact():
    from exact_lattice import mismatch
    c = M.l1_lattice()
    N = M.L1_SHAPE[0]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(N, -1))
    got = twice(lambda: run_l1(c, True, True, "store"))
    assert np.array_equal(got["sums"][:, 0], c["sums_w"]), f"weighted sums: got {got['sums'][:, 0].tolist()}, want {c['sums_w'].tolist()}"
    assert np.array_equal(got["da"], c["da_w"].reshape(N, -1)), "weighted gradient: " + mismatch(t(got["da"]), t(c["da_w"]))
    got = twice(lambda: run_l1(c, False, True, None))
    assert np.array_equal(got["sums"][:, 0], c["sums_1"]), f"plain sums: got {got['sums'][:, 0].tolist()}, want {c['sums_1'].tolist()}"
    got = twice(lambda: run_l1(c, True, False, "acc"))
    assert np.array_equal(got["da"], (c["da0"] + c["da_w"]).reshape(N, -1)), "accumulated gradient: " + mismatch(t(got["da"]), t(c["da0"] + c["da_w"]))
    got = twice(lambda: run_l1(c, False, True, "acc"))
    assert np.array_equal(got["sums"][:, 0], c["sums_1"])
    assert np.array_equal(got["da"], (c["da0"] + c["da_1"]).reshape(N, -1)), "accumulated plain gradient: " + mismatch(t(got["da"]), t(c["da0"] + c["da_1"]))
    got = twice(lambda: run_l1(c, False, False, "store", gs_n=False, gscale=0.25))          # no per-sample scale
    want = 0.25 * np.sign(c["da_1"]).reshape(N, -1)
    assert np.array_equal(got["da"], want), "unscaled gradient: " + mismatch(t(got["da"]), t(want))


def run_plane(c, with_b):
    planes, hw = M.PLANE_SHAPE
    a, b = inp(c["a"]), inp(c["b"] if with_b else None)
    out = Out(planes * 2, init=0.0)
    call("csbsr_plane_reduce", _ptr(a), _ptr(b), planes, hw, out.ptr)
    assert out.margins_intact(), "csbsr_plane_reduce wrote outside its output"
    return dict(out=out.get(planes, 2))


def test_plane_reduce_two_chunks_exact():
    c = M.plane_lattice()
    got = twice(lambda: run_plane(c, False))["out"]
    assert np.array_equal(got[:, 0], c["sum_a"]) and np.array_equal(got[:, 1], c["sum_aa"]), (got.tolist(), c["sum_a"].tolist(), c["sum_aa"].tolist())
    got = twice(lambda: run_plane(c, True))["out"]
    assert np.array_equal(got[:, 0], c["sum_a"]) and np.array_equal(got[:, 1], c["sum_ab"]), (got.tolist(), c["sum_a"].tolist(), c["sum_ab"].tolist())


def test_segloss_two_chunks():
    from oracle import csbsr_oracle as O
    N, H, W = M.SEG_SHAPE
    hw = H * W
    p, t = M.segloss_inputs()
    sdf = torch.from_numpy(O.compute_sdf(t.numpy()))                      # fp64; rounded to fp32 for the kernel AND the reference
    sdf32 = sdf.float()
    alpha, weight = 0.6, 0.4
    gsc = torch.tensor([0.5, 2.0])
    pd = p.double().requires_grad_(True)
    loss = O.boundary_combo_loss(pd, t.double(), alpha, O.PathCfg(bce_w=(20.0, 1.0), wbd_w=(1.0, 2.0)), sdf32.double())
    assert loss.dtype == torch.float64
    (loss * gsc.double() * weight).sum().backward()

    def run():
        dp_, dt, ds, dg = inp(p), inp(t), inp(sdf32), inp(gsc)
        sums, lo, dp = Out(N * 8, init=0.0), Out(N, init=0.0), Out(N * hw)
        call("csbsr_segloss_reduce", _ptr(dp_), _ptr(dt), _ptr(ds), N, hw, sums.ptr, 20.0, 1.0)
        call("csbsr_segloss_finish", _ptr(dp_), _ptr(dt), _ptr(ds), N, hw, sums.ptr, alpha, 20.0, 1.0, 1.0, 2.0, weight, _ptr(dg), lo.ptr, dp.ptr, 0)
        for o in (sums, lo, dp):
            assert o.margins_intact(), "the segmentation loss wrote outside an output"
        return dict(sums=sums.get(N, 8), loss=lo.get(), dp=dp.get(N, hw))

    got = twice(run)
    assert np.array_equal(got["sums"][:, 3].astype(np.float64), t.double().sum((1, 2, 3)).numpy()), "sum t^2 is an integer: every pixel once"
    assert np.array_equal(got["sums"][:, 5:], np.zeros((N, 3), np.float32)), "the unused columns of the sums were written"
    ref_l, ref_g = (weight * loss.detach()).numpy(), pd.grad.reshape(N, hw).numpy()
    e_l = np.abs(got["loss"] - ref_l).max() / np.abs(ref_l).max()
    e_g = np.abs(got["dp"] - ref_g).max() / np.abs(ref_g).max()
    print(f"segloss: loss {e_l:.3g}, gradient {e_g:.3g} of the maximum")
    assert e_l < 1e-5
    assert e_g < 1e-4
    zero = (p.reshape(N, hw) == 0).numpy()
    assert zero.sum() >= 14 and (got["dp"][zero] == 0).all(), "clamp(min=1e-8) passes no gradient at p == 0"
