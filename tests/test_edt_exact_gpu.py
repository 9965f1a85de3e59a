"""Exact parity of the Euclidean distance transform of csrc/image_ops.hip through the C ABI: csbsr_sdf (edt_cols_kernel, edt_rows_kernel,
sdf_combine_kernel) and csbsr_crack_weight (crack_cols_kernel, crack_rows_weight_kernel, whose row search is a copy of edt_rows_kernel's)
on every row of the geometry table of tests/edt_cases.py -- references, the model of the block-bounded search, the mutants and the proof
that the rows catch them are validated without a GPU by tests/test_edt_cases_cpu.py.  The guarded call harness is tests/abi_harness.py:
the shared reduction scratch refilled with NaN, the mask inside a NaN-filled allocation (and the same bits after the call), the outputs
and the NaN-preset scratch inside sentinel-filled allocations whose margins are checked, every row twice with identical bits.

What is asked
  csbsr_sdf            rows with H^2 + W^2 < 2^24: BIT FOR BIT edt_cases.sdf_restated32 (numpy float32; sqrtf and / are correctly rounded on
                       the device), the sign of a zero aside.  Every row: within the counted bound of oracle.csbsr_oracle.compute_sdf in
                       float64, 3 * 2^-24 + 2^-44 on those rows and 5 * 2^-24 + 2^-44 on the wider ones (counted in edt_cases' docstring).
                       Only the pixels of a sample of nothing but foreground are left out (the reference is NaN there; the kernel
                       writes -1, which the restatement asks bit for bit), and only the row all_foreground has one.
  csbsr_crack_weight   w == lambda exactly on foreground pixels and on samples without foreground; elsewhere within (amp d + 2) 2^-23
                       relative of lambda exp(-amp d), d the float64 distance (the bound of tests/test_crack_weight_gpu.py), at the row's
                       amp = 80 / diagonal, for which an error of 1 in d2 misses that bound wherever d2 <= 2^21 and no weight is below
                       FLT_MIN (edt_cases.weight_amp).  w_lr: F.interpolate of the device's own w_hr on the CPU within 4 ulp.
  soft masks           the foreground rule is the reference's astype(np.uint8): the rows soft_values, soft_halo, seeded_sparse and the
                       loader row (a DeviceTrainLoader batch with resized_crop, its sdf against compute_sdf of its own mask) FAIL on a
                       kernel with the ``!= 0`` rule -- seen on the MI355X against the library built before the rule changed: 698
                       elements of soft_values, 545 of soft_halo and 19 199 of seeded_sparse differ from the restatement, and the
                       loader row is 5.6e6 bounds away from float64 (an error of about 1: a sample the reference leaves at zero) -- and
                       pass with the truncation rule; the other 138 tests pass on both libraries.
  bad arguments        W = 8193, null pointers, an LR map whose scale does not divide the width: a non-zero status, nothing launched,
                       nothing written.

Measured on the MI355X: every bit-for-bit row identical in every element, and so are the three rows outside the exactness domain (not
asked: wide_1x3x4096, wide_1x2x4097, wide_1x3x8192 have few features, and no rounded sum decided a minimum); the assumption that sqrtf
and / are correctly rounded held.  Worst error / bound:
  csbsr_sdf against float64      0.646 (big_5x96x1000) on the exact rows, bound 3 * 2^-24;  0.204 / 0.196 / 0.193 on the three wide rows,
                                 bound 5 * 2^-24;  the loader row 0.288 (575 soft pixels in a (4, 1, 32, 48) batch)
  csbsr_crack_weight             0.822 (n3_extents, amp 0.2666) of (amp d + 2) 2^-23;  full_sparse 0.675;  w_lr at most 2 ulp
Wall time of this module on the MI355X: 1.3 s for its 142 tests, the slowest 0.08 s (w513_h40) after the first test's 0.47 s of set-up.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crack_weight_cases as CW
import edt_cases as E
from abi_harness import Out, _ptr, call, inp, same_bits, twice

pytestmark = pytest.mark.gpu
NAMES = [r["name"] for r in E.ROWS]


def run_sdf(mask):
    """csbsr_sdf on a guarded copy of ``mask`` [N, 1, H, W], twice -> float32 [N, 1, H, W]"""
    mask = np.array(mask, np.float32)          # (a writable copy: the cached masks are read-only)
    N, _, H, W = mask.shape
    npx = N * H * W

    def once():
        m, out, scratch = inp(mask), Out(npx), Out(3 * npx + 2 * N, init=float("nan"))
        call("csbsr_sdf", _ptr(m), out.ptr, scratch.ptr, N, H, W)
        assert out.margins_intact() and scratch.margins_intact(), "csbsr_sdf wrote outside its output or its scratch"
        assert same_bits(m.cpu().numpy(), mask.reshape(-1)), "csbsr_sdf changed its input"
        return dict(sdf=out.get(N, 1, H, W))
    return twice(once)["sdf"]


def run_weight(mask, amp, scale):
    mask = np.array(mask, np.float32)          # (a writable copy: the cached masks are read-only)
    N, _, H, W = mask.shape
    npx = N * H * W

    def once():
        m, w_hr, w_lr, scratch = inp(mask), Out(npx), Out(npx // (scale * scale)), Out(npx, init=float("nan"))
        call("csbsr_crack_weight", _ptr(m), w_hr.ptr, w_lr.ptr, scratch.ptr, N, H, W, float(amp), float(E.LAMBDA), scale)
        assert w_hr.margins_intact() and w_lr.margins_intact() and scratch.margins_intact(), "csbsr_crack_weight wrote outside a buffer"
        assert same_bits(m.cpu().numpy(), mask.reshape(-1)), "csbsr_crack_weight changed its input"
        return dict(w_hr=w_hr.get(N, 1, H, W), w_lr=w_lr.get(N, 1, H // scale, W // scale))
    r = twice(once)
    return r["w_hr"], r["w_lr"]


@pytest.mark.parametrize("name", NAMES)
def test_sdf(name):
    r = E.row(name)
    got = run_sdf(E.mask_of(name))
    ratio, left = E.sdf_ratio(got, name)
    wrong = E.sdf_mismatches(got, name)
    print(f"MEASURED sdf {name} ({r['N']}, {r['H']}, {r['W']}): error / bound {ratio:.3f} against float64, {wrong} elements differ from the "
          f"float32 restatement ({'asked' if r['exact'] else 'not asked: outside the exactness domain'}), {left} pixels left out")
    assert np.isfinite(got).all()
    assert left == (r["H"] * r["W"] * int(E.refs(name)[2].sum())) and (left > 0) == (name == "all_foreground")
    if r["exact"]:
        assert wrong == 0
    assert ratio <= 1


@pytest.mark.parametrize("name", NAMES)
def test_crack_weight(name):
    r = E.row(name)
    amp = E.weight_amp(name)
    scale = next(s for s in (4, 2, 1) if r["H"] % s == 0 and r["W"] % s == 0)
    w_hr, w_lr = run_weight(E.mask_of(name), amp, scale)
    ok, ratio = E.weight_check(w_hr, name)
    want = F.interpolate(torch.from_numpy(w_hr), scale_factor=1 / scale, mode="bilinear").numpy() if scale > 1 else w_hr
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(CW.FLT_MIN)))
    e_lr = float((np.abs(w_lr.astype(np.float64) - want.astype(np.float64)) / ulp).max())
    print(f"MEASURED weight {name} amp {amp:.4g} scale {scale}: relative error / bound {ratio:.3f}, w_lr {e_lr:.2f} ulp")
    assert ok, "w != lambda on a foreground pixel or in a sample without foreground"
    assert ratio <= 1
    assert w_lr.shape == want.shape and e_lr <= 4


def test_loader_batch_with_soft_mask():
    """a DeviceTrainLoader batch with resized_crop on (the pool and crop of tests/test_resized_crop_gpu.py): the mask has soft pixels, and
    the sdf the loader hands out is compute_sdf of that mask within the counted bound"""
    from test_resized_crop_gpu import make_loader
    ld = make_loader()[3]
    sel, params = ld.draw(4)
    mask, sdf = (t.cpu().numpy() for t in ld.batch(sel, params)[2::2])
    soft = int(((mask > 0) & (mask < 1)).sum())
    assert soft > 0 and mask.shape == sdf.shape and not E.all_foreground(mask).any()
    err = float(np.abs(sdf.astype(np.float64) - E.sdf_ref64(mask)).max()) / E.sdf_bound(True)
    print(f"MEASURED loader batch {mask.shape}: {soft} soft pixels, error / bound {err:.3f}")
    assert E.is_exact(*mask.shape[2:]) and err <= 1
    assert same_bits(run_sdf(mask), sdf)          # the loader's call is the guarded call


def test_bad_arguments_write_nothing():
    from csbsr_amd._lib import CsbsrHipError
    W = E.MAX_W + 1
    mask = np.zeros((1, 1, 1, W), np.float32)
    mask[0, 0, 0, 5] = 1
    m = inp(mask)
    outs = [Out(W), Out(3 * W + 2), Out(W), Out(W)]          # sdf, its scratch, w_hr, the weight's scratch
    sdf, scr, w_hr, wscr = outs
    bad = [("csbsr_sdf", (_ptr(m), sdf.ptr, scr.ptr, 1, 1, W)),
           ("csbsr_sdf", (None, sdf.ptr, scr.ptr, 1, 1, 64)),
           ("csbsr_sdf", (_ptr(m), None, scr.ptr, 1, 1, 64)),
           ("csbsr_sdf", (_ptr(m), sdf.ptr, None, 1, 1, 64)),
           ("csbsr_crack_weight", (_ptr(m), w_hr.ptr, None, wscr.ptr, 1, 1, W, 0.1, 2.0, 1)),
           ("csbsr_crack_weight", (None, w_hr.ptr, None, wscr.ptr, 1, 1, 64, 0.1, 2.0, 1)),
           ("csbsr_crack_weight", (_ptr(m), None, None, wscr.ptr, 1, 1, 64, 0.1, 2.0, 1)),
           ("csbsr_crack_weight", (_ptr(m), w_hr.ptr, None, None, 1, 1, 64, 0.1, 2.0, 1)),
           ("csbsr_crack_weight", (_ptr(m), w_hr.ptr, sdf.ptr, wscr.ptr, 1, 1, 66, 0.1, 2.0, 4))]          # an LR map of a width 4 does not divide
    for entry, args in bad:
        with pytest.raises(CsbsrHipError):
            call(entry, *args)
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs), f"{entry}{args[3:]} wrote something before it refused"
    assert same_bits(m.cpu().numpy(), mask.reshape(-1))
    # the widest accepted row next to it is served (wide_1x3x8192 asks its values)
    assert E.row("wide_1x3x8192")["W"] == E.MAX_W
