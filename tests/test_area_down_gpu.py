"""SOLVER.DOWNSCALE_INTERPOLATION = 'area' on the device: csbsr_area_down_fwd / _bwd through the C ABI against torch's own
F.interpolate(mode='area') and its autograd on the CPU -- bit for bit at f = 2, 4, 8 --, the two LR paths of the resident loader, the loss
models against the REFERENCE's fixtures (tests/golden/e2e_pspnet_area_it*.npz, made by tests/golden/make_area_golden.py), and the trainer's
data-against-loss check."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import area_cases as AC
from golden_utils import max_rel_to_scale

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # floats of 0xA5 bytes either side of every output


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guarded(shape, offset=0, fill=None):
    """an fp32 tensor of ``shape`` inside a guard band; ``offset`` floats past a 16-byte boundary.  -> (tensor, check())"""
    n = int(np.prod(shape))
    whole = torch.full(((GUARD + offset + n + GUARD) * 4,), 0xA5, dtype=torch.uint8, device=DEV)
    t = whole.view(torch.float32)[GUARD + offset:GUARD + offset + n].view(*shape)
    if fill is not None:
        t.fill_(fill)
    lo, hi = (GUARD + offset) * 4, (GUARD + offset + n) * 4

    def check():
        assert bool((whole[:lo] == 0xA5).all()) and bool((whole[hi:] == 0xA5).all()), "a write outside the output"
    return t, check


def _at_offset(a, offset):
    """``a`` (numpy) on the device, ``offset`` floats past a 16-byte boundary (torch allocations are 256-byte aligned)"""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def _fwd(x, f, y):
    from csbsr_amd import _lib as L
    planes, H, W = x.shape
    with torch.cuda.device(x.device):
        L.call("csbsr_area_down_fwd", _ptr(x), _ptr(y), planes, H, W, f, L.stream(x.device))
    return y


def _bwd(dy, f, dx, accumulate=0):
    from csbsr_amd import _lib as L
    planes, H, W = dx.shape
    with torch.cuda.device(dx.device):
        L.call("csbsr_area_down_bwd", _ptr(dy), _ptr(dx), int(accumulate), planes, H, W, f, L.stream(dx.device))
    return dx


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(planes, H, W, f, seed=0):
    """(x, dy, torch's y, torch's dx) on the host, computed once per shape"""
    x = AC.random_input(planes, H, W, seed=7 * f + H + seed)
    dy = AC.random_input(planes, H // f, W // f, seed=7 * f + H + seed + 1)
    y, dx = AC.torch_area(x, f, dy)
    return x, dy, y, dx


def _run_both(x, dy, f, offset=0):
    """forward and backward into guarded outputs, twice -> (y, dx) on the host; the two runs must agree bit for bit"""
    planes, H, W = x.shape
    xd, dyd = _at_offset(x, offset), _at_offset(dy, offset)
    outs = []
    for _ in range(2):
        y, check_y = _guarded((planes, H // f, W // f), offset)
        dx, check_dx = _guarded((planes, H, W), offset)
        _fwd(xd, f, y)
        _bwd(dyd, f, dx)
        torch.cuda.synchronize()
        check_y()
        check_dx()
        outs.append((y.clone(), dx.clone()))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    return outs[0][0].cpu(), outs[0][1].cpu()


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("f", [2, 4, 8])
def test_kernels_equal_torch_bit_for_bit(f):
    """planes = 6 with one output per plane, 32 x 40, and 65 outputs per row (one lane past a wave) -- tests/area_cases.kernel_shapes, with
    its note on f = 8 -- against F.interpolate(mode='area') and its autograd on the CPU (area_cases.torch_area, with its note on the
    1 x 1 output): torch.equal, forward and backward.  accumulate = 1 into a buffer of ones against 1 + grad at f*f * 2^-23 * max|dy|."""
    for planes, H, W in AC.kernel_shapes(f):
        x, dy, want_y, want_dx = _case(planes, H, W, f)
        y, dx = _run_both(x, dy, f)
        assert torch.equal(_bits(y), _bits(torch.from_numpy(want_y))), (f, planes, H, W, float((y - torch.from_numpy(want_y)).abs().max()))
        assert torch.equal(_bits(dx), _bits(torch.from_numpy(want_dx))), (f, planes, H, W)
        ones, check = _guarded((planes, H, W), fill=1.0)
        _bwd(torch.from_numpy(dy).to(DEV), f, ones, accumulate=1)
        torch.cuda.synchronize()
        check()
        err = float((ones.cpu() - (1.0 + torch.from_numpy(want_dx))).abs().max())
        assert err <= f * f * 2.0 ** -23 * float(np.abs(dy).max()), (f, planes, H, W, err)


@pytest.mark.parametrize("case", [AC.WRAP_CASE, AC.WRAP_CASE_TWO_PER_LANE])
def test_grid_stride_loop_wraps(case):
    """3 x 1700 x 1704 at f = 2: 2.17 M outputs and 2.17 M float4s of dx, more than the 8192 x 256 threads of the capped grid, so the
    loop of the backward and of a one-output-per-lane forward wraps.  The f = 2 forward owns TWO outputs per lane (one float4 per input
    row): its loop wraps on the second case, 6 planes of the same image."""
    planes, H, W, f = case
    x, dy, want_y, want_dx = _case(planes, H, W, f)
    assert planes * (H // f) * (W // f) > 8192 * 256 and planes * H * W // 4 > 8192 * 256
    if case == AC.WRAP_CASE_TWO_PER_LANE:
        assert planes * (H // f) * (W // f) // 2 > 8192 * 256
    xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    y, check_y = _guarded((planes, H // f, W // f))
    dx, check_dx = _guarded((planes, H, W))
    _fwd(xd, f, y)
    _bwd(dyd, f, dx)
    torch.cuda.synchronize()
    check_y()
    check_dx()
    assert torch.equal(_bits(y.cpu()), _bits(torch.from_numpy(want_y))) and torch.equal(_bits(dx.cpu()), _bits(torch.from_numpy(want_dx)))


@pytest.mark.parametrize("f", [2, 4, 8])
def test_scalar_path_on_a_view_four_bytes_into_its_allocation(f):
    """input, output and both gradients start 4 bytes past a 16-byte boundary: no float4 can be used; same sums in the same order"""
    planes, H, W = AC.kernel_shapes(f)[1]
    x, dy, want_y, want_dx = _case(planes, H, W, f)
    y, dx = _run_both(x, dy, f, offset=1)
    assert torch.equal(_bits(y), _bits(torch.from_numpy(want_y))) and torch.equal(_bits(dx), _bits(torch.from_numpy(want_dx)))
    if f == 2:          # and the wrap of the one-output-per-lane forward, on the issue's wrap case
        planes, H, W, _ = AC.WRAP_CASE
        x, dy, want_y, want_dx = _case(planes, H, W, 2)
        y, check = _guarded((planes, H // 2, W // 2), 1)
        _fwd(_at_offset(x, 1), 2, y)
        torch.cuda.synchronize()
        check()
        assert torch.equal(_bits(y.cpu()), _bits(torch.from_numpy(want_y)))


def test_factor_three_within_the_rounding_of_nine_terms():
    """f = 3: f*f is no power of two and torch's area is bit-equal to neither 'divide by 9' nor 'multiply by 1/9'.  Both sides round a sum
    of at most f*f terms and one quotient: f*f * 2^-23 * max|x| (forward), f*f * 2^-23 * max|dy| (backward)."""
    f = 3
    for planes, H, W in ((6, 3, 3), (6, 33, 39), (6, 36, 65 * 3)):
        x, dy, want_y, want_dx = _case(planes, H, W, f)
        y, dx = _run_both(x, dy, f)
        e_y, e_dx = float((y - torch.from_numpy(want_y)).abs().max()), float((dx - torch.from_numpy(want_dx)).abs().max())
        print(f"f=3 {planes}x{H}x{W}: forward {e_y:.2e} backward {e_dx:.2e}")
        assert e_y <= 9 * 2.0 ** -23 * float(np.abs(x).max()) and e_dx <= 9 * 2.0 ** -23 * float(np.abs(dy).max())
        # the contract itself (one division by f*f) is met exactly
        assert torch.equal(_bits(y), _bits(torch.from_numpy(AC.area_down(x, f)))) and torch.equal(_bits(dx), _bits(torch.from_numpy(AC.area_down_bwd(dy, f))))


def test_bad_arguments_return_an_error_and_launch_nothing():
    from csbsr_amd import _lib as L
    x = torch.ones(2, 8, 12, device=DEV)
    st = L.stream(x.device)
    y = torch.full((2, 8, 12), 7.0, device=DEV)          # large enough for any of the calls below, had they run
    dx = torch.full((2, 8, 12), 7.0, device=DEV)
    for H, W, f in ((8, 12, 3), (8, 12, 8), (8, 12, 0), (8, 12, -2), (7, 12, 2)):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_area_down_fwd", _ptr(x), _ptr(y), 2, H, W, f, st)
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_area_down_bwd", _ptr(x), _ptr(dx), 0, 2, H, W, f, st)
    for a, b in ((None, y), (x, None)):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_area_down_fwd", _ptr(a), _ptr(b), 2, 8, 12, 2, st)
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_area_down_bwd", _ptr(a), _ptr(b), 0, 2, 8, 12, 2, st)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((dx == 7.0).all())
    L.call("csbsr_area_down_fwd", _ptr(x), _ptr(y), 2, 8, 12, 2, st)          # and the error state does not stick
    torch.cuda.synchronize()
    assert bool((y.view(-1)[:2 * 4 * 6] == 1.0).all())


# ------------------------------------------------------------------------------------------------------------------ the data path
def _dataset():
    from csbsr_amd.data.resident import ResidentDataset
    import resident_cases as RC
    images, masks = RC.random_pairs(np.random.default_rng(3), [(40, 52), (36, 45), (33, 38), (50, 33), (37, 64), (44, 41)])
    return ResidentDataset(images, masks, device=DEV)


def test_loader_without_blur_yields_the_area_downscale_of_its_hr():
    from csbsr_amd.data.resident import DeviceTrainLoader
    ld = DeviceTrainLoader(_dataset(), 32, 4, batch_size=4, seed=5, num_iterations=2, blur=False, interpolation="area", drop_last=True)
    n = 0
    for x, hr, mask, k, sdf in ld:
        want = torch.from_numpy(AC.torch_area(hr.cpu().reshape(-1, 32, 32).numpy(), 4)).reshape(x.shape)
        assert tuple(x.shape) == (4, 3, 8, 8) and tuple(hr.shape) == (4, 3, 32, 32) and torch.equal(_bits(x.cpu()), _bits(want))
        n += 1
    assert n == 2


def test_loader_with_blur_against_the_cpu_blur_and_torch_area():
    """x = area(blur(hr)): 1e-5 of the maximum, csbsr_blur_fwd's own bound (tests/test_elementwise_gpu.py); the box mean adds none"""
    from csbsr_amd.data.resident import DeviceTrainLoader
    ld = DeviceTrainLoader(_dataset(), 32, 4, batch_size=4, seed=5, num_iterations=2, interpolation="area")
    for x, hr, mask, k, sdf in ld:
        hr_c, k_c = hr.cpu(), k.cpu()
        K = k_c.shape[-1]
        blurred = torch.cat([F.conv2d(hr_c[b:b + 1], k_c[b].expand(3, 1, K, K), padding=(K - 1) // 2, groups=3) for b in range(hr_c.shape[0])])
        want = F.interpolate(blurred, size=(8, 8), mode="area")
        err = max_rel_to_scale(x.cpu(), want)
        print(f"loader x vs CPU area(blur(hr)): {err:.2e}")
        assert err <= 1e-5


def test_the_name_changes_no_draw_no_state_and_nothing_but_x():
    from csbsr_amd.data.resident import DeviceTrainLoader
    ds = _dataset()
    a = DeviceTrainLoader(ds, 32, 4, batch_size=4, seed=11, num_iterations=3, interpolation="area")
    b = DeviceTrainLoader(ds, 32, 4, batch_size=4, seed=11, num_iterations=3)
    for (sa, pa), (sb, pb) in zip(a.iter_decisions(), b.iter_decisions()):
        assert torch.equal(sa, sb) and torch.equal(pa, pb)
        ba, bb = a.batch(sa, pa), b.batch(sb, pb)
        assert all(torch.equal(u, v) for u, v in zip(ba[1:], bb[1:])) and not torch.equal(ba[0], bb[0])
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for key in sa:
        assert (sa[key] is None and sb[key] is None) or torch.equal(torch.as_tensor(sa[key]), torch.as_tensor(sb[key])), key


# ------------------------------------------------------------------------------------------------------------------ the models
def _cfg(g, downscale):
    from csbsr_amd.config import cfg as base_cfg
    cfg = base_cfg.clone()
    cfg.MODEL.SCALE_FACTOR, cfg.MODEL.DETECTOR_TYPE = int(g["scale"]), str(g["detector"])
    cfg.SOLVER.TASK_LOSS_WEIGHT = float(g["beta"])
    cfg.SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SR_AMP, cfg.SOLVER.ORIENTED_WEIGHT_ITER = float(g["sfo_sr_amp"]), int(g["oriented_w_iter"])
    cfg.SOLVER.DOWNSCALE_INTERPOLATION = downscale
    return cfg


def _joint(g, downscale):
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    m = JointModelWithLoss(_cfg(g, downscale), 1000, 0, None, antialias=bool(g["antialias"]), device=DEV)
    deterministic_fill(m.state_dict())
    m.ss_loss_fn.alpha = float(g["alpha"])
    m.micro_batch, m.max_resident = 8, 8
    m.dropout_masks = {}
    m.train()
    return m


def _inputs(g):
    return tuple(torch.from_numpy(g[k]) for k in ("x", "hr", "mask", "kernel"))


def test_the_downscale_reaches_the_loss_and_nothing_else():
    """equal weights, equal inputs: KBPN, the detector and its loss never see the down-sampler; the SR loss does"""
    outs = {}
    for case in ("e2e_pspnet_area_it1", "e2e_pspnet_area_it40000"):
        g = AC.load_fixture(case)
        x, hr, mask, k = _inputs(g)
        for mode in ("area", "bicubic"):
            m = _joint(g, mode)
            assert m.downscale == mode
            with torch.no_grad():
                outs[mode] = [t.clone() for t in m(int(g["it"]), x, sr_targets=hr, segment_targets=mask, kernel_targets=k)]
            del m
        (seg_la, sr_la, seg_a, sr_a, k_a), (seg_lb, sr_lb, seg_b, sr_b, k_b) = outs["area"], outs["bicubic"]
        assert torch.equal(sr_a, sr_b) and torch.equal(k_a, k_b)
        if int(g["it"]) == 40000:
            assert torch.equal(seg_a, seg_b) and torch.equal(seg_la, seg_lb)
        assert bool((sr_la != sr_lb).all())


# measured on an MI355X (see the docstring below): max |last_dkvec - reference| / max |reference| of the bicubic control
DKVEC_CONTROL_MEASURED = 1.88e-6


@pytest.mark.parametrize("mode", ["area", "bicubic"])
def test_loss_and_its_seeds_against_the_reference_on_its_own_sr_image(mode):
    """forward_from_sr fed the it1 fixture's own sr_preds / kernel_preds: the loss terms and their backward down to the SR image and the
    kernel vector, on the reference's bits.  'bicubic' is the CONTROL: the fixture's ctl_* keys, parent code only.

      sr_loss     1e-5 relative: two L1 means of values within csbsr_blur_fwd's 1e-5
      last_dsr    1e-5 of the reference gradient's maximum: the HR term is a sign on identical bits, the LR term csbsr_blur_bwd_input's
                  bound; min |lr_pred - x| >= 1e-4 (the fixture's seed condition) rules out a flipped sign, so no element is left out
      last_dkvec  3 x the control's measured value, at least 1e-4 (csbsr_blur_bwd_kernel's bound).  The fixture holds d sr_loss.sum() /
                  d kernel_preds, the gradient at the NORMALISED kernel the model returns; last_dkvec is the gradient at the vector that
                  was fed, i.e. that gradient through the normalisation v / sum(v) -- applied to the fixture's in fp64 here.

                  Measured: control 1.88e-6, area 2.03e-6 (of max |reference| = 2.8e-2 / 2.5e-2), so the bound is its floor, 1e-4.

    Measured beside them: sr_loss 6.9e-8 (area) / 7.7e-8 (control), last_dsr 6.7e-7 / 9.5e-7.
    (The control asserts the last_dkvec bound only: the antialiased bicubic kernels carry tolerances of their own, tests/test_elementwise_gpu.py.)"""
    g = AC.load_fixture("e2e_pspnet_area_it1")
    key = (lambda k: k) if mode == "area" else (lambda k: "ctl_" + k)
    x, hr, mask, k = _inputs(g)
    B = x.shape[0]
    m = _joint(g, mode)
    kvec = torch.from_numpy(g["kernel_preds"]).reshape(B, -1)
    seg_l, sr_l, seg, sr, kp = m.forward_from_sr(1, torch.from_numpy(g["sr_preds"]), kvec, x, hr, mask, k)
    sr_l.sum().backward()
    torch.cuda.synchronize()
    want_l = torch.from_numpy(g[key("sr_loss")])
    e_loss = float(((sr_l.detach().cpu() - want_l).abs() / want_l.abs()).max())
    e_dsr = max_rel_to_scale(m.last_dsr.cpu(), g[key("dsr")])
    v = kvec.double()
    ksum = v.sum(1, keepdim=True)
    dvec = torch.from_numpy(g[key("dkpred")]).reshape(B, -1).double()
    want_dk = (dvec - (dvec * (v / ksum)).sum(1, keepdim=True)) / ksum
    e_dk = max_rel_to_scale(m.last_dkvec.cpu(), want_dk)
    print(f"[{mode}] sr_loss {e_loss:.2e}  last_dsr {e_dsr:.2e}  last_dkvec {e_dk:.2e}  (max |dkvec| {float(want_dk.abs().max()):.3e}, "
          f"max |dvec| {float(dvec.abs().max()):.3e})")
    assert float(g["min_abs_lr_diff"]) >= 1e-4
    if mode == "area":
        assert e_loss <= 1e-5 and e_dsr <= 1e-5, (e_loss, e_dsr)
    assert e_dk <= max(3 * DKVEC_CONTROL_MEASURED, 1e-4), e_dk


def _run_step(m, g, joint=True):
    from csbsr_amd.trainer import calc_loss
    x, hr, mask, k = _inputs(g)
    it = int(g["it"])
    if joint:
        seg_l, sr_l, seg, sr, kp = m(it, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)
        loss = calc_loss(seg_l, sr_l, it, m.cfg)
    else:
        sr_l, sr, kp = m(it, x, sr_targets=hr, kernel_targets=k)
        seg_l = seg = None
        loss = sr_l.mean()
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m._named_full() if isinstance(p, torch.nn.Parameter)}
    return dict(segment_loss=seg_l, sr_loss=sr_l.detach(), segment_preds=seg, sr_preds=sr, kernel_preds=kp, loss=float(loss.detach())), grads


@pytest.mark.parametrize("case", ["e2e_pspnet_area_it1", "e2e_pspnet_area_it40000"])
def test_end_to_end_against_the_reference_fixture(case):
    """Forward: the bounds tests/test_joint_gpu.py::test_forward_matches_golden applies to its plain PSPNet cases (SR image, kernel, SR loss
    1e-3 of the maximum; the composed map / loss / BatchNorm buffers / IoU its SEG_BOUND sanity constants; the scalar within the loss
    bound).  Gradients: the sampled digest as tests/test_bicubic_sr_gpu.py compares one (test_wc_parity_gpu._grad_errors) with the per-phase
    bounds of test_gradients_match_oracle -- SR phase 3e-2 per tensor (0.1 where a gate flip is possible, scalars 0.1 + 2e-3 absolute),
    median < 5e-3; joint phase median < 0.5, 90th percentile < 0.7."""
    from oracle import csbsr_oracle as O
    from test_joint_gpu import SEG_BOUND, gate_flip_prone
    from test_wc_parity_gpu import _grad_errors
    g = AC.load_fixture(case)
    b_seg, b_segl, b_bn, b_iou = SEG_BOUND["PSPNet"]
    m = _joint(g, "area")
    outs, grads = _run_step(m, g)
    worst = {k: max_rel_to_scale(outs[k].detach().cpu(), g[k]) for k in ("segment_preds", "sr_preds", "kernel_preds", "segment_loss", "sr_loss")}
    sd = m.state_dict()
    e_bn = max(max_rel_to_scale(sd[kk[4:]].cpu(), v) for kk, v in g.items() if kk.startswith("buf."))
    iou = float(O.iou(outs["segment_preds"].cpu(), torch.from_numpy(g["segment_preds"])).min())
    print(case, {k: f"{v:.1e}" for k, v in worst.items()}, f"BN buffers {e_bn:.1e} IoU vs ref {iou:.4f} loss {outs['loss']:.6f} / {float(g['loss']):.6f}")
    for k in ("sr_preds", "kernel_preds", "sr_loss"):
        assert worst[k] < 1e-3, (k, worst[k])
    assert worst["segment_preds"] < b_seg and worst["segment_loss"] < b_segl and e_bn < b_bn and iou > b_iou
    assert abs(outs["loss"] - float(g["loss"])) < b_segl * abs(float(g["loss"]))
    errs = _grad_errors(g, grads, "")
    joint = int(g["it"]) >= 30001
    big = np.array([max(en, es) for n, numel, en, es in errs if numel > 1])
    print(case, "grad digest: median %.2e p90 %.2e max %.2e (n=%d)" % (np.median(big), np.percentile(big, 90), big.max(), len(big)))
    # (iteration 1 trains the SR module alone: 76 tensors with a gradient; the joint phase 247)
    assert len(big) > (100 if joint else 50) and np.isfinite(big).all()
    if joint:
        assert np.median(big) < 0.5 and np.percentile(big, 90) < 0.7
    else:
        ref_norm = dict(zip((str(v) for v in g["grad_names"]), (float(v) for v in g["grad_norms"])))
        bad = [(n, en, es) for n, numel, en, es in errs if numel > 1 and max(en, es) > (0.1 if gate_flip_prone(n) else 3e-2)]
        # (a scalar's one sampled element IS the scalar: es * |ref| = |got - ref|, signed)
        bad += [(n, en, es) for n, numel, en, es in errs if numel == 1 and es * ref_norm[n] > 0.1 * ref_norm[n] + 2e-3]
        assert not bad, (len(bad), bad[:8])
        assert np.median(big) < 5e-3


def test_sr_only_model_is_the_joint_model_bit_for_bit_at_iteration_one():
    from csbsr_amd.modeling.build_model import SRModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    g = AC.load_fixture("e2e_pspnet_area_it1")
    joint = _joint(g, "area")
    j_out, j_grads = _run_step(joint, g)
    del joint
    sr_only = SRModelWithLoss(_cfg(g, "area"), antialias=bool(g["antialias"]), device=DEV)
    deterministic_fill(sr_only.state_dict())
    sr_only.micro_batch, sr_only.max_resident, sr_only.dropout_masks = 8, 8, {}
    sr_only.train()
    assert sr_only.downscale == "area"
    s_out, s_grads = _run_step(sr_only, g, joint=False)
    for k in ("sr_loss", "sr_preds", "kernel_preds"):
        assert torch.equal(s_out[k], j_out[k]), k
    assert s_out["loss"] == j_out["loss"]
    trained = 0
    for n, gr in s_grads.items():
        assert (gr is None) == (j_grads[n] is None) and (gr is None or torch.equal(gr, j_grads[n])), n
        trained += int(gr is not None and float(gr.abs().max()) > 0)
    assert trained > 50


# ------------------------------------------------------------------------------------------------------------------ the trainer
def test_three_steps_of_do_train_and_the_mismatch_check():
    from csbsr_amd import trainer as T
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.resident import DeviceTrainLoader, ResidentDataset
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    rng = np.random.default_rng(7)
    images, masks = [], []
    for H, W in ((64, 80), (72, 64), (80, 80), (66, 71)):
        yy, xx = np.mgrid[0:H, 0:W]
        base = 128 + 60 * np.sin(xx / rng.uniform(4, 9) + rng.uniform(0, 3)) * np.cos(yy / rng.uniform(4, 9))
        images.append(np.clip(base[:, :, None] + rng.normal(0, 12, size=(H, W, 3)), 0, 255).astype(np.uint8))
        masks.append((255 * (np.hypot(yy, xx) % 23 < 3)).astype(np.uint8))
    ds = ResidentDataset(images, masks, device=DEV)
    cfg = base_cfg.clone()
    cfg.SOLVER.BATCH_SIZE, cfg.SOLVER.DOWNSCALE_INTERPOLATION = 2, "area"
    model = JointModelWithLoss(cfg, len(images), 0, None, device=DEV)
    opt = T.build_optimizer(cfg, model)
    mk = lambda **kw: DeviceTrainLoader(ds, 64, 4, batch_size=2, num_iterations=3, seed=31, drop_last=True, **kw)
    with pytest.raises(ValueError, match="DOWNSCALE_INTERPOLATION"):
        T.do_train(cfg, model, opt, T.build_scheduler(cfg, opt), mk(), log_step=3, log=lambda r: None)
    with pytest.raises(ValueError, match="DOWNSCALE_INTERPOLATION"):
        T.validate(model, mk(), 1)
    assert all(p.grad is None for p in model.parameters())          # nothing ran
    logs = []
    T.do_train(cfg, model, opt, T.build_scheduler(cfg, opt), DeviceTrainLoader.from_cfg(cfg, ds, crop=64, num_iterations=3, seed=31, drop_last=True),
               log_step=3, log=logs.append)
    rec = [r for r in logs if "sr_loss" in r]
    assert len(rec) == 1 and rec[0]["iteration"] == 3 and np.isfinite(rec[0]["sr_loss"]) and rec[0]["sr_loss"] > 0
    assert np.isfinite(rec[0]["segment_loss"]) and rec[0]["overflow_steps"] == 0
