"""SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP on the device: the kernel csbsr_crack_weight against the reference's own maps, the weighted SR
loss against exact identities and against the reference's e2e fixtures (forward and the gradients of sr_loss.mean()), and a short
do_train run across ORIENTED_WEIGHT_ITER with a resume in the middle.  Fixtures: tests/golden/make_crack_weight_golden.py."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crack_weight_cases as CW
from golden_utils import load_golden, max_rel_to_scale

pytestmark = pytest.mark.gpu

LAM = np.float32(CW.LAMBDA)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("tag,amp", CW.CASES)
def test_kernel_matches_the_reference_maps(tag, amp):
    """w_hr against CrackOrientedExpWeight's output: exactly lambda on foreground pixels and on samples without (or of nothing but)
    foreground; elsewhere a relative error of at most (amp * d + 2) * 2^-23 -- one ulp on d moves the exponent's argument by
    amp * d * 2^-24, plus two ulp for the two expf implementations, doubled as margin -- or, where the reference value is below FLT_MIN
    (the device may flush denormals), an absolute error of FLT_MIN.  w_lr against F.interpolate of the device's OWN w_hr on the CPU: a
    four-term sum with weight 0.25 in any order, 4 ulp.  Two runs give the same bits."""
    g = CW.maps()
    mask, ref = g[f"mask_{tag}"], g[f"w_hr_{tag}_{amp:g}"]
    w_hr, w_lr = CW.run_kernel(mask, amp)
    fg, d = CW.foreground(mask), CW.distance(mask)
    none = ~fg.reshape(fg.shape[0], -1).any(1)
    assert (w_hr[fg] == LAM).all()
    assert (w_hr[none] == LAM).all() and (w_hr[fg.reshape(fg.shape[0], -1).all(1)] == LAM).all()
    if tag == "a":
        assert none.tolist() == [False, True, False, False] and fg[2].all()
        for y, x in ((5, 7), (20, 150)):          # the soft pixels (0.5, 0.99) are background: the weight of their distance to the corner pixel
            assert mask[3, 0, y, x] not in (0.0, 1.0) and w_hr[3, 0, y, x] < LAM and d[3, 0, y, x] == np.sqrt(float((39 - y) ** 2 + (299 - x) ** 2))
    refd, gotd = ref.astype(np.float64), w_hr.astype(np.float64)
    normal = refd >= CW.FLT_MIN
    rel = np.abs(gotd - refd)[normal] / refd[normal]
    bound = ((amp * d + 2) * 2.0 ** -23)[normal]
    sub = np.abs(gotd - refd)[~normal]
    print(f"{tag} amp {amp:g}: worst relative error / bound {float((rel / bound).max()):.3f}, sub-FLT_MIN pixels {int((~normal).sum())}"
          f" (worst |diff| {float(sub.max()) if sub.size else 0.0:.2e}), bit-equal pixels {float((_bits(w_hr) == _bits(ref)).mean()):.4f}")
    assert (rel <= bound).all() and (sub <= CW.FLT_MIN).all()
    want = F.interpolate(torch.from_numpy(w_hr), scale_factor=1 / CW.SCALE, mode="bilinear").numpy()
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(CW.FLT_MIN)))
    e_lr = np.abs(w_lr.astype(np.float64) - want.astype(np.float64)) / ulp
    print(f"    w_lr vs F.interpolate(device w_hr): worst {float(e_lr.max()):.2f} ulp; vs the reference's LR map {max_rel_to_scale(w_lr, g[f'w_lr_{tag}_{amp:g}']):.2e}")
    assert w_lr.shape == want.shape and (e_lr <= 4).all()
    again_hr, again_lr = CW.run_kernel(mask, amp)
    assert np.array_equal(_bits(again_hr), _bits(w_hr)) and np.array_equal(_bits(again_lr), _bits(w_lr))
    only_hr, no_lr = CW.run_kernel(mask, amp, lr=False)          # the LR map is optional and changes nothing else
    assert no_lr is None and np.array_equal(_bits(only_hr), _bits(w_hr))


# ----------------------------------------------------------------------------------------------------------------- 2. the model
def _model(g, co_sr_amp=0.0, ow_iter=-1, sfo_sr_amp=0.0):
    """tests/test_joint_gpu.build_model with the crack-oriented key"""
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    cfg = base_cfg.clone()
    cfg.MODEL.SCALE_FACTOR, cfg.MODEL.DETECTOR_TYPE = int(g["scale"]), "PSPNet"
    cfg.SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP, cfg.SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SR_AMP = float(co_sr_amp), float(sfo_sr_amp)
    cfg.SOLVER.ORIENTED_WEIGHT_ITER = int(ow_iter)
    m = JointModelWithLoss(cfg, 1000, 0, None, antialias=bool(g["antialias"]))
    deterministic_fill(m.state_dict())
    m.ss_loss_fn.alpha = float(g["alpha"])
    m.micro_batch, m.max_resident = 8, 8
    m.train()
    m.dropout_masks = {}          # every Dropout2d is the identity
    return m


def _fixture_model(g):
    return _model(g, float(g["co_sr_amp"]), int(g["oriented_w_iter"]), float(g["sfo_sr_amp"]))


def _forward(m, g, it=None, mask=None):
    t = lambda k: torch.from_numpy(g[k])
    return m(int(g["it"]) if it is None else it, t("x"), sr_targets=t("hr"), segment_targets=t("mask") if mask is None else mask,
             kernel_targets=t("kernel"))


def test_forward_is_exact_where_the_weight_is_a_constant():
    """A mask without a foreground pixel: w^C = 2 everywhere, and with SR_LOSS_FUNC_SR_WEIGHT = [0.4, 0.4, 0] the SR loss of the w^C model
    is EXACTLY twice the plain model's (a scaling by 2 is exact in fp32, so any re-ordering of the weighted sums would show); everything
    else has the same bits.  At iter <= ORIENTED_WEIGHT_ITER every output has the plain model's bits."""
    g = load_golden("e2e_pspnet_it40000")
    it = int(g["it"])
    empty = torch.zeros(g["mask"].shape)
    names = ("segment_loss", "sr_loss", "segment_preds", "sr_preds", "kernel_preds")
    with torch.no_grad():
        plain = dict(zip(names, (v.cpu() for v in _forward(_model(g), g, mask=empty))))
        m = _model(g, co_sr_amp=0.1, ow_iter=it - 1)
        assert m.pc.sr_w == (0.4, 0.4, 0.0)
        on = dict(zip(names, (v.cpu() for v in _forward(m, g, mask=empty))))
        off = dict(zip(names, (v.cpu() for v in _forward(_model(g, co_sr_amp=0.1, ow_iter=it), g, mask=empty))))
        real = dict(zip(names, (v.cpu() for v in _forward(m, g))))          # the fixture's own mask: the weight is no constant there
    assert float(plain["sr_loss"].min()) > 0
    assert torch.equal(on["sr_loss"], 2 * plain["sr_loss"]), (on["sr_loss"], plain["sr_loss"])
    for k in names:
        if k != "sr_loss":
            assert torch.equal(on[k], plain[k]), k
        assert torch.equal(off[k], plain[k]), k
    assert not torch.equal(real["sr_loss"], on["sr_loss"]) and torch.equal(real["sr_preds"], on["sr_preds"])


def _run(g):
    m = _fixture_model(g)
    it = int(g["it"])
    seg_l, sr_l, seg, sr, kp = _forward(m, g)
    pc = m.pc
    loss = (1 - pc.beta) * sr_l.mean() + pc.beta * seg_l.mean()
    assert not (pc.joint_pretrain[0] <= it < pc.joint_pretrain[1])
    loss.backward()
    torch.cuda.synchronize()
    outs = dict(segment_loss=seg_l.detach().cpu(), sr_loss=sr_l.detach().cpu(), segment_preds=seg.cpu(), sr_preds=sr.cpu(),
                kernel_preds=kp.cpu(), loss=float(loss))
    bufs = {k: v.detach().cpu() for k, v in m.state_dict().items() if "running" in k}
    return outs, bufs


@pytest.mark.parametrize("case", ["e2e_pspnet_wco_it40000", "e2e_pspnet_wcofo_it40000"])
def test_forward_matches_the_reference(case):
    """The quantities, the helper and the bounds of tests/test_joint_gpu.py::test_forward_matches_golden.  w^C alone is an exact constant of
    the mask, so its SR loss gets the unweighted bound 1e-3; with w^F on as well the loss inherits the segmentation map's conditioning
    through exp(|seg - mask|) and gets that test's 5e-3."""
    from test_joint_gpu import SEG_BOUND
    from oracle import csbsr_oracle as O
    g = load_golden(case)
    assert float(g["co_sr_amp"]) == 0.1 and int(g["oriented_w_iter"]) == 100 and float(g["sfo_sr_amp"]) == (1.0 if "wcofo" in case else 0.0)
    b_seg, b_segl, b_bn, b_iou = SEG_BOUND["PSPNet"]
    outs, bufs = _run(g)
    worst = {k: max_rel_to_scale(outs[k], g[k]) for k in ("segment_preds", "sr_preds", "kernel_preds", "segment_loss", "sr_loss")}
    e_bn = max(max_rel_to_scale(bufs[k[4:]], v) for k, v in g.items() if k.startswith("buf."))
    iou = float(O.iou(outs["segment_preds"], torch.from_numpy(g["segment_preds"])).min())
    print(case, {k: f"{v:.1e}" for k, v in worst.items()}, f"BN buffers {e_bn:.1e} IoU vs ref {iou:.4f}")
    for k in ("sr_preds", "kernel_preds", "sr_loss"):
        assert worst[k] < (5e-3 if k == "sr_loss" and float(g["sfo_sr_amp"]) != 0 else 1e-3), (k, worst[k])
    assert worst["segment_preds"] < b_seg and worst["segment_loss"] < b_segl and e_bn < b_bn and iou > b_iou
    assert abs(outs["loss"] - float(g["loss"])) < b_segl * abs(float(g["loss"]))


_digest_errors = {}


def _srgrad_errors(case):
    """Per ``sr_model.*`` tensor of more than one element: |norm - reference norm| / reference norm of d(mean sr_loss)/d(parameter), and the
    relative L2 distance of the 32 recorded elements, against the reference's digests -> {name: (norm error, sample error)}.  Detector
    parameters must get no gradient."""
    if case in _digest_errors:
        return _digest_errors[case]
    g = load_golden(case)
    if "srgrad_names" in g:
        m = _fixture_model(g)
        dig = g
    else:
        m = _model(g)
        dig = load_golden(case + "_srgrad")
    sr_l = _forward(m, g)[1]
    sr_l.mean().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in m._named_full() if isinstance(v, torch.nn.Parameter)}
    for n, gr in grads.items():
        if n.startswith("segmentation_model"):
            assert gr is None or float(gr.abs().max()) == 0.0, n
    errs = {}
    for n, ref_norm, ref_s in zip((str(v) for v in dig["srgrad_names"]), dig["srgrad_norms"], dig["srgrad_samples32"]):
        assert grads[n] is not None, n
        flat = grads[n].detach().cpu().reshape(-1)
        if flat.numel() == 1 or ref_norm < 1e-9:          # (PReLU slopes: signed sums with heavy cancellation, tests/test_joint_gpu.py)
            continue
        idx = [(zlib.crc32((n + str(j)).encode()) % flat.numel()) for j in range(32)]
        e_s = float(np.linalg.norm(flat[idx].double().numpy() - ref_s) / (np.linalg.norm(ref_s.astype(np.float64)) + 1e-30))
        errs[n] = (abs(float(flat.double().norm()) - ref_norm) / ref_norm, e_s)
    assert len(errs) > 100
    _digest_errors[case] = errs
    return errs


def _summary(errs):
    from test_joint_gpu import gate_flip_prone
    e = np.array([v[0] for v in errs.values()])
    calm = np.array([v[0] for n, v in errs.items() if not gate_flip_prone(n)])
    return float(e.max()), float(np.median(calm)), float(calm.max()), float(max(v[1] for v in errs.values()))


@pytest.mark.parametrize("case", ["e2e_pspnet_wco_it40000", "e2e_pspnet_wcofo_it40000"])
def test_sr_loss_gradients_match_the_reference_digests(case):
    """d(mean sr_loss)/d(parameters) against the second backward of the reference, recorded as digests.  The yardstick is measured first
    with the same method on the UNWEIGHTED case (e2e_pspnet_it40000 against e2e_pspnet_it40000_srgrad.npz): worst per-tensor relative norm
    error, and over the tensors that are not gate_flip_prone its median and maximum.  w^C is an exact constant of the mask, so its
    gradients are held to twice those figures and never to more than tests/test_joint_gpu.py::test_sr_loss_gradients_match_oracle
    allows (0.1 per tensor, median 5e-3, maximum 3e-2); with w^F on as well the bounds are that test's own for its wf case.  The 32
    recorded elements of every tensor are held to the per-tensor 0.1 in relative L2.
    Measured (MI355X; worst per tensor / median / maximum of the relative norm error, then the worst 32-element error):
        unweighted  3.12e-3 / 2.63e-4 / 2.10e-3, 1.03e-1
        wco         2.06e-3 / 2.24e-4 / 2.06e-3, 8.55e-3      -> bounds 6.24e-3 / 5.26e-4 / 4.20e-3
        wcofo       1.62e-3 / 1.98e-4 / 1.62e-3, 7.79e-3"""
    base_all, base_med, base_max, base_smp = _summary(_srgrad_errors("e2e_pspnet_it40000"))
    e_all, e_med, e_max, e_smp = _summary(_srgrad_errors(case))
    print(f"unweighted: per-tensor {base_all:.2e}  median {base_med:.2e}  max {base_max:.2e}  samples {base_smp:.2e}")
    print(f"{case}: per-tensor {e_all:.2e}  median {e_med:.2e}  max {e_max:.2e}  samples {e_smp:.2e}")
    if "wcofo" in case:
        b_all, b_med, b_max = 0.1, 5e-3, 3e-2
    else:
        b_all, b_med, b_max = min(2 * base_all, 0.1), min(2 * base_med, 5e-3), min(2 * base_max, 3e-2)
    assert e_all < b_all and e_med < b_med and e_max < b_max, ((e_all, b_all), (e_med, b_med), (e_max, b_max))
    assert e_smp < 0.1


# ----------------------------------------------------------------------------------------------------------------- 3. the trainer
def test_do_train_crosses_the_start_iteration_and_resumes(tmp_path):
    """Four iterations over a DeviceTrainLoader (crop 64, scale 4, batch 2) with ORIENTED_WEIGHT_ITER = 2: iterations 1 and 2 log the SR
    loss of a run without the key, bit for bit, iterations 3 and 4 another one; a run saved at 2 and resumed into new objects is the
    uninterrupted run, bit for bit."""
    from csbsr_amd import trainer as T
    from csbsr_amd.data.resident import DeviceTrainLoader
    from test_trainer_gpu import _pool, _small_model
    from csbsr_amd.config import cfg as base_cfg
    ds = _pool()
    loader = lambda n, seed: DeviceTrainLoader(ds, 64, 4, batch_size=2, num_iterations=n, seed=seed, drop_last=True)

    def cfg_of(amp):
        cfg = base_cfg.clone()
        cfg.MODEL.SCALE_FACTOR, cfg.MODEL.DETECTOR_TYPE, cfg.SOLVER.BATCH_SIZE = 4, "PSPNet", 2
        cfg.SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP, cfg.SOLVER.ORIENTED_WEIGHT_ITER = amp, 2
        return cfg

    def run(cfg, model, opt, ld, resume_iter, out=None):
        logs = []
        T.do_train(cfg, model, opt, T.build_scheduler(cfg, opt, resume_iter), ld, resume_iter=resume_iter, log_step=1, save_step=2,
                   output_dir=out, log=logs.append)
        return [(r["iteration"], r["segment_loss"], r["sr_loss"]) for r in logs if "sr_loss" in r]

    def fresh(cfg, resume_iter, seed=5):
        torch.manual_seed(seed)
        m = _small_model(cfg, resume_iter)
        return m, T.build_optimizer(cfg, m)
    off, on = cfg_of(0.0), cfg_of(0.1)
    m, opt = fresh(off, 0)
    logs_off = run(off, m, opt, loader(4, 31), 0)
    full, opt_full = fresh(on, 0)
    logs_on = run(on, full, opt_full, loader(4, 31), 0)
    assert [r[0] for r in logs_on] == [1, 2, 3, 4] == [r[0] for r in logs_off]
    assert logs_on[:2] == logs_off[:2]
    assert logs_on[2][2] != logs_off[2][2] and logs_on[3][2] != logs_off[3][2]
    first, opt_first = fresh(on, 0)
    logs_a = run(on, first, opt_first, loader(2, 31), 0, str(tmp_path))
    del first, opt_first
    second, opt_second = fresh(on, 0, seed=777)
    torch.rand(3, device="cuda:0")
    ld = loader(4, 999)
    it = T.resume(on, str(tmp_path), 2, second, opt_second, ld)
    assert it == 2
    logs_b = run(on, second, opt_second, ld, it)
    assert logs_a + logs_b == logs_on
    sd, sd_full = second.state_dict(), full.state_dict()
    for name, t in sd.items():
        assert torch.equal(t, sd_full[name]), name
