"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol include/csbsr_hip.h declares, the
ctypes structures match the C layout, host logic (config, state_dict names, alpha schedule, deterministic fill,
synthetic data) behaves like the reference's, and the product refuses to run without the HIP path."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    from csbsr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "csbsr_amd", "csrc"), "-j8"], check=True)
    return _lib.LIB_PATH


def test_library_exports_every_declared_symbol(lib_path):
    from csbsr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    declared = set(re.findall(r"\b(csbsr_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"csbsr_seg_t", "csbsr_conv_desc_t"}
    lib = ctypes.CDLL(lib_path)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in csbsr_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    lib.csbsr_version.restype = ctypes.c_int
    assert lib.csbsr_version() >= 100


def test_ctypes_struct_sizes_match_c(lib_path, tmp_path):
    """sizeof() of every descriptor struct as seen by a C compiler == ctypes.sizeof of its mirror."""
    from csbsr_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "csbsr_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(csbsr_seg_t),'
                   ' sizeof(csbsr_conv_desc_t), sizeof(csbsr_wgrad_desc_t), sizeof(csbsr_epi_bwd_desc_t), sizeof(csbsr_bn_desc_t));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(c) for c in (_lib.Seg, _lib.ConvDesc, _lib.WgradDesc, _lib.EpiBwdDesc, _lib.BnDesc)]
    assert got == want


def test_bad_arguments_are_reported_not_thrown(lib_path):
    from csbsr_amd import _lib as L
    L.load()
    d = L.ConvDesc()
    with pytest.raises(L.CsbsrHipError, match="null pointer"):
        L.call("csbsr_conv_forward", ctypes.byref(d), None)


def test_state_dict_matches_reference_layout():
    from csbsr_amd.config import cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.modeling.shapes import joint_state_shapes
    m = JointModelWithLoss(cfg.clone(), 1000, 0, None)
    sd = m.state_dict()
    shapes = joint_state_shapes()
    assert list(sd.keys()) == list(shapes.keys())
    assert len(sd) == 410 and len(list(m.parameters())) == 290
    assert sum(p.numel() for p in m.parameters()) == 89249704
    assert all(tuple(sd[k].shape) == tuple(shapes[k]) for k in sd)
    # the golden fixtures carry the reference's own parameter-name list
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_pspnet_it1.npz"))
    ref_names = [str(n) for n in g["grad_names"]]
    mine = [k for k, v in m._named_full() if isinstance(v, torch.nn.Parameter)]
    assert mine == ref_names
    # round trip + reference-style key fixing
    sd2 = {k: torch.full_like(v, 0.5) if v.is_floating_point() else v for k, v in sd.items()}
    m.load_state_dict(sd2)
    assert float(m.state_dict()["sr_model.feat.0.weight"].mean()) == 0.5
    with pytest.raises(RuntimeError):
        m.load_state_dict({"nope": torch.zeros(1)}, strict=True)


@pytest.mark.parametrize("detector,scale,fixture,n_state,n_param,n_elem,n_train", [
    ("PSPNet_BlurSkip", 8, "e2e_blurskip_x8_it40000", 442, 316, 127318388, 26),        # config 5: only blur_skip.* trains
    ("HRNet_OCR", 4, "e2e_hrnet_ocr_it40000", 2051, 1109, 135658533, 1109),           # config 4
])
def test_state_dict_of_other_detectors(detector, scale, fixture, n_state, n_param, n_elem, n_train):
    """state_dict layout / parameter order / trainable set of the config 4 and 5 models equal the reference's (the fixtures carry
    the reference's own named_parameters() list; the counts are SURVEY.md section 8c's)."""
    from csbsr_amd.config import cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    c = cfg.clone()
    c.MODEL.DETECTOR_TYPE, c.MODEL.SCALE_FACTOR = detector, scale
    m = JointModelWithLoss(c, 1000, 0, None)
    assert len(m.state_dict()) == n_state
    params = [(k, v) for k, v in m._named_full() if isinstance(v, torch.nn.Parameter)]
    assert len(params) == n_param and sum(v.numel() for _, v in params) == n_elem
    assert sum(v.requires_grad for _, v in params) == n_train
    g = np.load(os.path.join(ROOT, "tests", "golden", fixture + ".npz"))
    assert [k for k, _ in params] == [str(n) for n in g["grad_names"]]
    trainable_ref = {str(n) for n, nrm in zip(g["grad_names"], g["grad_norms"]) if nrm >= 0}
    assert {k for k, v in params if v.requires_grad} == trainable_ref


def test_alpha_schedule_matches_reference_rule():
    """BoundaryComboLoss alpha bookkeeping (loss_functions.py:27-41, 76-81)."""
    from csbsr_amd.modeling.build_model import BoundaryComboState
    s = BoundaryComboState(per_epoch=10, resume_iter=0)
    assert s.alpha == 1.0 and s.iter == 0
    alphas = []
    for _ in range(25):
        s.update_alpha()
        alphas.append(round(s.alpha, 4))
    assert alphas[0] == 0.99 and alphas[9] == 0.99 and alphas[10] == 0.98 and alphas[20] == 0.97
    s2 = BoundaryComboState(per_epoch=10, resume_iter=995)
    assert abs(s2.alpha - 0.01) < 1e-12 and s2.iter == 5
    s2.fix_alpha = True
    a0 = s2.alpha
    for _ in range(30):
        s2.update_alpha()
    assert s2.alpha == a0


def test_config_tree_accepts_the_reference_yaml(tmp_path):
    from csbsr_amd.config import cfg, path_config
    c = cfg.clone()
    y = tmp_path / "c.yaml"
    y.write_text("SOLVER:\n  TASK_LOSS_WEIGHT: 0.3\n  BATCH_SIZE: 6\n  SR_PRETRAIN_ITER: [1, 30001]\nMODEL:\n  SR: \"KBPN\"\n  SCALE_FACTOR: 4\n"
                 "BLUR:\n  KERNEL_SIZE: 7\nINPUT:\n  IMAGE_SIZE: [224, 224]\n")
    c.merge_from_file(str(y))
    c.freeze()
    with pytest.raises(AttributeError):
        c.MODEL.SR = "x"
    p = path_config(c)
    assert (p.scale, p.ksize, p.ksize_out, p.beta) == (4, 7, 21, 0.3)
    assert p.sr_w == (0.4, 0.4, 0.0)        # defaults.py:72 literally [0.4, 0.4, 0, 2]


def test_unsupported_variants_fail_loudly():
    from csbsr_amd.config import cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    c = cfg.clone()
    c.MODEL.DETECTOR_TYPE = "u-net16"
    with pytest.raises(NotImplementedError):
        JointModelWithLoss(c, 1000, 0, None)
    c = cfg.clone()
    c.SOLVER.SEG_LOSS_FUNC = "Dice"
    with pytest.raises(NotImplementedError):
        JointModelWithLoss(c, 1000, 0, None)
    # every cfg key the path consumes is either honoured or refused -- never silently ignored
    for key, val in (("MODEL.NUM_CLASSES", 2), ("MODEL.SUM_LR_ERROR_POS", "mid"),
                     ("MODEL.SR_SEG_INV", True), ("MODEL.JOINT_LEARNING", False), ("SOLVER.INTERM_SSLOSSWEGHT4SR", True),
                     ("SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", 1.0), ("SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SS_AMP", 1.0), ("MODEL.SR", "DBPN")):
        c = cfg.clone()
        c.merge_from_list([key, val])
        with pytest.raises(NotImplementedError):
            JointModelWithLoss(c, 1000, 0, None)
    # ... and the honoured ones reach the flat path configuration the kernels read
    c = cfg.clone()
    c.merge_from_list(["MODEL.SR_RESIDUAL_LEARNING", False, "SOLVER.ONLY_KERNEL_LOSS_FOR_PRETRAIN", True, "MODEL.SR_PIXEL_SHUFFLE", True])
    m = JointModelWithLoss(c, 1000, 0, None)
    assert m.pc.residual_learning is False and m.pc.only_kernel_loss is True and m.pc.pixel_shuffle is True
    # the two KBPN structure variants change the state_dict as the reference's constructor does (kbpn.py:169-171, 369-374)
    c = cfg.clone()
    c.merge_from_list(["MODEL.KBPN_KERNEL_SFT", False, "MODEL.SUM_LR_ERROR_POS", "LR"])
    m = JointModelWithLoss(c, 1000, 0, None)
    keys = list(m.state_dict().keys())
    assert m.pc.kernel_sft is False and m.pc.lr_error is True
    assert not any(".sft." in k for k in keys) and not any(".kb.up_conv1." in k for k in keys)
    assert sum(1 for k in keys if k.endswith(".kb.conv.layer.weight")) == 4 and len(keys) == 410 - 3 * 8 - 4
    # ... in the reference's own parameter order (the fixtures carry its named_parameters() list)
    from golden_utils import load_golden
    for case, ov in (("e2e_pspnet_nosft_it40000", ["MODEL.KBPN_KERNEL_SFT", False]), ("e2e_pspnet_lrerr_it40000", ["MODEL.SUM_LR_ERROR_POS", "LR"]),
                     ("e2e_pspnet_zeropad_it40000", ["MODEL.ZERO_PAD_KERNEL", True])):
        c = cfg.clone()
        c.merge_from_list(ov)
        mine = [k for k in JointModelWithLoss(c, 1000, 0, None).state_dict().keys() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
        assert mine == [str(n) for n in load_golden(case)["grad_names"]], case


def test_up_down_scheduler_matches_the_reference_rule():
    """lr_scheduler.py:31-42 as used by train.py:95-96 (LambdaLR multiplier)."""
    from csbsr_amd.utils.lr_scheduler import UpDownScheduler
    s = UpDownScheduler(30001, 0, True)
    assert [s(i) for i in (0, 30000, 100000, 100001, 124999, 125000, 200000)] == [1, 1, 1, 10, 10, 1, 1]
    assert UpDownScheduler(30001, 0, False)(110000) == 1
    r = UpDownScheduler(30001, 100000, True)          # resumed at iteration 100000: LambdaLR restarts its counter
    assert [r(i) for i in (0, 1, 24999, 25000)] == [1, 10, 10, 1]
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=2e-5)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=UpDownScheduler(2, 70001, True))
    opt.step(); sch.step()
    assert abs(opt.param_groups[0]["lr"] - 2e-4) < 1e-12


def test_warmup_multistep_lr_matches_the_reference_rule():
    """lr_scheduler.py:14-29: linear ramp from warmup_factor * SOLVER.LR to SOLVER.LR over warmup_iters steps, then constant (the
    milestones are never consulted); every parameter group gets that rate (the reference returns a one-element list, which current torch
    rejects for more than one group)."""
    from csbsr_amd.config import cfg
    from csbsr_amd.utils.lr_scheduler import WarmupMultiStepLR
    c = cfg.clone()
    c.SOLVER.LR = 2e-5
    opt = torch.optim.Adam([{"params": [torch.nn.Parameter(torch.zeros(1))]}, {"params": [torch.nn.Parameter(torch.zeros(1))], "lr": 7e-3}], lr=1.0)
    sch = WarmupMultiStepLR(c, opt, milestones=[3, 6], gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=4)
    seen = []
    for _ in range(8):
        seen.append(opt.param_groups[0]["lr"])
        opt.step(); sch.step()
    want = [2e-5 * f for f in (1 / 3, 1 / 3 + 2 / 3 * 0.25, 1 / 3 + 2 / 3 * 0.5, 1 / 3 + 2 / 3 * 0.75, 1, 1, 1, 1)]
    assert all(abs(a - b) < 1e-12 for a, b in zip(seen, want)), (seen, want)
    assert opt.param_groups[1]["lr"] == 2e-5


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    from csbsr_amd import _lib as L
    from csbsr_amd.config import cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    m = JointModelWithLoss(cfg.clone(), 1000, 0, None)
    with pytest.raises(L.CsbsrHipError):
        m(1, torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 32, 32), torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 21, 21))


def test_product_never_imports_the_oracle():
    for dp, _, fs in os.walk(os.path.join(ROOT, "csbsr_amd")):
        for f in fs:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b|from\s+oracle\s+import|importlib.*oracle", txt, re.M), f"{f} imports the oracle"


def test_synthetic_batch_shapes_and_determinism():
    from csbsr_amd.data.synthetic import make_batch
    x, hr, mask, k = make_batch(2, 16, seed=5)
    x2, hr2, mask2, k2 = make_batch(2, 16, seed=5)
    assert x.shape == (2, 3, 16, 16) and hr.shape == (2, 3, 64, 64) and mask.shape == (2, 1, 64, 64) and k.shape == (2, 1, 21, 21)
    assert torch.equal(x, x2) and torch.equal(mask, mask2)
    assert torch.allclose(k.sum((2, 3)), torch.ones(2, 1)) and float(mask.sum()) > 0 and set(mask.unique().tolist()) <= {0.0, 1.0}


def test_deterministic_fill_is_reproducible():
    from csbsr_amd.utils.detfill import det_state_dict
    from csbsr_amd.modeling.shapes import kbpn_shapes
    shapes = {k: v for k, v in list(kbpn_shapes().items())[:12]}
    a, b = det_state_dict(shapes), det_state_dict(shapes)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert float(a["sr_model.feat.0.weight"].std()) > 0


def test_kernel_branch_table_is_the_two_conv_branch():
    """csbsr_amd.modeling.kbpn.kernel_branch_table -- the fe_kernel branch of KernelPredictorLikeIKC (kbpn.py:565-569) as a [B, 25, c]
    two-ring class table -- against the branch computed literally with F.conv2d on the expanded map, forward and backward (fp64)."""
    import torch.nn.functional as F
    from csbsr_amd.modeling.kbpn import kernel_branch_table, border_tap_mask, ring_tap_classes
    gen = torch.Generator().manual_seed(5)
    B, cin, c0, c1, co, H, W = 2, 11, 7, 6, 5, 7, 9
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_(True)
    kv, w0, w1, wt = rnd(B, cin), rnd(c0, cin, 3, 3), rnd(c1, c0, 3, 3), rnd(co, c1)
    act = lambda t: F.leaky_relu(t, 0.01)
    tab = kernel_branch_table(kv, w0, w1, wt, border_tap_mask().double(), ring_tap_classes().double(), act, act)
    y = F.conv2d(act(F.conv2d(act(F.conv2d(kv[:, :, None, None].expand(B, cin, H, W), w0, padding=1)), w1, padding=1)), wt[:, :, None, None])
    typ = lambda v, n: v if v < 2 else (v - n + 5 if v >= n - 2 else 2)
    g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    sums = torch.zeros(B, 5, 5, co, dtype=torch.float64)
    for i in range(H):
        for j in range(W):
            assert float((tab[:, typ(i, H), typ(j, W)] - y[:, :, i, j]).abs().max()) < 1e-12
            sums[:, typ(i, H), typ(j, W)] += g[:, :, i, j]
    for a, b in zip(torch.autograd.grad(y, [kv, w0, w1, wt], g, retain_graph=True), torch.autograd.grad(tab, [kv, w0, w1, wt], sums)):
        assert float((a - b).abs().max()) < 1e-10


def test_kernel_row_names_agree_between_bench_and_profiles():
    """bench.py names a launch by the id the library reports (csbsr_debug_last_conv_kernel: kernel in the low byte, template instance above),
    scripts/summarise_profiles.py names the same launch by its rocprofv3 row: csbsr_amd/utils/kernel_names.py must give both the SAME string, or
    the roofline block's PMC lookups silently miss (review r04, item 8)."""
    from csbsr_amd.utils.kernel_names import conv_row, wgrad_row, canon, family
    pairs = [
        (7 | (1 << 8), "_Z22conv_igemm_glds_kernelILi256ELi4ELi2ELi2ELb1ELb0EEv5ConvKPKDF16_"),
        (3 | (2 << 8), "void conv_igemm_glds_kernel<128, 2, 2, 1, false, true>(ConvK, _Float16 const*)"),
        (14, "_Z22conv_igemm_glds_kernelILi128ELi2ELi2ELi0ELb0ELb0EEv5ConvKPKDF16_"),
        (9 | ((2 | 4 | 8) << 8), "_Z14conv_tp_kernelILi2ELb0ELb1ELb1ELb1EEv7ConvTpKPKDF16_PDF16_"),
        (9 | (1 << 8), "_Z14conv_tp_kernelILi2ELb1ELb0ELb0ELb0EEv7ConvTpKPKDF16_PDF16_"),
        (8 | ((4 | 8) << 8), "void conv_hr_kernel<4, false, 9, 2, true, false>(ConvHrK)"),
        (8 | ((1 | 2 | 32) << 8), "void conv_hr_kernel<7, false, 1, 1, false, true>(ConvHrK)"),
        (17, "_Z14conv_x3_kernelILi3ELi1024EEv5ConvK7X3ExtraPKDF16_"),
        (10 | (1 << 8), "_Z14conv_x3_kernelILi3ELi2048EEv5ConvK7X3ExtraPKDF16_"),
        (18, "_Z14conv_x3_kernelILi2ELi1024EEv5ConvK7X3ExtraPKDF16_"),
        (13, "void conv_thin_cin2_kernel<false>(ConvK, int, int, int, int, Cin2Dact)"),
        (20 | ((1 | 4 | 8) << 8), "void conv_x3n_kernel<true, false, true, true>(ConvK, XNExtra)"),
        (20 | ((1 | 4) << 8), "_Z15conv_x3n_kernelILb1ELb0ELb1ELb0EEv5ConvK7XNExtra"),
        (20 | (3 << 8), "_Z15conv_x3n_kernelILb1ELb1ELb0ELb0EEv5ConvK7XNExtra"),
        (20, "void conv_x3n_kernel<false, false, false, false>(ConvK, XNExtra)"),
    ]
    for kid, raw in pairs:
        assert conv_row(kid) == canon(raw), (kid, conv_row(kid), canon(raw))
    for kid, raw in [(7, "_Z22conv_wgrad_glds_kernelILi256ELi256ELi2ELi4ELi2ELb1EEv6WgradKPKDF16_"),
                     (9, "_Z22conv_wgrad_glds_kernelILi128ELi512ELi2ELi4ELi2ELb1EEv6WgradKPKDF16_"),
                     (3, "void conv_wgrad_kernel<32, 128, 1, 4, true>(WgradK)"), (8, "void conv_wgrad_hr_kernel<7, 4, 4, 4>(WgradHrK)")]:
        assert wgrad_row(kid) == canon(raw), (kid, wgrad_row(kid), canon(raw))
    assert family("conv_tp_kernel<res=1,acc=0,mask=0,sums=0>") == "conv_tp_kernel" and family("epilogue_bwd_kernel") == "epilogue_bwd_kernel"


def test_bench_refuses_a_rank_count_it_cannot_run():
    """bench.py --gpus N must never fall back to a silent 1-GPU run (round-5 review): a launcher WORLD_SIZE that disagrees with --gpus, or
    fewer visible devices than ranks, exits non-zero before anything touches a GPU."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSBSR_FORCE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="3", RANK="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=3" in r.stderr and not r.stdout.strip()
    import torch
    n = torch.cuda.device_count()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n + 1)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "visible" in r.stderr and not r.stdout.strip()


def test_bench_dump_outputs_writes_float32_with_a_fixed_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: small tensors whole, larger ones as the same seeded sample of positions in every run, all float32."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    big = torch.randn(2, 3, 40, 40, generator=torch.Generator().manual_seed(0))
    for d in ("a", "b"):
        bench.dump_outputs({"sr_preds": big, "loss": torch.tensor(0.25, dtype=torch.float64), "kernel_preds": big[:, :1, :5, :5]}, str(tmp_path / d))
    a, b = np.load(tmp_path / "a" / "sr_preds.npy"), np.load(tmp_path / "b" / "sr_preds.npy")
    assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
    assert np.isin(a, big.numpy().reshape(-1)).all()
    k = np.load(tmp_path / "a" / "kernel_preds.npy")
    assert k.dtype == np.float32 and np.array_equal(k, big[:, :1, :5, :5].numpy())
    assert np.load(tmp_path / "a" / "loss.npy").dtype == np.float32 and float(np.load(tmp_path / "a" / "loss.npy")) == 0.25


def test_dropin_resolves_the_references_import_name():
    """csbsr_amd.dropin.install(): `from model.modeling.build_model import JointModelWithLoss, JointModel` -- the reference's own import line
    (train.py:30, test.py:21) -- yields this build's classes; the names it does not build raise NotImplementedError on construction; nothing
    else of the `model` package is shadowed.  Run in a child interpreter (the finder and the placeholder packages are process-global)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import csbsr_amd.dropin as d\n"
        "assert d.install() and not d.install()\n"
        "from model.modeling.build_model import JointModelWithLoss, JointModel, JointInvModelWithLoss, SRModelWithLoss, JointInvModel\n"
        "from csbsr_amd.modeling import build_model as B\n"
        "assert JointModelWithLoss is B.JointModelWithLoss and JointModel is B.JointModel\n"
        "for c in (JointInvModelWithLoss, SRModelWithLoss, JointInvModel):\n"
        "    try:\n"
        "        c(None)\n"
        "    except NotImplementedError:\n"
        "        pass\n"
        "    else:\n"
        "        raise SystemExit('unbuilt class constructed')\n"
        "import importlib.util\n"
        "assert importlib.util.find_spec('model.engine') is None or 'csbsr' not in str(importlib.util.find_spec('model.engine').origin)\n"
        "d.uninstall()\n"
        "print('ok')\n") % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
