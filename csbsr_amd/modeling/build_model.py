"""Drop-in counterparts of the reference's ``model.modeling.build_model`` classes for the KBPN + PSPNet path:

    JointModelWithLoss(cfg, num_train_ds, resume_iter, sr_transforms)
        .forward(iter, x, sr_targets=None, segment_targets=None, kernel_targets=None)
            -> (segment_loss[B], sr_loss[B], segment_preds, sr_preds, kernel_preds[B,1,K,K])
    JointModel(cfg).forward(x, damy_kernel, sr_targets=None) -> (sr_preds, segment_preds, kernel_preds)
    SRModelWithLoss(cfg, sr_transforms, num_train_ds, resume_iter)
        .forward(iter, x, sr_targets=None, kernel_targets=None) -> (sr_loss[B], sr_preds, kernel_preds[B,1,K,K])

(/root/reference/model/modeling/build_model.py:323-416, 441-500).  Same constructor / forward signatures,
same state_dict keys, same attributes the trainer touches (``sr_model``, ``segmentation_model``,
``ss_loss_fn.{alpha,fix_alpha,iter,update_alpha()}``, ``iter_cnt``), same per-sample unreduced losses, so
``loss = calc_loss(...); loss.backward(); optimizer.step()`` from trainer.py:67-71 runs unchanged.

Underneath nothing is torch.nn: the forward hands raw device pointers to libcsbsr_hip.so (csbsr_amd/engine.py)
and the two loss vectors are outputs of one torch.autograd.Function whose backward runs the hand-written HIP
backward pass; PyTorch only owns memory, streams and the optimizer.
"""
import math
import os
import re
import warnings
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import _lib as L
from ..config import path_config
from ..config.defaults import check_downscale
from ..engine import Engine, _ptr
from ..utils.misc import fix_model_state_dict
from .kbpn import KBPN
from .pspnet import PSPNet
from .hrnet_ocr import HRNetOCR
from .shapes import joint_state_shapes


class BoundaryComboState:
    """alpha schedule of BoundaryComboLoss (loss_functions.py:27-41, 76-81); the loss itself is fused in HIP."""

    def __init__(self, per_epoch, resume_iter=0, alpha_min=0.01, decrease_ratio=1.0):
        self.per_epoch, self.alpha_min, self.decrease_ratio = per_epoch, alpha_min, decrease_ratio
        self.fix_alpha = False
        self.iter = resume_iter % per_epoch
        self.alpha = 1.0 - (resume_iter // per_epoch) * 0.01 * decrease_ratio
        self.alpha = alpha_min if self.alpha <= alpha_min else self.alpha

    def update_alpha(self):
        if self.iter % self.per_epoch == 0 and self.alpha > self.alpha_min and not self.fix_alpha:
            self.alpha -= 0.01 * self.decrease_ratio
            self.iter = 1
        else:
            self.iter += 1


class _ParamGroup(nn.Module):
    """Holds parameters / buffers under the reference's dotted names (``sr_model.feat.0.weight`` ...)."""

    def __init__(self, shapes, prefix):
        super().__init__()
        self._names = {}
        for full, shp in shapes.items():
            if not full.startswith(prefix + "."):
                continue
            local = full[len(prefix) + 1:]
            key = local.replace(".", "__")
            self._names[local] = key
            if full.endswith(("running_mean", "running_var")):
                self.register_buffer(key, torch.zeros(shp) if full.endswith("mean") else torch.ones(shp))
            elif full.endswith("num_batches_tracked"):
                self.register_buffer(key, torch.zeros((), dtype=torch.long))
            else:
                self.register_parameter(key, nn.Parameter(torch.zeros(shp)))

    def named_local(self):
        for local, key in self._names.items():
            yield local, getattr(self, key)


def _init_reference_style(name, t, gen):
    """Random init with the reference's distributions (kbpn.py:73-82 kaiming-normal convs / zero biases, PReLU 0.01;
    extractors.py:124-130 normal(0, sqrt(2/n)) convs, BN gamma=1 beta=0; pspnet PReLU 0.25, default Conv2d init elsewhere)."""
    with torch.no_grad():
        if t.dim() == 4:
            if name.startswith("sr_model") or ".blur_skip." in name:      # blocks.py:53-61 (kaiming / xavier normal)
                fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                t.normal_(0, math.sqrt(2.0 / fan_in), generator=gen)
            elif ".feats." in name:
                n = t.shape[2] * t.shape[3] * t.shape[0]
                t.normal_(0, math.sqrt(2.0 / n), generator=gen)
            else:
                fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                bound = 1.0 / math.sqrt(fan_in)
                t.uniform_(-bound, bound, generator=gen)
        elif name.endswith("act.weight"):
            t.fill_(0.01)
        elif name.endswith("conv.2.weight"):
            t.fill_(0.25)
        elif name.endswith(".weight"):
            t.fill_(1.0)
        else:
            t.zero_()


def pretrained_sr_path(cfg, root="weights"):
    """``<root>/pretrain/KBPN_pretrain_x{SCALE}_stage{S}[_bicubic{K}].pth`` (build_model.py:104-107): the file the SR-only regime leaves
    and every model with ``MODEL.SR_SCRATCH = False`` starts from; ``_bicubic{K}`` when BLUR.KERNEL_SIZE != BLUR.KERNEL_SIZE_OUTPUT."""
    name = f"KBPN_pretrain_x{cfg.MODEL.SCALE_FACTOR}_stage{cfg.MODEL.NUM_STAGES}"
    if cfg.BLUR.KERNEL_SIZE != cfg.BLUR.KERNEL_SIZE_OUTPUT:
        name += f"_bicubic{cfg.BLUR.KERNEL_SIZE}"
    return os.path.join(root, "pretrain", name + ".pth")


def load_pretrained_sr(model, cfg, root="weights"):
    """build_model.py:108-109: the file's keys lose ``len("sr_model.")`` leading characters (fix_model_state_dict), the load is
    non-strict (tensors the file does not name keep their init) and any key KBPN does not have is an error.  Returns the path."""
    path = pretrained_sr_path(cfg, root)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"MODEL.SR_SCRATCH=False needs the pretrained KBPN weights {path}")
    sd = fix_model_state_dict(torch.load(path, map_location="cpu"), addition_word="sr_model.")
    own = dict(model.sr_model.named_local())
    unexpected = [k for k in sd if k not in own]
    if unexpected:
        raise RuntimeError(f"unexpected_keys are exist in {path}.\n {unexpected[:8]}")
    with torch.no_grad():
        for k, v in sd.items():
            own[k].copy_(v)
    # (no slope probe to drop: this runs in the constructor, before the runtime and its engine exist -- see _JointBase.load_state_dict)
    return path


class _JointBase(nn.Module):
    def __init__(self, cfg, antialias=True, device="cuda:0", seed=None, pretrained_root="weights", sr_only=False, sr_transforms=None):
        super().__init__()
        # ``sr_only`` (SRModelWithLoss): KBPN and its loss alone -- no detector is constructed, moved to the device or given a gradient bucket
        self.sr_only = bool(sr_only)
        # MODEL.SR="bicubic" (build_model.py:69-73, 90-91): the paper's lower-bound row, the detector on the bicubically up-scaled LR image.
        # PSPNet_BlurSkip is not built with it: its SFT layers are fed KBPN's kernel estimate, which this model does not have
        self.bicubic = cfg.MODEL.SR == "bicubic" and not self.sr_only
        if self.sr_only:
            if cfg.MODEL.SR != "KBPN" or cfg.MODEL.SCALE_FACTOR == 1 or cfg.MODEL.SR_SEG_INV:
                raise NotImplementedError(f"csbsr_amd pretrains MODEL.SR='KBPN' on 3-channel images at SCALE_FACTOR > 1; got SR={cfg.MODEL.SR} "
                                          f"SCALE_FACTOR={cfg.MODEL.SCALE_FACTOR} SR_SEG_INV={cfg.MODEL.SR_SEG_INV}")
        elif cfg.MODEL.SR not in ("KBPN", "bicubic") or cfg.MODEL.DETECTOR_TYPE not in ("PSPNet", "PSPNet_BlurSkip", "HRNet_OCR") or \
                (self.bicubic and cfg.MODEL.DETECTOR_TYPE == "PSPNet_BlurSkip"):
            raise NotImplementedError(f"csbsr_amd builds KBPN + PSPNet / PSPNet_BlurSkip / HRNet_OCR and bicubic + PSPNet / HRNet_OCR; got "
                                      f"SR={cfg.MODEL.SR} DETECTOR_TYPE={cfg.MODEL.DETECTOR_TYPE}")
        if self.bicubic and cfg.MODEL.SCALE_FACTOR % 4:      # csbsr_aa_bicubic_up stores four outputs of one input cell per lane
            raise NotImplementedError(f"MODEL.SR='bicubic' with SCALE_FACTOR={cfg.MODEL.SCALE_FACTOR}: a multiple of 4")
        if cfg.MODEL.SUM_LR_ERROR_POS not in ("HR", "LR"):      # kbpn.py:174-187: the reference's forward handles exactly these two
            raise NotImplementedError(f"MODEL.SUM_LR_ERROR_POS={cfg.MODEL.SUM_LR_ERROR_POS!r}: 'HR' or 'LR'")
        if not self.sr_only:
            if cfg.MODEL.NUM_CLASSES != 1:      # build_model.py:209: every kernel of this path assumes the 1-class crack map
                raise NotImplementedError(f"MODEL.NUM_CLASSES={cfg.MODEL.NUM_CLASSES}: only the 1-class detectors are built")
            if cfg.MODEL.SR_SEG_INV or not cfg.MODEL.JOINT_LEARNING:
                raise NotImplementedError("only MODEL.JOINT_LEARNING=True with SR_SEG_INV=False (SR feeds the detector, one joint loss) is built")
        self.cfg = cfg
        self.pc = path_config(cfg, antialias)
        # SOLVER.DOWNSCALE_INTERPOLATION (train.py:43): FactorResize's mode, which the reference hands to the datasets and to KBPNLoss's
        # Get_pseudo_lr alike; it exits on any other value.  JointModel and MODEL.SR="bicubic" models have no SR loss: the key has no effect
        # on them, as in the reference.  A ``sr_transforms`` that carries an ``interpolation`` (the reference's FactorResize under
        # csbsr_amd.dropin: the string 'area' or torchvision's BICUBIC enum) must say the same as the cfg key
        self.downscale = check_downscale(self.pc.downscale, "SOLVER.DOWNSCALE_INTERPOLATION", NotImplementedError)
        given = getattr(sr_transforms, "interpolation", None)
        if given is not None and str(getattr(given, "value", given)).lower() != self.downscale:
            raise ValueError(f"sr_transforms down-scales with {given!r} but SOLVER.DOWNSCALE_INTERPOLATION={self.downscale!r}: the loss "
                             "would not model the degradation the data was made with")
        self.scale_factor = cfg.MODEL.SCALE_FACTOR
        self.norm_method = cfg.SOLVER.NORM_SR_OUTPUT
        self.seg_model_name = None if self.sr_only else cfg.MODEL.DETECTOR_TYPE
        self.blur_skip = self.seg_model_name == "PSPNet_BlurSkip"
        # what the code below asks of these flags: is there a KBPN, is there a detector, does KBPN take gradients (BlurSkip freezes it)
        self._has_kbpn, self._has_detector = not self.bicubic, not self.sr_only
        self._kbpn_trains = self._has_kbpn and not self.blur_skip
        self._device = torch.device(device)
        shapes = joint_state_shapes(self.pc.scale, self.pc.num_stages, self.pc.ksize, self.pc.ksize_out, self.seg_model_name or "PSPNet",
                                    pixel_shuffle=self.pc.pixel_shuffle, kernel_sft=self.pc.kernel_sft, lr_error=self.pc.lr_error,
                                    zero_pad_kernel=self.pc.zero_pad_kernel)
        # registration order = reference state_dict order: segmentation_model.* then sr_model.*
        self.segmentation_model = _ParamGroup(shapes, "segmentation_model") if self._has_detector else None
        # (bicubic: the reference's ``sr_model`` is this string and its state_dict / parameters() hold the detector alone)
        self.sr_model = _ParamGroup(shapes, "sr_model") if self._has_kbpn else "bicubic"
        gen = torch.Generator().manual_seed(cfg.SEED if seed is None else seed)
        for full, t in self._named_full():
            if t.is_floating_point() and not full.endswith(("running_mean", "running_var")):
                _init_reference_style(full, t.data, gen)
        if self._has_kbpn and not cfg.MODEL.SR_SCRATCH:      # build_model.py:101-110; the detector's tensors keep the seeded init above
            self.pretrained_sr_path = load_pretrained_sr(self, cfg, pretrained_root)
        if self.blur_skip:        # build_model.py:352-368: everything but blur_skip.* is fixed
            for full, t in self._named_full():
                if isinstance(t, nn.Parameter):
                    t.requires_grad = ".blur_skip." in full
        self._rt = None
        # KBPN runs in micro-batches (exact: no batch-coupled op).  Larger ones amortise per-launch costs (B=8: 4.10 img/s at 1,
        # 4.24 at 2, 4.30 at 4, same peak memory); ``max_resident`` = how many micro-batches keep their activations for the backward
        # (26.5 GB per image at HR 1792^2), the others are recomputed there.  None = as many as the free HBM allows.
        self.micro_batch = 4
        self.max_resident = None
        self.lean_saves = None        # None: lean KBPN saves (KBPN.forward) only when that keeps more micro-batches resident; True / False force it
        self.dropout_enabled = True
        self.dropout_masks = None     # tests may inject {name: [B,C] fp32} keep-masks
        # Precision of the detector's FORWARD pass: "split" (default) runs activations and weights as fp16 hi + lo pairs, three MFMA passes
        # per conv into one fp32 accumulator; "fp16" is plain fp16 storage and one pass, the throughput configuration bench.py reports beside
        # the headline.  The backward is the same in both.
        self.detector_precision = "split"
        # ``detector_plan`` refines the split mode per layer: an ordered list of (regex on the conv's parameter name, K blocks) -- 3 = full
        # hi + lo product, 2 = hi + lo activation against the fp16 weight, 1 = plain fp16 operands (Conv.fwd_blocks); the first match wins and
        # unmatched layers run 3.  Two blocks go to BlurSkip's blur_skip layers and to PSPNet's decoder tail (up_1 .. final); every other
        # layer keeps three.  ``detector_hp_dgrad`` runs dgrads against [w_hi | w_lo]; it is off.  The sweeps behind each choice: DESIGN.md section 2.
        self.detector_plan = [(r"blur_skip\.[02]\.conv_(scale|shift)\.[01]\.|blur_skip\.[13]\.layer", 2)] if self.blur_skip else None
        if self.seg_model_name == "PSPNet" and os.environ.get("CSBSR_DEC_PLAN", "1") != "0":
            self.detector_plan = [(r"\.(up_[123]|final)\.", 2)]
        if os.environ.get("CSBSR_BS_PLAN") == "0":        # (A/B hook: three blocks everywhere)
            self.detector_plan = None
        self.detector_hp_dgrad = os.environ.get("CSBSR_HP_DGRAD") == "1"      # (A/B hook; default off)

    # ---- naming: state_dict keys are the reference's dotted names
    def _named_full(self):
        for grp, has in (("segmentation_model", self._has_detector), ("sr_model", self._has_kbpn)):
            for local, t in getattr(self, grp).named_local() if has else ():
                yield f"{grp}.{local}", t

    def state_dict(self, *a, **kw):
        return OrderedDict((k, v.detach() if isinstance(v, nn.Parameter) else v) for k, v in self._named_full())

    def load_state_dict(self, sd, strict=True):
        own = dict(self._named_full())
        missing = [k for k in own if k not in sd]
        unexpected = [k for k in sd if k not in own]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        with torch.no_grad():
            for k, v in sd.items():
                if k in own:
                    own[k].copy_(v)
        if self._rt is not None:
            self._invalidate()
            # slope probes of the weights just replaced are stale (the engine finds them by address, so the nn.Parameter names them)
            self._rt["eng"].new_step([own[k] for k in sd if k in own])
        return missing, unexpected

    # ---- runtime (engine + layer objects) is built lazily on the device
    def _runtime(self):
        if self._rt is None:
            if not torch.cuda.is_available():
                raise L.CsbsrHipError("csbsr_amd needs an MI355X (no CPU fallback)")
            self.to(self._device)
            eng = Engine(self._device)
            P = {k: (v.data if isinstance(v, nn.Parameter) else v) for k, v in self._named_full()}
            psp = None if not self._has_detector else HRNetOCR(eng, P) if self.seg_model_name == "HRNet_OCR" else \
                PSPNet(eng, P, blur_dim=self.pc.ksize_out ** 2 if self.blur_skip else None)
            self._rt = {"eng": eng, "P": P, "kbpn": KBPN(eng, P, self.pc) if self._has_kbpn else None, "psp": psp}
            self._make_grad_buckets()
        if self._rt["psp"] is None:        # SR-only: no detector, so no detector precision plan to apply
            return self._rt
        if self.detector_precision not in ("fp16", "split"):
            raise ValueError(f"detector_precision must be 'fp16' or 'split', got {self.detector_precision!r}")
        split = self.detector_precision == "split"
        self._rt["psp"].split = split
        plan = [(re.compile(pat), int(nb)) for pat, nb in (self.detector_plan or ())]
        for c in self._rt["psp"].all_convs():      # the split mode's dgrads run against fp16 hi + lo weight pairs (Conv.bwd_input)
            c.hp_dgrad = split and bool(self.detector_hp_dgrad)
            c.fwd_blocks = next((nb for pat, nb in plan if pat.search(c.name)), 3)
            c.dc_comp = c.fwd_blocks < 3          # a layer that keeps its weights' fp16 rounding gets the mean compensation (Conv._dc_bias)
        return self._rt

    def _bucket_of(self, name):
        """gradient bucket of a parameter: the order buckets complete in the explicit backward (segmentation net, then KBPN stages
        S .. 1 -- output_conv goes with stage S --, then the predictor + VGG head)."""
        if name.startswith("segmentation_model"):
            return "seg"
        S = self.pc.num_stages
        if name.startswith("sr_model.back_projection_stages."):
            return f"kbpn.{int(name.split('.')[2]) + 1}"
        if name.startswith("sr_model.output_conv"):
            return f"kbpn.{S}"
        return "kbpn.0"

    def _make_grad_buckets(self):
        """One flat fp32 buffer per bucket; every trainable parameter's accumulator (``gacc``, written by the kernels) is a view of
        it, so a bucket is zeroed / all-reduced / scaled as ONE tensor."""
        rt = self._rt
        sizes = {}
        for k, v in self._named_full():
            if isinstance(v, nn.Parameter) and v.requires_grad:
                sizes[self._bucket_of(k)] = sizes.get(self._bucket_of(k), 0) + v.numel()
        flats = {b: torch.zeros(n, dtype=torch.float32, device=self._device) for b, n in sizes.items()}
        off = {b: 0 for b in sizes}
        for k, v in self._named_full():
            if isinstance(v, nn.Parameter) and v.requires_grad:
                b, t = self._bucket_of(k), rt["P"][k]
                t.gacc = flats[b][off[b]:off[b] + v.numel()].view(t.shape)
                t.gacc_touched = False
                off[b] += v.numel()
        rt["flat"] = flats
        rt["pnames"] = [k for k, v in self._named_full() if isinstance(v, nn.Parameter)]     # == self.parameters() order

    def _invalidate(self):
        rt = self._rt
        if rt["kbpn"] is not None:
            rt["kbpn"].invalidate()
        if rt["psp"] is not None:
            rt["psp"].invalidate()
        rt["eng"].new_step()            # (master weights may have been stepped: every PReLU slope probe may issue one new asynchronous read)

    # ---- shared forward pieces
    def _mount(self, t):
        return None if t is None else t.to(self._device, torch.float32).contiguous()

    def _begin(self, *tensors):
        """The start of every forward: KBPN's mode flags where there is a KBPN, a new engine step (the optimiser may have stepped the master
        weights) and the batch on the device as contiguous fp32."""
        kbpn = self._runtime()["kbpn"]
        if kbpn is not None:
            kbpn.training_mode, kbpn.pad_dropout = self.training, self.dropout_enabled and self.dropout_masks is None
        self._invalidate()
        return [self._mount(t) for t in tensors]

    def _instnorm_stats(self, sr32):
        eng = self._rt["eng"]
        B, Cc, H, W = sr32.shape
        red = eng.f32(B * Cc, 2)
        L.call("csbsr_plane_reduce", _ptr(sr32), None, B * Cc, H * W, _ptr(red), eng.stream)
        mean = red[:, 0] / (H * W)
        var = (red[:, 1] / (H * W) - mean * mean).clamp_min(0)
        return mean.contiguous(), torch.rsqrt(var + 1e-5).contiguous()

    def _norm_sr(self, sr32):
        """build_model.py:125-141 -> FM fp16 NHWC8 for the segmentation net, plus what the backward needs."""
        eng = self._rt["eng"]
        B = sr32.shape[0]
        if self.norm_method == "instance":
            mean, invstd = self._instnorm_stats(sr32)
        elif self.norm_method == "all":
            mean = torch.tensor(self.pc.mean, device=self._device).repeat(B).contiguous()
            invstd = (1.0 / torch.tensor(self.pc.std, device=self._device)).repeat(B).contiguous()
        else:
            mean = invstd = None
        return eng.nchw32_to_fm(sr32, mean=mean, invstd=invstd, split=self.detector_precision == "split"), mean, invstd

    def _bicubic_up(self, x, clip):
        """MODEL.SR="bicubic": transforms.Resize(size * scale, BICUBIC) of the LR batch (build_model.py:69-73), clipped to [0, 1] in the
        same pass when asked (clip_sr)."""
        eng, pc = self._rt["eng"], self.pc
        B, Cc, h, w = x.shape
        sr32 = eng.f32(B, Cc, h * pc.scale, w * pc.scale, zero=False)
        L.call("csbsr_aa_bicubic_up", _ptr(x), _ptr(sr32), B * Cc, h, w, pc.scale, int(pc.antialias), int(bool(clip)), eng.stream)
        return sr32


class _StepFn(torch.autograd.Function):
    """(segment_loss[B], sr_loss[B]) = f(parameters), either of them None in a model that does not have it; backward = the HIP backward pass."""

    @staticmethod
    def forward(ctx, model, st, seg_loss, sr_loss, *params):
        ctx.model, ctx.st = model, st          # the saved state travels with THIS graph: a later forward cannot clobber it
        ctx.set_materialize_grads(False)       # an unused loss vector arrives as None, not as a zero tensor to be scanned
        return tuple(None if v is None else v.clone() for v in (seg_loss, sr_loss))

    @staticmethod
    def backward(ctx, dseg, dsr):
        st, ctx.st = ctx.st, None
        if st is None:
            raise RuntimeError("csbsr_amd: backward called twice on the same forward (activations are freed by the first backward)")
        grads = tuple(ctx.model._hip_backward(st, dseg, dsr))
        return (None,) * (len(ctx.needs_input_grad) - len(grads)) + grads


class _TrainBase(_JointBase):
    """What JointModelWithLoss and SRModelWithLoss share: the KBPN forward in micro-batches with its residency budget, KBPNLoss, the SR
    gradient seed, the KBPN backward schedule and the end of a backward (exchange, overflow skip, un-scaling)."""

    def _init_loss_scale(self):
        self.grad_scale = None          # None: chosen per call as 2^round(log2(B*H*W)) (see _begin_backward)
        self.scale_backoff = 0          # log2 reduction of the automatic scale after overflowed steps
        self.overflow_steps = 0
        self.last_step_overflowed = False
        self.reducer = None             # csbsr_amd.parallel.GradBucketReducer when data-parallel

    def _kbpn_forward(self, iter, x, kgt):
        """KBPN over the mounted batch in micro-batches -> (sr32 [B,3,H,W], kvec [B,kk], saves, micro-batch): the first ``n_res``
        micro-batches keep their activations for the backward (``saves[i]``), the others are recomputed there."""
        eng, kbpn, pc = self._rt["eng"], self._rt["kbpn"], self.pc
        B, _, h, w = x.shape
        H, W = h * pc.scale, w * pc.scale
        mb = max(1, min(self.micro_batch, B))
        keep = self.training and torch.is_grad_enabled()
        # (the rank agreement inside _auto_resident is a collective: only a forward that will be followed by a backward takes part in it, so
        # a rank-0-only validation pass, an evaluator sharing the model or a no_grad call can never leave the other ranks waiting)
        n_res, lean = (self.max_resident, bool(self.lean_saves)) if self.max_resident is not None else self._auto_resident(B, mb, H, W, agree=keep)
        if self.max_resident is None and keep and n_res == 0 and mb >= B and B >= 2 and self._kbpn_trains:
            # the whole batch as ONE micro-batch is all-or-nothing: when it does not fit (RCCL buffers, another tenant, fragmentation)
            # halve the micro-batch so that part of the batch stays resident instead of recomputing every KBPN forward in the backward.
            # n_res is the agreed minimum over the ranks, so every rank takes this branch (and its second agreement) together
            mb2 = (B + 1) // 2
            n2, lean2 = self._auto_resident(B, mb2, H, W, agree=keep)
            if n2 > 0:
                mb, n_res, lean = mb2, n2, lean2
        self._n_res, self._lean, self._mb_used = n_res, lean, mb
        sr32 = eng.f32(B, 3, H, W, zero=False)
        kvec = eng.f32(B, pc.ksize_out ** 2, zero=False)
        saves, self._pad_takes = [], []
        for i, b0 in enumerate(range(0, B, mb)):
            resident = keep and i < n_res and self._kbpn_trains      # BlurSkip: KBPN is frozen, no backward through it
            s_, k_ = kbpn.forward(x[b0:b0 + mb], iter, kgt[b0:b0 + mb], save=resident, lean=lean)
            saves.append(kbpn.saved if resident else None)
            self._pad_takes.append(kbpn.pad_taken)        # ZERO_PAD_KERNEL: a recomputed forward replays these (KBPN.forward)
            kbpn.saved = None
            sr32[b0:b0 + mb] = s_
            kvec[b0:b0 + mb] = k_
        return sr32, kvec, saves, mb

    def _sr_loss_terms(self, iter, x, hr, kgt, sr32, kvec, seg32, mask):
        """KBPNLoss (sr_loss_functions.py:35-66), forward sums only -> (sr_loss [B], kernel_preds [B,1,K,K], what _sr_loss_seed needs).
        ``seg32`` / ``mask`` feed the oriented weight map alone; the SR-only model has neither and refuses the keys that would ask for it.
        The pseudo-LR image is the blurred SR image down-scaled as ``pc.downscale`` says (Get_pseudo_lr, sr_loss_functions.py:94): the
        antialiased bicubic resize or, with "area", the f x f box mean -- ``antialias`` has no meaning then."""
        eng, pc = self._rt["eng"], self.pc
        B, _, h, w = x.shape
        H, W = h * pc.scale, w * pc.scale
        hw = H * W
        # KBPNLoss: L1(sr, hr), L1(down(blur(sr)), x), MSE(kernel) * 0
        ksum = kvec.sum(1, keepdim=True)
        vec = (kvec / ksum).contiguous()
        K = pc.ksize_out
        oriented = iter > pc.oriented_w_iter and pc.oriented_w_iter != -1
        wmap = None
        if oriented and pc.sfo_sr_amp != 0:
            wmap = torch.exp(pc.sfo_sr_amp * (seg32 - mask).abs()).contiguous()      # oriented_weight.py:73-83 (detached)
        wmap_lr = None
        if wmap is not None:
            wmap_lr = eng.f32(B, 1, h, w, zero=False)
            L.call("csbsr_bilinear32_fwd", _ptr(wmap), _ptr(wmap_lr), B, H, W, h, w, 0, eng.stream)
        if oriented and pc.co_sr_amp != 0:
            wmap, wmap_lr = self._crack_weight(mask, wmap, wmap_lr)
        blurred = eng.f32(B, 3, H, W, zero=False)
        L.call("csbsr_blur_fwd", _ptr(sr32), _ptr(vec), B, 3, H, W, K, 1, None, _ptr(blurred), None, 0, eng.stream)
        lr_pred = eng.f32(B, 3, h, w, zero=False)
        if pc.downscale == "area":
            L.call("csbsr_area_down_fwd", _ptr(blurred), _ptr(lr_pred), B * 3, H, W, pc.scale, eng.stream)
        else:
            L.call("csbsr_aa_bicubic_down_fwd", _ptr(blurred), _ptr(lr_pred), B * 3, H, W, pc.scale, int(pc.antialias), eng.stream)
        s_hr, s_lr = eng.f32(B), eng.f32(B)
        L.call("csbsr_l1_fwd_bwd", _ptr(sr32), _ptr(hr), _ptr(wmap), B, 3, hw, _ptr(s_hr), 0.0, None, None, 0, eng.stream)
        L.call("csbsr_l1_fwd_bwd", _ptr(lr_pred), _ptr(x), _ptr(wmap_lr), B, 3, h * w, _ptr(s_lr), 0.0, None, None, 0, eng.stream)
        kpred = vec.reshape(B, 1, K, K)
        k_l = ((kpred - kgt) ** 2).mean((1, 2, 3))
        # SOLVER.ONLY_KERNEL_LOSS_FOR_PRETRAIN (sr_loss_functions.py:50-51): during the kernel-module pretraining phase the SR loss IS the
        # kernel MSE (the reference returns the unreduced [B,1,K,K] map there and calc_loss takes its mean: the per-sample mean has the same mean)
        sr_w = (0.0, 0.0, 1.0) if (pc.only_kernel_loss and pc.kernel_pretrain[0] <= iter < pc.kernel_pretrain[1]) else pc.sr_w
        sr_loss = sr_w[0] * s_hr / (3 * hw) + sr_w[1] * s_lr / (3 * h * w) + sr_w[2] * k_l
        del blurred
        return sr_loss, kpred, dict(ksum=ksum, vec=vec, lr_pred=lr_pred, wmap=wmap, wmap_lr=wmap_lr, sr_w=sr_w)

    def _crack_weight(self, mask, wf, wf_lr):
        """SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP: the crack-oriented weight w^C = 2 exp(-amp d) of the whole batch (CrackOrientedExpWeight,
        oriented_weight.py:46-58,92-119; d = distance to the nearest crack pixel, a pixel being a crack where the mask truncated to uint8
        is non-zero; 2 everywhere for a sample without one) and its bilinear LR reduction -> (HR weight, LR weight) of the two L1 terms,
        times the fail-oriented pair ``wf`` / ``wf_lr`` where that is on: KBPNLoss.multiple_weight's order, the LR weight being the product
        of the two reduced maps.  Constants of the backward.  lambda is the class default 2; the reference's constructor also reads
        CRACK_ORIENTED_WEIGHT4SR_BIAS and never uses it, so this build has no such key."""
        eng, pc = self._rt["eng"], self.pc
        B, _, H, W = mask.shape
        wc, wc_lr = eng.f32(B, 1, H, W, zero=False), eng.f32(B, 1, H // pc.scale, W // pc.scale, zero=False)
        scratch = eng.f32(B * H * W, zero=False)
        L.call("csbsr_crack_weight", _ptr(mask), _ptr(wc), _ptr(wc_lr), _ptr(scratch), B, H, W, pc.co_sr_amp, 2.0, pc.scale, eng.stream)
        del scratch
        return (wc, wc_lr) if wf is None else (wc * wf, wc_lr * wf_lr)

    def _auto_resident(self, B, mb, H, W, agree=True):
        """micro-batches whose KBPN activations fit next to the detector's working set -- the SR-only model has none, so its budget has
        no detector term -- (measured at HR 1792^2: 26.5 GB per image of KBPN activations, 6.3 / 9.5 GB per image for PSPNet / HRNet-OCR incl. their backward workspaces -- the split-precision
        detector holds two planes per activation) with 18 GB to spare.  The budget is what is FREE now (driver-reported free memory
        plus what torch's caching allocator holds but does not use), so another tenant of the GPU or a second model in the process
        lowers the residency instead of running the step out of memory; the rest is recomputed in the backward."""
        r = (H * W) / float(1792 * 1792)
        free, _ = torch.cuda.mem_get_info(self._device)
        free += torch.cuda.memory_reserved(self._device) - torch.cuda.memory_allocated(self._device)
        det = 0.0               # no detector: its working set is KBPN's to keep
        if self._has_detector:
            det = (9.5e9 if self.seg_model_name == "HRNet_OCR" else 6.3e9) * r * B
            if self.detector_precision == "split":
                det += 4.9e9 * r * B
        n_mb = (B + mb - 1) // mb

        def fit(per_img):
            imgs = int((free - 18e9 - det) // (per_img * r)) if r > 0 else B
            return max(0, min(n_mb, imgs // mb))
        full, lean = fit(26.5e9), fit(21.2e9)      # lean saves: the kernel predictors' fe_SR chains are rebuilt in the backward (KBPN.forward)
        if agree and self.reducer is not None and self.reducer.active:
            # data-parallel: the ranks must take the SAME schedule (at ~240 of 288 GB the collective library's buffers can tip one rank into
            # recomputing a KBPN forward, and every other rank would wait for it at the all-reduce): the minimum over the ranks, agreed
            # in one tiny collective per problem shape.  EVERY rank must present each training shape (B, micro-batch, H, W) -- the
            # data-parallel contract anyway: equal shards, train.py:105-112 of the reference -- and only training forwards with autograd
            # on take part (``agree``); eval / no_grad forwards keep nothing resident and use the local figures.  The agreement is kept
            # for the life of the model: renewing it when ONE rank's free memory drops later would be a collective only that rank enters
            key = (B, mb, H, W, self.detector_precision)
            agreed = self.__dict__.setdefault("_sched_agreed", {})
            if key not in agreed:
                agreed[key] = self.reducer.agree_min([full, lean])
            full, lean = agreed[key]
        if self.lean_saves is not None:
            return (lean, True) if self.lean_saves else (full, False)
        return (lean, True) if lean > full else (full, False)

    def _saved_state(self, iter, x, det=None, hr=None, kgt=None, sr32=None, kvec=None, saves=None, mb=None, terms=None):
        """What one backward needs, carried by its autograd node: the detector's part (``det``, _detector_and_losses) where there is a
        detector and, with ``terms`` (_sr_loss_terms), the SR half's -- what _sr_loss_seed and the KBPN schedule read.  ``saves`` None:
        the graph ends at a given SR image (forward_from_sr)."""
        B, _, h, w = x.shape
        st = dict(iter=iter, B=B, h=h, w=w, saves=saves, **(det or {}))
        if terms is not None:
            st.update(x=x, hr=hr, kgt=kgt, sr32=sr32, kvec=kvec, mb=mb, n_res=self._n_res,
                      pad_takes=self._pad_takes if saves is not None else None, **terms)
        return st

    def _begin_backward(self, npix, backoff=True):
        """The start of every backward -> (loss scale, parameter names in ``parameters()`` order): sets the engine's scale and hands the
        kernels fresh fp32 accumulators.

        The loss scale of the fp16 activation gradients: the per-pixel loss gradient is O(1/(B*H*W)), ``npix``; PSPNet keeps that magnitude
        down to the input, HRNet-OCR grows it ~1e5x towards the stem (measured, reference-style init), so it starts 2^8 lower.
        ``scale_backoff`` is the dynamic part (GradScaler semantics): a backward that overflowed returns no gradients for that step and
        lowers the scale for the following ones.  ``grad_scale`` overrides all of it.  ``backoff=False`` (kbpn_backward_from, whose
        upstream gradient is given) is 2^round(log2(npix)) whatever the model's state."""
        rt = self._rt
        e = round(math.log2(npix))
        gs = float(2 ** e) if not backoff else \
            self.grad_scale or float(2 ** (e - (8 if self.seg_model_name == "HRNet_OCR" else 0) - self.scale_backoff))
        rt["eng"].grad_scale = gs
        for k in rt["pnames"]:
            rt["P"][k].gacc_touched = False
        torch._foreach_zero_(list(rt["flat"].values()))      # the accumulators are views of a handful of flat buckets
        return gs, rt["pnames"]

    def _hip_backward(self, st, dseg_loss, dsr_loss):
        """The backward of every model: the detector half where there is a detector and the caller's scalar used the segmentation loss,
        then the KBPN half where KBPN takes gradients and the graph did not end at a given SR image."""
        rt, pc = self._rt, self.pc
        eng, psp = rt["eng"], rt["psp"]
        B, h, w = st["B"], st["h"], st["w"]
        H, W = h * pc.scale, w * pc.scale
        hw = H * W
        gs, pnames = self._begin_backward(B * hw)
        dsr32 = eng.f32(B, 3, H, W) if self._has_kbpn else None      # (bicubic: the input is no function of a parameter)
        # which halves of the backward run follows from which loss vector the caller's scalar loss used (autograd hands None for an
        # unused output): a function of the training phase, identical on every rank, and no device read-back
        seg_active = self._has_detector and dseg_loss is not None
        if self._has_detector:
            # the node's reference ends here: the detector's backward consumes the tape entry by entry, and an iteration without a
            # segmentation loss (SR pretraining phase) frees all of it before the KBPN backward
            tape = st.pop("psp_saved")
            psp.saved = tape if seg_active else None
            del tape
        if seg_active:
            gsc = (dseg_loss.to(torch.float32) * gs).contiguous()
            dseg32, daux32 = eng.f32(B, 1, H, W, zero=False), eng.f32(B, 1, H, W, zero=False)
            pw, lw = pc.bce_w, pc.wbd_w
            for p_, sums, wgt, dp in ((st["seg32"], st["sums_m"], self.main_weight, dseg32), (st["aux32"], st["sums_a"], self.aux_weight, daux32)):
                L.call("csbsr_segloss_finish", _ptr(p_), _ptr(st["mask"]), _ptr(st["sdf"]), B, hw, _ptr(sums), st["alpha"], pw[0], pw[1],
                       lw[0], lw[1], wgt, _ptr(gsc), None, _ptr(dp), 0, eng.stream)
            dxin = psp.backward(dseg32, daux32, need_dxin=self._has_kbpn)      # (bicubic: no first-conv input gradient)
            eng.join_wgrad()                    # the detector's weight gradients (side stream) are complete
            if not self._kbpn_trains:           # bicubic, or BlurSkip where only blur_skip.* trains: no gradient leaves the segmentation net
                return self._finish_backward(pnames, gs, ("segmentation_model",), st)
            if self.reducer is not None:        # segmentation gradients are final: exchange them under the KBPN backward
                self.reducer.launch_flat(rt["flat"].get("seg"))
                st["seg_launched"] = True
            if st["mean"] is not None and self.norm_method == "instance":
                red = eng.f32(B * 3, 2)
                L.call("csbsr_instnorm_bwd", _ptr(dxin.t), dxin.ld, _ptr(st["sr32"]), _ptr(st["mean"]), _ptr(st["invstd"]), _ptr(dsr32), 0,
                       B, 3, hw, _ptr(red), eng.stream)
            else:
                eng.fm_to_nchw32(dxin, dsr32, 3)
                if st["invstd"] is not None:
                    dsr32 *= st["invstd"].reshape(B, 3, 1, 1)
            del dxin, dseg32, daux32
        elif not self._kbpn_trains:
            return self._finish_backward(pnames, gs, (), st)
        dkvec = self._sr_loss_seed(st, dsr_loss, gs, dsr32)
        if st["saves"] is None:        # forward_from_sr: the graph ends at the given SR image
            self.last_dsr, self.last_dkvec = dsr32 / gs, dkvec / gs
            return self._finish_backward(pnames, gs, ("segmentation_model",) if seg_active else (), st)
        # ---- KBPN backward (per micro-batch; recompute the forward when it was not kept)
        st["kbpn_launched"] = self._kbpn_backward_schedule(st, dsr32, dkvec)
        return self._finish_backward(pnames, gs, ("sr_model",), st)

    def _sr_loss_seed(self, st, dsr_loss, gs, dsr32):
        """Seeds of the KBPN backward from the SR loss: adds dLoss/d sr_preds (x ``gs``) into ``dsr32`` and returns dLoss/d kernel vector
        [B,kk] (zeros when the caller's scalar did not use the SR loss).  The LR term goes back through the adjoint of the down-scale
        ``pc.downscale`` names; with "area" that is dy / f^2 replicated and ``antialias`` has no meaning."""
        eng, pc = self._rt["eng"], self.pc
        B, h, w = st["B"], st["h"], st["w"]
        H, W = h * pc.scale, w * pc.scale
        hw = H * W
        dkvec = eng.f32(B, pc.ksize_out ** 2)
        if dsr_loss is not None:
            g = (dsr_loss.to(torch.float32) * gs)
            K = pc.ksize_out
            sr_w = st["sr_w"]
            g_hr = (g * sr_w[0] / (3 * hw)).contiguous()
            g_lr = (g * sr_w[1] / (3 * h * w)).contiguous()
            L.call("csbsr_l1_fwd_bwd", _ptr(st["sr32"]), _ptr(st["hr"]), _ptr(st["wmap"]), B, 3, hw, None, 1.0, _ptr(g_hr), _ptr(dsr32), 1,
                   eng.stream)
            dlr = eng.f32(B, 3, h, w, zero=False)
            L.call("csbsr_l1_fwd_bwd", _ptr(st["lr_pred"]), _ptr(st["x"]), _ptr(st["wmap_lr"]), B, 3, h * w, None, 1.0, _ptr(g_lr), _ptr(dlr), 0,
                   eng.stream)
            dbl = eng.f32(B, 3, H, W, zero=False)
            if pc.downscale == "area":
                L.call("csbsr_area_down_bwd", _ptr(dlr), _ptr(dbl), 0, B * 3, H, W, pc.scale, eng.stream)
            else:
                L.call("csbsr_aa_bicubic_down_bwd", _ptr(dlr), _ptr(dbl), 0, B * 3, H, W, pc.scale, int(pc.antialias), eng.stream)
            L.call("csbsr_blur_bwd_input", _ptr(dbl), _ptr(st["vec"]), _ptr(dsr32), 1, B, 3, H, W, K, 1, eng.stream)
            dvec = eng.f32(B, K * K)
            L.call("csbsr_blur_bwd_kernel", _ptr(dbl), _ptr(st["sr32"]), _ptr(dvec), B, 3, H, W, K, 1, eng.stream)
            if sr_w[2] != 0:
                dvec += (g * sr_w[2] / (K * K)).reshape(B, 1) * 2 * (st["vec"] - st["kgt"].reshape(B, -1))
            dkvec = (dvec - (dvec * st["vec"]).sum(1, keepdim=True)) / st["ksum"]
            del dbl, dlr
        return dkvec

    def _kbpn_backward_schedule(self, st, dsr32, dkvec):
        """KBPN backward per micro-batch with the upstream gradients ``dsr32`` / ``dkvec`` (x loss scale); returns the buckets whose
        exchange was launched under it (data-parallel)."""
        rt = self._rt
        kbpn = rt["kbpn"]
        B, mb, saves = st["B"], st["mb"], st["saves"]
        order = list(enumerate(range(0, B, mb)))
        # resident micro-batches last-in first-out (frees HBM before the recomputed ones run), then the rest with their forward
        # recomputed here (KBPN has no batch-coupled op: exact)
        sched = [(i, b0, False) for i, b0 in reversed(order) if saves[i] is not None] + [(i, b0, True) for i, b0 in order if i >= st["n_res"]]
        launched = set()

        def stage_done(s):      # last micro-batch only: stage s's parameter gradients are final -> exchange them under the rest
            if self.reducer is not None:
                self.reducer.launch_flat(rt["flat"].get(f"kbpn.{s}"))
                launched.add(f"kbpn.{s}")
        for j, (i, b0, recompute) in enumerate(sched):
            if recompute:
                kbpn.forward(st["x"][b0:b0 + mb], st["iter"], st["kgt"][b0:b0 + mb], save=True,
                             pad_replay=st["pad_takes"][i] if kbpn.zero_pad else None)
            else:
                kbpn.saved, saves[i] = saves[i], None
            kbpn.backward(dsr32[b0:b0 + mb].contiguous(), dkvec[b0:b0 + mb].contiguous(),
                          stage_done=stage_done if j == len(sched) - 1 else None)
        return launched

    def _finish_backward(self, pnames, gs, reduce_groups, st):
        rt = self._rt
        rt["eng"].join_wgrad()
        if self.reducer is not None:
            # whatever this phase's backward wrote and has not been launched yet (every rank takes the same branch: the set of
            # buckets depends on the training phase only)
            for b, flat in rt["flat"].items():
                grp = "segmentation_model" if b == "seg" else "sr_model"
                if grp in reduce_groups and not (b == "seg" and st.get("seg_launched")) and b not in st.get("kbpn_launched", ()):
                    self.reducer.launch_flat(flat)
            self.reducer.finish()
        inv = 1.0 / gs
        # overflow check on the (already all-reduced, so rank-consistent) accumulators: one scalar read back per step
        finite = bool(torch.isfinite(torch.stack(torch._foreach_norm(list(rt["flat"].values()))).sum()))
        if not finite:
            self.overflow_steps += 1
            if self.grad_scale is None:
                self.scale_backoff += 4
            warnings.warn(f"csbsr_amd: fp16 gradient overflow at loss scale {gs:g}; this step is skipped (every gradient is None)"
                          + ("" if self.grad_scale is not None else f", next scale {gs / 16:g}"))
            self.last_step_overflowed = True
            # GradScaler semantics: optimizer.step() must be a no-op for this step.  Gradients of None make torch optimisers skip the
            # parameter entirely (no moment decay, no step count, no weight move); zeros would still move Adam's weights by its momentum.
            return [None] * len(pnames)
        self.last_step_overflowed = False
        # parameters no kernel touched (frozen phase / unused) keep grad None; the others leave as accumulator x 1 / scale -- one multi-tensor
        # launch set instead of one launch per parameter (290 with PSPNet, 1109 with HRNet-OCR; same fp32 products)
        out = [None] * len(pnames)
        idx = [i for i, k in enumerate(pnames) if getattr(rt["P"][k], "gacc_touched", False)]
        if idx:
            for i, g in zip(idx, torch._foreach_mul([rt["P"][pnames[i]].gacc for i in idx], inv)):
                out[i] = g
        return out


class JointModelWithLoss(_TrainBase):
    def __init__(self, cfg, num_train_ds, resume_iter, sr_transforms=None, antialias=True, device="cuda:0", seed=None, pretrained_root="weights"):
        super().__init__(cfg, antialias, device, seed, pretrained_root, sr_transforms=sr_transforms)
        # bicubic: calc_sr_loss returns None before it looks at the loss function (build_model.py:163-166), so the keys that only shape
        # KBPN or the SR loss have no effect, as in the reference (the list: DESIGN.md section 1.5); _JointBase's refusals of values no model
        # of this build takes (SUM_LR_ERROR_POS, NUM_CLASSES, SR_SEG_INV, JOINT_LEARNING) hold for this model too
        if cfg.SOLVER.SEG_LOSS_FUNC != "BoundaryCombo" or (cfg.SOLVER.SR_LOSS_FUNC != "KBPN" and not self.bicubic):
            raise NotImplementedError("csbsr_amd builds SEG_LOSS_FUNC=BoundaryCombo with SR_LOSS_FUNC=KBPN")
        if cfg.SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SS_AMP != 0 or cfg.SOLVER.INTERM_SSLOSSWEGHT4SR:
            raise NotImplementedError("oriented loss weights other than SEG_FAIL_ORIENTED_WEIGHT4SR and CRACK_ORIENTED_WEIGHT4SR are not built")
        if cfg.SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP != 0 and cfg.SOLVER.ORIENTED_WEIGHT_ITER == -1:
            raise NotImplementedError("SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP with ORIENTED_WEIGHT_ITER = -1: KBPNLoss applies no oriented weight "
                                      "then, so the key could never act, and this build keeps refusing the combination (tests/test_host_cpu.py pins "
                                      "it); set ORIENTED_WEIGHT_ITER to the iteration after which the weight applies")
        seg_rsm = resume_iter - (cfg.SOLVER.SR_PRETRAIN_ITER[1] - 1) if resume_iter > (cfg.SOLVER.SR_PRETRAIN_ITER[1] - 1) else 0
        per_epoch = num_train_ds // cfg.SOLVER.BATCH_SIZE + 1
        self.ss_loss_fn = BoundaryComboState(per_epoch, seg_rsm, decrease_ratio=cfg.SOLVER.BOUNDARY_DEC_RATIO)
        self.sr_loss_fn = "KBPNLoss"
        self.aux_weight, self.main_weight = cfg.SOLVER.SEG_AUX_LOSS_WEIGHT, cfg.SOLVER.SEG_MAIN_LOSS_WEIGHT
        self.iter_cnt = True
        self._init_loss_scale()
        self.last_dsr = self.last_dkvec = None      # set by the backward of forward_from_sr (validation)

    # ------------------------------------------------------------------ forward
    def forward(self, iter, x, sr_targets=None, segment_targets=None, kernel_targets=None, segment_sdf=None):
        """``segment_sdf`` (optional, not in the reference's signature): the signed distance map of ``segment_targets`` already on the
        device -- csbsr_amd.data.degrade.DeviceDegradation computes it with the batch -- so the loss does not recompute it."""
        x, hr, mask, kgt, sdf = self._begin(x, sr_targets if self._has_kbpn else None, segment_targets, kernel_targets, segment_sdf)
        if self._has_kbpn:
            sr32, kvec, saves, mb = self._kbpn_forward(iter, x, kgt)
        else:
            # forward_sr's bicubic branch: sr_preds is the UNCLIPPED up-scaled input, kernel_preds zeros of the target's shape, sr_loss None;
            # the detector and its loss are the kernels of the joint model's detector half on the same bytes
            self._n_res = 0
            sr32, kvec, saves, mb = self._bicubic_up(x, clip=False), None, None, x.shape[0]
        return self._detector_and_losses(iter, x, hr, mask, kgt, sr32, kvec, saves, mb, sdf=sdf)

    def forward_from_sr(self, iter, sr_preds, kernel_vec, x, sr_targets, segment_targets, kernel_targets):
        """Validation entry point: the detector + loss half of ``forward`` fed a GIVEN SR image [B,3,H,W] and (un-normalised) kernel
        vector [B,kk] instead of KBPN's -- e.g. the reference's own sr_preds from a golden fixture -- so the detector, the losses
        and their backward can be compared with the reference on identical inputs.  ``backward()`` on the returned losses stops at
        the SR image: its gradient (true scale) is left in ``self.last_dsr`` / ``self.last_dkvec``; KBPN parameters get no gradient."""
        if self.bicubic:
            raise NotImplementedError("forward_from_sr / kbpn_backward_from are entry points of the KBPN model; MODEL.SR='bicubic' has no SR loss")
        x, hr, mask, kgt, sr32, kvec = self._begin(x, sr_targets, segment_targets, kernel_targets, sr_preds, kernel_vec)
        self._n_res = 0
        return self._detector_and_losses(iter, x, hr, mask, kgt, sr32, kvec.reshape(x.shape[0], -1), None, x.shape[0])

    @torch.no_grad()
    def kbpn_backward_from(self, iter, x, kernel_targets, dsr, dkvec):
        """Validation entry point: KBPN forward + backward with a GIVEN upstream gradient (dLoss/d sr_preds [B,3,H,W] and
        dLoss/d kernel vector [B,kk], true scale) -- e.g. the reference's own, from a golden fixture.  Returns {state_dict name: grad}."""
        if self.bicubic:
            raise NotImplementedError("forward_from_sr / kbpn_backward_from are entry points of the KBPN model; MODEL.SR='bicubic' has no KBPN")
        x, kgt, dsr, dkvec = self._begin(x, kernel_targets, dsr, dkvec)
        rt, pc = self._rt, self.pc
        eng, kbpn = rt["eng"], rt["kbpn"]
        B, _, h, w = x.shape
        gs, pnames = self._begin_backward(B * h * w * pc.scale * pc.scale, backoff=False)
        names = [k for k in pnames if k.startswith("sr_model")]
        mb = max(1, min(self.micro_batch, B))
        for b0 in range(0, B, mb):
            kbpn.forward(x[b0:b0 + mb], iter, kgt[b0:b0 + mb], save=True)
            kbpn.backward((dsr[b0:b0 + mb] * gs).contiguous(), (dkvec[b0:b0 + mb] * gs).contiguous())
        eng.join_wgrad()
        return {k: (rt["P"][k].gacc / gs if getattr(rt["P"][k], "gacc_touched", False) else None) for k in names}

    def _detector_and_losses(self, iter, x, hr, mask, kgt, sr32, kvec, saves, mb, sdf=None):
        rt, pc = self._rt, self.pc
        eng, psp = rt["eng"], rt["psp"]
        B, _, h, w = x.shape
        H, W = h * pc.scale, w * pc.scale
        training = self.training
        xin, mean, invstd = self._norm_sr(sr32)
        drop = psp.make_dropout(B, training, self.dropout_enabled) if self.dropout_masks is None else \
            {k: self.dropout_masks.get(k) for k in psp.drop_keys}
        drop = {k: (None if v is None else v.to(self._device, torch.float32).contiguous()) for k, v in drop.items()}
        seg32, aux32 = psp.forward(xin, drop, training, kvec=kvec if self.blur_skip else None)
        keep = training and torch.is_grad_enabled()
        # the detector's tape (None unless ``keep``: the forward writes none otherwise) is carried by the autograd node, not by the (shared)
        # detector object: nothing a backward reads stays on a layer
        psp_saved, psp.saved = psp.saved, None
        # ---- losses (forward sums only; gradients are produced in _hip_backward)
        hw = H * W
        if sdf is None:
            sdf = eng.f32(B, 1, H, W, zero=False)
            scratch = eng.f32(3 * B * hw + 2 * B, zero=False)
            L.call("csbsr_sdf", _ptr(mask), _ptr(sdf), _ptr(scratch), B, H, W, eng.stream)
            del scratch
        alpha = float(self.ss_loss_fn.alpha)
        seg_loss = eng.f32(B)
        sums_m, sums_a = eng.f32(B, 8), eng.f32(B, 8)
        pw, lw = pc.bce_w, pc.wbd_w
        for p_, sums, wgt in ((seg32, sums_m, self.main_weight), (aux32, sums_a, self.aux_weight)):
            L.call("csbsr_segloss_reduce", _ptr(p_), _ptr(mask), _ptr(sdf), B, hw, _ptr(sums), pw[0], pw[1], eng.stream)
            L.call("csbsr_segloss_finish", _ptr(p_), _ptr(mask), _ptr(sdf), B, hw, _ptr(sums), alpha, pw[0], pw[1], lw[0], lw[1], wgt,
                   None, _ptr(seg_loss), None, 0, eng.stream)
        # MODEL.SR="bicubic": no SR loss (None, as the reference's), zeros for the kernel, and the graph ends at the detector's input
        sr_loss, kpred, terms = self._sr_loss_terms(iter, x, hr, kgt, sr32, kvec, seg32, mask) if self._has_kbpn else (None, None, None)
        if keep:
            det = dict(mask=mask, mean=mean, invstd=invstd, seg32=seg32, aux32=aux32, sdf=sdf, sums_m=sums_m, sums_a=sums_a, alpha=alpha,
                       psp_saved=psp_saved)
            st = self._saved_state(iter, x, det, hr, kgt, sr32, kvec, saves, mb, terms)
            seg_loss, sr_loss = _StepFn.apply(self, st, seg_loss, sr_loss, *self.parameters())
        return seg_loss, sr_loss, seg32, sr32, torch.zeros_like(kgt) if kpred is None else kpred


class SRModelWithLoss(_TrainBase):
    """KBPN and KBPNLoss alone (build_model.py:535-552): the model of the reference's ``DATASET.ONLY_IMAGES`` regime, whose run leaves the
    weights every ``MODEL.SR_SCRATCH = False`` model starts from (``pretrained_sr_path``).

        .forward(iter, x, sr_targets=None, kernel_targets=None) -> (sr_loss[B], sr_preds[B,3,H,W], kernel_preds[B,1,K,K])

    It holds ``sr_model.*`` only: ``state_dict()`` and ``parameters()`` are the ``sr_model.*`` part of the joint model's, in its order, and no
    detector is constructed, moved to the device or given a gradient bucket.  The forward and the backward are the joint model's SR half
    (_TrainBase): the same launches on the same bytes, so inside ``SR_PRETRAIN_ITER`` the two models produce the same bits.  The loss scale
    follows the PSPNet rule, 2^round(log2(B*H*W)) minus ``scale_backoff``, and the residency budget has no detector term."""

    def __init__(self, cfg, sr_transforms=None, num_train_ds=None, resume_iter=None, antialias=True, device="cuda:0", seed=None,
                 pretrained_root="weights"):
        if cfg.SOLVER.SR_LOSS_FUNC != "KBPN":
            raise NotImplementedError(f"SOLVER.SR_LOSS_FUNC={cfg.SOLVER.SR_LOSS_FUNC!r}: csbsr_amd builds KBPNLoss")
        if cfg.SOLVER.ORIENTED_WEIGHT_ITER != -1 and (cfg.SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SR_AMP != 0 or cfg.SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP != 0):
            # sr_loss_functions.py hands segment_preds=None to the oriented weight there: the reference fails at the first such iteration
            raise NotImplementedError("an oriented SR-loss weight needs the detector's map, which the SR-only model does not have")
        super().__init__(cfg, antialias, device, seed, pretrained_root, sr_only=True, sr_transforms=sr_transforms)
        self.sr_loss_fn = "KBPNLoss"
        self._init_loss_scale()

    def forward(self, iter, x, sr_targets=None, kernel_targets=None):
        x, hr, kgt = self._begin(x, sr_targets, kernel_targets)
        sr32, kvec, saves, mb = self._kbpn_forward(iter, x, kgt)
        sr_loss, kpred, terms = self._sr_loss_terms(iter, x, hr, kgt, sr32, kvec, None, None)
        if self.training and torch.is_grad_enabled():
            st = self._saved_state(iter, x, None, hr, kgt, sr32, kvec, saves, mb, terms)
            sr_loss = _StepFn.apply(self, st, None, sr_loss, *self.parameters())[1]
        return sr_loss, sr32, kpred


class JointModel(_JointBase):
    """Inference counterpart (build_model.py:441-500): SR clipped to [0,1] before segmentation, kernel normalised."""

    def __init__(self, cfg, antialias=True, device="cuda:0", seed=None, pretrained_root="weights"):
        super().__init__(cfg, antialias, device, seed, pretrained_root)
        self.ksize = cfg.BLUR.KERNEL_SIZE_OUTPUT

    @torch.no_grad()
    def forward(self, x, damy_kernel, sr_targets=None):
        x, kgt = self._begin(x, damy_kernel)
        kbpn, psp = self._rt["kbpn"], self._rt["psp"]
        if self._has_kbpn:
            sr32, kvec = kbpn.forward(x, -1, kgt, save=False)
            sr32.clamp_(0, 1)
        else:                   # build_model.py:69-73 + clip_sr: the clip is the up-sampler's own
            sr32, kvec = self._bicubic_up(x, clip=True), None
        xin, _, _ = self._norm_sr(sr32)
        seg32, _ = psp.forward(xin, {k: None for k in psp.drop_keys}, training=self.training, kvec=kvec if self.blur_skip else None)
        if kvec is None:
            return sr32, seg32, torch.zeros_like(kgt)
        return sr32, seg32, (kvec / kvec.sum(1, keepdim=True)).reshape(x.shape[0], 1, self.ksize, self.ksize)
