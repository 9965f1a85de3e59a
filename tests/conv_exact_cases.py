"""The case table of tests/test_conv_exact_gpu.py: one row per dispatch path of the convolution kernels, with the kernel ID it must
reach.  Plain data, importable without a GPU: tests/test_conv_exact_coverage_cpu.py checks that every forward kernel (``enum CONVK_*``,
csrc/conv_common.h) and every weight-gradient kernel (``enum WGRADK_*``, csrc/conv_wgrad.h) has a row or a written exclusion.

Row fields:
  op      "fwd" (Conv.fwd), "dgrad" (Conv.bwd_input of the layer described), "wgrad" (Conv.bwd_weights), "classbias" (Conv.fwd_classbias)
  shape   cin, cout, k, stride, pad, transposed and the layer's INPUT size N x H x W (dgrad / wgrad: of the forward layer)
  epi     fwd: activation (none / relu / lrelu / prelu, slope 0.25 / sigmoid) + residual (_add / _sub / _fma), or "bn" (BatchNorm sums) /
          "sum" (per-sample channel sums, output not stored);  dgrad: "" / "acc" (accumulate into the old gradient) / "mask"
          (activation mask of the layer below, slope 0.25) / "acc_mask"
  modes   debug modes: csbsr_debug_set_<name>(value) for the library, "eng.<attr>" for Engine attributes, "arg.cb_mode" the
          class-bias table of a "classbias" row (Conv.fwd_classbias; segs = (feature channels, folded channels))
  kid     csbsr_debug_last_conv_kernel() & 255 (fwd / dgrad) or csbsr_debug_last_wgrad_kernel() (wgrad)
  var     csbsr_debug_last_conv_kernel() >> 8 (the template instance, csbsr_debug.h), None where the dispatcher encodes none
  budget  a persistent-grid family (conv_x3 / x3n / x3w / tp / hr): run again under CU budgets (BUDGETS), bit-identical
"""
from collections import namedtuple

# library defaults of the debug modes: the initial values of the mode variables in csrc/ (tests/test_conv_exact_coverage_cpu.py reads
# them from the sources).  The GPU test restores these after every row.
DEFAULT_MODES = {"conv_glds": 2, "conv_x3": 1, "conv_x3n": 1, "conv_x3w": 0, "conv_tp": 1, "wgrad_tr": 1, "wgrad_hr": 1}

# CU budgets of the tile-walk runs (csbsr_debug_stream_set_cu_budget): a budget of g makes every workgroup walk tiles g apart (the wide
# form of conv_x3n runs 2 g workgroups); conv_hr rounds its grid up to a multiple of 8 x cout-tile groups, so it gets 8 and 16
BUDGETS = {"default": (1, 3, 7), "hr": (8, 16)}

Row = namedtuple("Row", "name op cin cout k s p tr N H W epi modes kid var budget segs why")


def R(name, op, cin, cout, k, s, p, tr, N, H, W, epi="none", modes=(), kid=-1, var=None, budget=False, segs=(), why=""):
    return Row(name, op, cin, cout, k, s, p, tr, N, H, W, epi, tuple(modes), kid, var, budget, tuple(segs), why)


X3 = (("conv_x3", 2),)
X3N = (("conv_x3n", 2),)
X3W = (("conv_x3w", 2), ("eng.use_x3w", 2))
TP = (("conv_tp", 2),)
ROWS = [
    # ---- register-staged implicit GEMM (csrc/conv_igemm.hip)
    R("igemm32", "fwd", 16, 32, 3, 1, 1, False, 2, 9, 11, "lrelu", kid=0, why="coutp 32: below every LDS-DMA tile, 16 channels: not x3n"),
    R("igemm64", "fwd", 16, 64, 3, 1, 1, False, 2, 12, 12, "relu_add", kid=1, why="16 input channels: the LDS-DMA general K walk needs >= 32"),
    R("igemm128", "fwd", 16, 128, 3, 1, 1, False, 2, 10, 12, "prelu", kid=2, why="as above, coutp > 64"),
    R("igemm128_tr", "fwd", 64, 128, 8, 4, 2, True, 2, 8, 8, "none", modes=(("conv_glds", 0),), kid=2, why="LDS-DMA kernels off: transposed, 16 phases"),
    R("igemm64_2seg", "fwd", 64, 64, 3, 1, 1, False, 2, 10, 12, "none", kid=1, segs=(24, 40),
      why="two input segments whose first is not whole 64-channel slices: not LDS-DMA"),
    # ---- LDS-DMA implicit GEMM (csrc/conv_igemm_glds.hip): 64 / 128 / 256 / 256W tiles, GK = general K walk (var 2)
    R("glds64", "fwd", 64, 64, 3, 1, 1, False, 2, 40, 70, "lrelu", kid=14, var=0, why="33..64 couts, K in whole 64-channel slices"),
    R("glds64_gk", "fwd", 48, 64, 3, 1, 1, False, 2, 40, 44, "none", kid=14, var=2, why="48 channels: a 64-wide K slice straddles taps"),
    R("glds128", "fwd", 128, 128, 3, 1, 1, False, 2, 16, 16, "lrelu_sub", kid=3, var=0, why="short K, < 65536 pixels"),
    R("glds128_gk", "fwd", 48, 96, 3, 1, 1, False, 2, 24, 40, "relu", kid=3, var=2, why="HRNet-W48 widths: general K walk"),
    R("glds128_tr", "fwd", 128, 128, 8, 4, 2, True, 2, 8, 8, "none", kid=3, var=0, why="transposed, too small for conv_tp's default mode"),
    R("glds128_2seg", "fwd", 128, 128, 3, 1, 1, False, 2, 10, 12, "none", kid=3, var=0, segs=(64, 64), why="two 64-channel segments"),
    R("glds256", "fwd", 256, 128, 3, 1, 1, False, 1, 256, 256, "none", kid=4, var=0, why="K 2304, 65536 pixels: the 256-row tile"),
    R("glds256_gk", "fwd", 264, 128, 3, 1, 1, False, 1, 256, 256, "relu", kid=4, var=2, why="as above, 264 channels: general K walk"),
    R("glds256w", "fwd", 256, 256, 3, 1, 1, False, 1, 256, 256, "none", modes=(("conv_x3", 0),), kid=7, var=0,
      why="256 couts: the 256 px x 256 cout tile (conv_x3 off: this launch fills the chip, conv_x3 would take it)"),
    R("glds256w_gk", "fwd", 264, 256, 3, 1, 1, False, 1, 256, 256, "lrelu", kid=7, var=2, why="as above, general K walk"),
    R("glds128_dgrad", "dgrad", 128, 128, 3, 1, 1, False, 2, 16, 16, "acc", kid=3, var=0, why="dgrad of a 128 -> 128 3x3, accumulating"),
    R("glds64_dgrad_s2", "dgrad", 64, 128, 3, 2, 1, False, 2, 32, 32, "", kid=14, var=0, why="strided conv: gather-form transposed dgrad, 64 couts"),
    # ---- thin kernels (csrc/conv_thin.hip)
    R("thin_cout", "fwd", 64, 3, 3, 1, 1, False, 2, 20, 24, "none", kid=5, why="3 couts: taps in rows"),
    R("thin_cin", "fwd", 3, 64, 3, 1, 1, False, 2, 19, 45, "relu", modes=(("conv_glds", 2 | 512),), kid=6, why="3-channel input, streaming variant off"),
    R("thin_cin2", "fwd", 3, 128, 3, 1, 1, False, 2, 19, 45, "lrelu", kid=13, why="3-channel input, plain epilogue: streaming kernel"),
    R("thin_tp", "fwd", 3, 128, 8, 4, 2, True, 2, 13, 21, "prelu_add", kid=11, why="kb.up_conv1: 3 -> 128 8x8 stride 4"),
    R("thin_sc", "dgrad", 3, 128, 8, 4, 2, True, 4, 128, 128, "", kid=15, why="dgrad of kb.up_conv1 into 3 channels, >= 65536 pixels"),
    R("thin_tpd", "dgrad", 3, 64, 7, 2, 3, False, 2, 192, 256, "", kid=16, why="dgrad of the PSPNet stem, >= 65536 pixels"),
    # ---- direct full-resolution kernel (csrc/conv_hr.hip): var bits 1 seven octets, 2 1x1, 4 two cout tiles, 8 mask, 16 stat
    R("hr32", "fwd", 32, 32, 3, 1, 1, False, 2, 363, 371, "lrelu", kid=8, var=0, budget=True, why="32 -> 32 3x3, >= 256K pixels"),
    R("hr49", "fwd", 49, 49, 3, 1, 1, False, 2, 363, 371, "none", kid=8, var=1 | 4, budget=True, why="49 (7 octets) -> 49: two cout tiles"),
    R("hr_1x1", "fwd", 32, 49, 1, 1, 0, False, 2, 363, 371, "relu", kid=8, var=2 | 4, budget=True, why="1x1"),
    R("hr_stat", "fwd", 32, 49, 3, 1, 1, False, 2, 363, 371, "sum", kid=8, var=4 | 16, budget=True, why="fe_cat.2: per-sample sums, no store"),
    R("hr_mask", "dgrad", 32, 32, 3, 1, 1, False, 2, 363, 371, "mask", kid=8, var=8, budget=True, why="dgrad with the activation mask"),
    # ---- phase-decomposed transposed conv (csrc/conv_tp.hip): var bits 1 res, 2 acc, 4 mask
    R("tp_res", "fwd", 128, 128, 8, 4, 2, True, 2, 32, 70, "prelu_add", modes=TP, kid=9, var=1, budget=True, why="up_conv3 shape"),
    R("tp_plain", "fwd", 128, 100, 8, 4, 2, True, 2, 32, 40, "relu", modes=TP, kid=9, var=0, budget=True, why="padded couts"),
    R("tp_dgrad_acc_mask", "dgrad", 128, 128, 8, 4, 2, False, 2, 96, 280, "acc_mask", modes=TP, kid=9, var=2 | 4, budget=True,
      why="dgrad of an 8x8 stride-4 conv, accumulating, masked"),
    R("tp_dgrad", "dgrad", 128, 128, 8, 4, 2, False, 2, 96, 280, "", modes=TP, kid=9, var=0, budget=True, why="plain dgrad"),
    # ---- wide 3x3 / k = 2 x stride kernel (csrc/conv_x3.hip): X3F / X3SF = straight-line rows, var 1 = the sigmoid / FMA rows
    R("x3f", "fwd", 128, 128, 3, 1, 1, False, 2, 24, 70, "lrelu", modes=X3, kid=17, var=0, budget=True, why="straight-line rows"),
    R("x3", "fwd", 128, 100, 3, 1, 1, False, 2, 24, 70, "lrelu_fma", modes=X3, kid=10, var=0, budget=True, why="FMA with an activation: general rows"),
    R("x3_sft", "fwd", 128, 128, 3, 1, 1, False, 2, 24, 70, "none_fma", modes=X3, kid=10, var=1, budget=True, why="SFT conv1 rows"),
    R("x3f_dgrad", "dgrad", 128, 128, 3, 1, 1, False, 2, 24, 70, "acc", modes=X3, kid=17, var=0, budget=True, why="dgrad, accumulating"),
    R("x3sf", "fwd", 128, 128, 8, 4, 2, False, 2, 96, 280, "lrelu", modes=X3, kid=18, var=0, budget=True, why="8x8 stride 4, 24 x 70 out"),
    R("x3s", "fwd", 128, 128, 8, 4, 2, False, 2, 96, 280, "none_fma", modes=X3, kid=12, var=0, budget=True, why="strided, FMA rows"),
    # ---- Winograd F(2,3) along x (csrc/conv_x3w.hip): var 1 straight-line rows, 2 SFT rows, 0 general
    R("x3w_fast", "fwd", 128, 128, 3, 1, 1, False, 2, 24, 70, "lrelu", modes=X3W, kid=19, var=1, budget=True, why="straight-line rows"),
    R("x3w_sft", "fwd", 128, 128, 3, 1, 1, False, 2, 24, 70, "none_fma", modes=X3W, kid=19, var=2, budget=True, why="SFT rows"),
    R("x3w_gen", "fwd", 128, 128, 3, 1, 1, False, 2, 24, 70, "lrelu_fma", modes=X3W, kid=19, var=0, budget=True, why="general rows"),
    # ---- narrow / wide resident-pixel 3x3 kernel (csrc/conv_x3n.hip): var 1 fast rows, 3 BN sums, 4 wide, 8 lean
    R("x3n_narrow", "fwd", 64, 64, 3, 1, 1, False, 2, 40, 130, "lrelu_fma", modes=X3N, kid=20, var=0, budget=True, why="narrow, general rows"),
    R("x3n_narrow_fast", "fwd", 64, 64, 3, 1, 1, False, 2, 40, 130, "lrelu", modes=X3N, kid=20, var=1, budget=True, why="narrow, fast rows"),
    R("x3n_narrow_bn", "fwd", 64, 64, 3, 1, 1, False, 2, 40, 130, "bn", modes=X3N, kid=20, var=3, budget=True, why="narrow + BN sums"),
    R("x3n_wide", "fwd", 128, 128, 3, 1, 1, False, 2, 40, 130, "relu_fma", modes=X3N, kid=20, var=4, budget=True, why="wide, general rows"),
    R("x3n_wide_fast", "fwd", 128, 128, 3, 1, 1, False, 2, 40, 130, "relu_add", modes=X3N, kid=20, var=5, budget=True, why="wide, fast rows"),
    R("x3n_wide_lean", "fwd", 128, 128, 3, 1, 1, False, 2, 40, 130, "lrelu", modes=X3N, kid=20, var=13, budget=True, why="wide, lean stores"),
    R("x3n_dgrad", "dgrad", 64, 128, 3, 1, 1, False, 2, 40, 130, "acc", modes=X3N, kid=20, var=1, budget=True, why="dgrad 128 -> 64"),
    # ---- padded couts (cout % 8 != 0): the masked last octet of every family's epilogue (conv_common.h: EpiFast::masked), pads must be zero
    R("igemm32_pad", "fwd", 16, 28, 3, 1, 1, False, 2, 9, 11, "lrelu", kid=0, why="28 -> 32 padded couts"),
    R("igemm128_pad", "fwd", 16, 100, 3, 1, 1, False, 2, 10, 12, "relu_add", kid=2, why="100 -> 104 padded couts"),
    R("glds64_pad", "fwd", 64, 60, 3, 1, 1, False, 2, 40, 70, "lrelu", kid=14, var=0, why="60 -> 64 padded couts"),
    R("glds128_pad", "fwd", 128, 100, 3, 1, 1, False, 2, 16, 16, "lrelu_sub", kid=3, var=0, why="100 -> 104 padded couts"),
    R("glds256_pad", "fwd", 256, 200, 3, 1, 1, False, 1, 256, 256, "relu", modes=(("conv_x3", 0),), kid=4, var=0,
      why="200 couts: 256-row tile (conv_x3 off: this launch fills the chip)"),
    R("glds256w_pad", "fwd", 256, 250, 3, 1, 1, False, 1, 256, 256, "lrelu", modes=(("conv_x3", 0),), kid=7, var=0, why="250 -> 256 padded couts"),
    R("x3f_pad", "fwd", 128, 100, 3, 1, 1, False, 2, 24, 70, "lrelu", modes=X3, kid=17, var=0, budget=True, why="straight-line rows, 104 padded"),
    R("x3w_pad", "fwd", 128, 100, 3, 1, 1, False, 2, 24, 70, "lrelu", modes=X3W, kid=19, var=1, budget=True, why="straight-line rows, 104 padded"),
    R("x3n_narrow_pad", "fwd", 64, 60, 3, 1, 1, False, 2, 40, 130, "lrelu", modes=X3N, kid=20, var=1, budget=True, why="narrow, 60 -> 64"),
    R("x3n_wide_pad", "fwd", 128, 100, 3, 1, 1, False, 2, 40, 130, "lrelu", modes=X3N, kid=20, var=13, budget=True, why="wide lean, 100 -> 104"),
    # ---- sigmoid epilogues: no exact result; compared with the sigmoid of the exact pre-activation to 1 fp16 ulp
    R("glds128_sigmoid", "fwd", 128, 100, 3, 1, 1, False, 2, 16, 16, "sigmoid", kid=3, var=0, why="general epilogue row"),
    R("x3_sigmoid", "fwd", 128, 100, 3, 1, 1, False, 2, 24, 70, "sigmoid", modes=X3, kid=10, var=1, budget=True, why="SFT conv1 scale branch"),
    R("x3w_sigmoid", "fwd", 128, 128, 3, 1, 1, False, 2, 24, 70, "sigmoid", modes=X3W, kid=19, var=2, budget=True, why="SFT rows"),
    R("x3n_wide_sigmoid", "fwd", 128, 100, 3, 1, 1, False, 2, 40, 130, "sigmoid", modes=X3N, kid=20, var=4, budget=True, why="wide, general rows"),
    # ---- more conv_tp dgrad instances
    R("tp_dgrad_acc", "dgrad", 128, 128, 8, 4, 2, False, 2, 96, 280, "acc", modes=TP, kid=9, var=2, budget=True, why="accumulating dgrad"),
    R("tp_dgrad_mask", "dgrad", 100, 128, 8, 4, 2, False, 2, 96, 280, "mask", modes=TP, kid=9, var=4, budget=True,
      why="masked dgrad into 100 -> 104 padded channels"),
    # ---- Conv.fwd_classbias: segment 1 enters as a per-(sample, position class) bias table; cb_mode 0 = 16 border classes, 1 = 25 two-ring classes
    R("classbias_ring_hr", "classbias", 32, 32, 1, 1, 0, False, 2, 363, 371, "lrelu", modes=(("arg.cb_mode", 1),), kid=8, var=2 | 32, budget=True, segs=(32, 16),
      why="fe_cat.0: 1x1, cb_mode 1 on conv_hr's class-bias variant"),
    R("classbias_border", "classbias", 128, 100, 3, 1, 1, False, 2, 12, 20, "lrelu", kid=3, var=0, segs=(128, 16),
      why="cb_mode 0, 3x3 on the general kernels"),
    R("classbias_ring", "classbias", 128, 100, 3, 1, 1, False, 2, 12, 20, "relu", modes=(("arg.cb_mode", 1),), kid=3, var=0, segs=(128, 16),
      why="cb_mode 1, 3x3 on the general kernels"),
    # ---- weight gradients (csrc/conv_wgrad*.hip); wgrad_tr 129 = register-staged kernel everywhere.  1850 pixels (2 x 25 x 37): the kernels
    # split the pixel range into 512-pixel slabs (csbsr_wgrad_splits: at most ceil(M / 512)), so every row walks four splits, the last one ragged
    R("wg_reg128", "wgrad", 128, 128, 3, 1, 1, False, 2, 25, 37, modes=(("wgrad_tr", 129),), kid=0, why="register-staged 128 x 128"),
    R("wg_reg128w", "wgrad", 768, 128, 3, 1, 1, False, 2, 25, 37, modes=(("wgrad_tr", 129),), kid=1, why="6912 columns: 128 x 256"),
    R("wg_reg64", "wgrad", 32, 64, 3, 1, 1, False, 2, 25, 37, kid=2, why="64 rows: below the LDS-DMA kernel"),
    R("wg_reg32", "wgrad", 16, 32, 3, 1, 1, False, 2, 25, 37, kid=3, why="32 rows"),
    R("wg_thin", "wgrad", 64, 3, 3, 1, 1, False, 2, 25, 37, kid=4, why="3 couts: taps in rows (64-channel input: not mirrored)"),
    R("wg_glds128", "wgrad", 128, 128, 3, 1, 1, False, 2, 25, 37, kid=5, why="LDS-DMA 128 x 128"),
    R("wg_glds128w", "wgrad", 768, 128, 3, 1, 1, False, 2, 25, 37, kid=6, why="LDS-DMA 128 x 256"),
    R("wg_glds256", "wgrad", 128, 256, 3, 1, 1, False, 2, 25, 37, kid=7, why="256 rows: 256 x 256"),
    R("wg_glds256_rem", "wgrad", 128, 320, 3, 1, 1, False, 2, 25, 37, kid=7, why="320 rows: 256 x 256 + the 64-row remainder launch"),
    R("wg_hr", "wgrad", 32, 32, 3, 1, 1, False, 2, 19, 45, modes=(("wgrad_hr", 2),), kid=8, why="full-resolution thin kernel"),
    R("wg_glds512", "wgrad", 128, 128, 8, 4, 2, False, 2, 100, 148, kid=9,
      why="8x8 stride 4 (25 x 37 out): the four-tap 128 x 512 tile, row shift across the splits"),
    R("wg_mirror_2seg", "wgrad", 256, 3, 3, 1, 1, False, 2, 25, 37, kid=5, segs=(128, 128),
      why="<= 64 couts, 128-channel segments: mirrored, two launches"),
    R("wg_tr", "wgrad", 128, 128, 8, 4, 2, True, 2, 25, 37, kid=9, why="transposed 8x8 stride 4: A = the LR input, tap-permuted 128 x 512"),
]

# kernel IDs with no row, and why
EXCLUDED = {}

# The template instances the dispatchers build (csbsr_debug.h, bits 8.. of csbsr_debug_last_conv_kernel) and the engine's entry points into the
# convolution kernels.  tests/test_conv_exact_coverage_cpu.py requires a row for each -- or an entry in NOT_COVERED with the reason.
REQUIRED_VARIANTS = {
    # conv_igemm_glds.hip: bit 1 FS (fused split stage), bit 2 GK (general K walk), for each tile
    "GLDS64": (14, (0, 1, 2, 3)), "GLDS128": (3, (0, 1, 2, 3)), "GLDS256": (4, (0, 1, 2, 3)), "GLDS256W": (7, (0, 1, 2, 3)),
    # conv_x3.hip: bit 1 the sigmoid / FMA rows of the general instance
    "X3": (10, (0, 1)), "X3F": (17, (0,)), "X3S": (12, (0,)), "X3SF": (18, (0,)),
    # conv_x3w.hip: 1 straight-line rows, 2 SFT rows
    "X3W": (19, (0, 1, 2)),
    # conv_x3n.hip: narrow 0 / 1 / 3 (BN sums), wide 4 / 5 / 13 (lean)
    "X3N": (20, (0, 1, 3, 4, 5, 13)),
    # conv_tp.hip: 1 res, 2 acc, 4 mask, 8 fused activation-gradient sums
    "TP": (9, (0, 1, 2, 4, 6, 14, 13)),
    # conv_hr.hip: the instances the models launch -- 1 seven octets, 2 1x1, 4 two cout tiles, 8 mask, 16 stat, 32 class bias
    "HR": (8, (0, 1 | 4, 2 | 4, 4 | 16, 8, 2 | 32)),
}
# entry points: Conv's public fwd* / bwd* methods (read from csbsr_amd/engine.py by the coverage test), the subclasses of Conv, and the
# operand modes that take separate kernel paths
ROW_ENTRY = {"fwd": "Conv.fwd", "dgrad": "Conv.bwd_input", "wgrad": "Conv.bwd_weights", "classbias": "Conv.fwd_classbias"}
# (the rows of tests/fused_exact_cases.py -- the paths with second outputs, the folded segment, ShuffleConv, kp_bwd -- name their entry
# point themselves: FRow.entry; tests/test_conv_exact_coverage_cpu.py counts both tables)
# (the split-precision rows -- the fused-split instances of conv_igemm_glds.hip, fwd_blocks 1 / 2 / 3, split output slices, the split-input
# forms of Conv.fwd_folded / fwd_const_1x1, the high-precision dgrad -- are a third table with a lattice of its own,
# tests/split_conv_cases.py; each of its rows names its mode, "split" or "Conv.hp_dgrad")
REQUIRED_MODES = ("sigmoid", "split", "Conv.hp_dgrad")

# required paths with neither a row nor a test yet, and why (nothing at present)
NOT_COVERED = {}
