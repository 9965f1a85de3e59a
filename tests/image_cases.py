"""Shared by tests/test_image_cases_cpu.py and tests/test_image_exact_gpu.py: references, exact-lattice inputs, case tables, a dispatch
restatement and reference mutants for the per-sample blur and the bicubic resizes of csrc/image_ops.hip.  No GPU.

References, written from the formulas in fp64 (every lattice value and every sum of them is an integer multiple of a power of two far
below 2^53, so fp64 holds them exactly, as int64 would):

  blur      y[n,c,oy,ox] = sum_{ky,kx} x[n,c,oy s - P + ky, ox s - P + kx] k[n][ky K + kx]  (- sub), zero padding, P = (K - 1) / 2,
            OH = (H + 2 P - K) // s + 1; the two adjoints dx (scatter of dy k) and dk (sum over c, oy, ox of dy x).
  bicubic   separable axis operators in the style of bicubic_cases.up_matrix: down_matrix(n, f, antialias) is [n // f, n],
            up_add_matrix(n, s) is [n s, n]; y = M_y x M_x^T and dx = M_y^T dy M_x.
            antialias=True: Keys' cubic with A = -0.5 stretched to support 2 f, taps [max(int(c - 2f + .5), 0), min(int(c + 2f + .5), n))
            around c = f (o + .5), divided by their in-image sum.  antialias=False and the up-scale: A = -0.75, four taps whose INDICES
            are clamped to the image (a clamped tap folds its weight onto the border pixel).

Exactness classes (each builder proves its own line on the reference before it returns):

  blur, all three entry points   operands are integers x 2^-q, K^2 max|x| max|k| < 2^24 units: a sum of products in ANY order is exact
                                 in fp32 -> bit-equality.  The fp16 output: x in {-1, 0, 1}, k in {-4 .. 4}, |y| <= 1764 < 2048.
  non-antialiased down, f even   the weights are exactly {-3, 19, 19, -3} / 32; x on 2^-4 {-15 .. 15} -> bit-equality, both directions.
  up_add, s = 2 / s = 4          weights are multiples of 2^-8 / 2^-11; integers in {-15 .. 15} / ternary input -> bit-equality.
  antialiased down, up_add s = 8 the result rounds: per element |got - ref| <= n 2^-24 (|M_y| |x| |M_x|^T (+ |out0|)), n from
                                 aa_roundings() / UP8_ROUNDINGS: a count of the kernel's roundings, not a fit to its output.

The heavy rows (585 x 590, 840 x 840, 1024 x 768) exist because a seam shows only there: tiles_per_wg = 2 and the grid-stride wrap.
"""
import functools
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from bicubic_cases import cub
from exact_lattice import FP32_EXACT, assert_fp16_exact, assert_fp32_exact, assert_on_lattice, assert_sum_bound, draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csbsr_amd", "csrc")
U = 2.0 ** -24          # fp32 unit roundoff


# ------------------------------------------------------------------------------------------- what the source states

@functools.lru_cache(maxsize=None)
def source():
    with open(os.path.join(CSRC, "image_ops.hip")) as f:
        return f.read()


def _section(start, end):
    s = source()
    a, b = s.index(start), s.index(end)
    assert a < b
    return s[a:b]


def blur_section():
    return _section("// ------------------------------------------------------------------------------------------- depthwise blur",
                    "// ------------------------------------------------------------------------------------------- bicubic")


def bicubic_section():
    return _section("// ------------------------------------------------------------------------------------------- bicubic",
                    "// ------------------------------------------------------------------------------------------- area down-scale")


@functools.lru_cache(maxsize=None)
def tile_constants():
    """the tile sizes and grid cap the case tables are built around, read from the lines of csrc/image_ops.hip that state them: a
    retiling changes these numbers (or breaks a pattern) and test_image_cases_cpu.py then fails the tables instead of a seam going
    silently untested"""
    s = source()

    def one(pattern, what):
        m = re.search(pattern, s)
        assert m, f"{what}: pattern {pattern!r} not found in csrc/image_ops.hip"
        return tuple(int(g) for g in m.groups())

    TR, TC = one(r"TR = (\d+), TC = (\d+), WC = TC \+ K - 1", "stride-1 blur tile")
    (TL,) = one(r"S = 4, TL = (\d+), WIN = 7", "stride-4 input-gradient tile")
    (TO1,) = one(r"constexpr int TO = (\d+), P = \(K - 1\) / 2, XW = TO - 1 \+ K", "stride-1 kernel-gradient tile")
    TOa, TOb, TOc = one(r"const int TO = stride == 1 \? (\d+) : \(stride <= 4 \? (\d+) : (\d+)\)", "kernel-gradient tile rule")
    WGS1, WGS = one(r"int tpw = \(total \+ (\d+)\) / (\d+);", "kernel-gradient workgroups per sample")
    BLOCK, CAP = one(r"grid_for\(long work, int block = (\d+), int cap = (\d+)\)", "grid cap")
    (FT,) = one(r"dim3 grid\(\(OW \+ 15\) / (\d+), \(OH \+ 15\) / 16, N \* C\)", "generic forward tile")
    assert TOa == TO1 and WGS1 == WGS - 1
    return dict(TR=TR, TC=TC, TL=TL, TO={1: TOa, 2: TOb, 4: TOb, 8: TOc}, WGS=WGS, BLOCK=BLOCK, CAP=CAP, FT=FT)


def out_size(n, K, s):
    P = (K - 1) // 2
    return (n + 2 * P - K) // s + 1


def blur_kernel_for(entry, K, stride, H, W, C):
    """(kernel name, tiles_per_wg) a call of ``entry`` ('fwd', 'bwd_input', 'bwd_kernel') launches.  A TRANSCRIPTION of the three
    extern "C" bodies of csrc/image_ops.hip (csbsr_blur_fwd, csbsr_blur_bwd_input, csbsr_blur_bwd_kernel): it cannot observe the
    launch, so it has to be kept in step with them by hand; the tile sizes it uses come from tile_constants().  tiles_per_wg is 1
    where the kernel has no such notion."""
    assert K in (5, 7, 21), "BLUR_DISPATCH refuses every other size"
    t = tile_constants()
    OH, OW = out_size(H, K, stride), out_size(W, K, stride)
    if entry == "fwd":
        return ("blur_bwd_input_s1_kernel<FWD>" if stride == 1 and K == 21 else "blur_fwd_kernel"), 1
    if entry == "bwd_input":
        if stride == 1 and K == 21:
            return "blur_bwd_input_s1_kernel<BWD>", 1
        if stride == 4 and K == 21 and H == 4 * OH and W == 4 * OW and W % 4 == 0:
            return "blur_bwd_input_s4_kernel", 1
        return "blur_bwd_input_kernel", 1
    assert entry == "bwd_kernel"
    TO = t["TO"][stride]
    total = C * ((OW + TO - 1) // TO) * ((OH + TO - 1) // TO)
    tpw = max((total + t["WGS"] - 1) // t["WGS"], 1)
    return ("blur_bwd_kernel_s1_kernel" if stride == 1 and K == 21 and OH == H and OW == W else "blur_bwd_kernel_kernel"), tpw


BLUR_KERNEL_NAMES = ["blur_fwd_kernel", "blur_bwd_input_kernel", "blur_bwd_input_s1_kernel<FWD>", "blur_bwd_input_s1_kernel<BWD>",
                     "blur_bwd_input_s4_kernel", "blur_bwd_kernel_kernel", "blur_bwd_kernel_s1_kernel"]


def grid_wraps(elements):
    """does a grid-stride kernel launched through grid_for() wrap (a thread takes more than one element)?"""
    t = tile_constants()
    return elements > t["BLOCK"] * t["CAP"]


# ------------------------------------------------------------------------------------------- blur references

def _k3(k, K):
    k = torch.as_tensor(k, dtype=torch.float64)
    return k.reshape(k.shape[0], K, K)


def _padded(x, K, pad, origin):
    """x with P + origin pixels before and P - origin after each image axis (origin = 0: the blur's own window)"""
    P = (K - 1) // 2
    return F.pad(torch.as_tensor(x, dtype=torch.float64), (P + origin, P - origin, P + origin, P - origin),
                 mode="replicate" if pad == "replicate" else "constant")


def blur_ref(x, k, K, stride, sub=None, pad="zero", origin=0):
    """fp64 [N, C, OH, OW]; ``pad`` / ``origin`` exist for the mutants (edge replication, a window that starts one pixel early)"""
    x = torch.as_tensor(x, dtype=torch.float64)
    N, C, H, W = x.shape
    k, s = _k3(k, K), stride
    OH, OW = out_size(H, K, s), out_size(W, K, s)
    xp = _padded(x, K, pad, origin)
    y = torch.zeros(N, C, OH, OW, dtype=torch.float64)
    for ky in range(K):
        for kx in range(K):
            y += xp[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] * k[:, ky, kx].view(N, 1, 1, 1)
    return y if sub is None else y - torch.as_tensor(sub, dtype=torch.float64)


def blur_dx_ref(dy, k, K, stride, H, W, pad="zero", origin=0):
    """fp64 [N, C, H, W]: the adjoint of blur_ref in x"""
    dy = torch.as_tensor(dy, dtype=torch.float64)
    N, C, OH, OW = dy.shape
    assert (OH, OW) == (out_size(H, K, stride), out_size(W, K, stride))
    k, s, P = _k3(k, K), stride, (K - 1) // 2
    g = torch.zeros(N, C, H + 2 * P, W + 2 * P, dtype=torch.float64)
    for ky in range(K):
        for kx in range(K):
            g[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] += dy * k[:, ky, kx].view(N, 1, 1, 1)
    a, b = P + origin, P - origin
    if pad == "replicate":          # the adjoint of edge replication folds the margins onto the border pixels
        g[:, :, a] += g[:, :, :a].sum(2)
        g[:, :, a + H - 1] += g[:, :, a + H:].sum(2)
        g[:, :, :, a] += g[:, :, :, :a].sum(3)
        g[:, :, :, a + W - 1] += g[:, :, :, a + W:].sum(3)
    return g[:, :, a:a + H, a:a + W].clone()


def blur_dk_ref(dy, x, K, stride, pad="zero", origin=0):
    """fp64 [N, K, K]: the adjoint of blur_ref in k, summed over the channels"""
    dy = torch.as_tensor(dy, dtype=torch.float64)
    N, C, OH, OW = dy.shape
    s = stride
    xp = _padded(x, K, pad, origin)
    dk = torch.zeros(N, K, K, dtype=torch.float64)
    for ky in range(K):
        for kx in range(K):
            dk[:, ky, kx] = (xp[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] * dy).sum((1, 2, 3))
    return dk


# ------------------------------------------------------------------------------------------- blur draws

def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(v) for v in key)) % (2 ** 31))


def draw_taps(N, K, amp, gen):
    """[N, K, K] non-zero integers in [-amp, amp], not normalised; asserted asymmetric (k != k flipped, k != k^T), different per
    sample, with four non-zero corners"""
    mag = torch.randint(1, amp + 1, (N, K, K), generator=gen)
    sign = torch.randint(0, 2, (N, K, K), generator=gen) * 2 - 1
    k = (mag * sign).to(torch.float32)
    for n in range(N):
        assert not torch.equal(k[n], k[n].flip(0, 1)) and not torch.equal(k[n], k[n].T), "taps: a symmetric draw"
        assert not torch.equal(k[n], k[n].flip(0)) and not torch.equal(k[n], k[n].flip(1)), "taps: a symmetric draw"
        assert all(float(k[n, i, j]) != 0 for i in (0, K - 1) for j in (0, K - 1)), "taps: a zero corner"
        assert n == 0 or not torch.equal(k[n], k[n - 1]), "taps: two samples share a kernel"
    return k


def _image(shape, q, amp, gen):
    """lattice image; dense when tiny (every pixel matters there), half zeros otherwise"""
    n = shape[-1] * shape[-2]
    t = draw(shape, q, amp, density=1.0 if n < 64 else 0.5, gen=gen)
    if n < 64:
        t = torch.where(t == 0, torch.full_like(t, 2.0 ** -q), t)
    return t


def blur_case(N, C, H, W, K, stride, fp16=False):
    """dict(x, k, sub, dy, dx0) of fp32 CPU tensors for one blur row, bounds proved.  fp16=False: x, sub, dy, dx0 in 2^-8 {-255 .. 255},
    k in {-64 .. 64} \\ {0}: 441 x 255 x 64 = 7.2e6 < 2^24 units of 2^-8, with one more unit-bounded term (sub, dx0) to spare.
    fp16=True: x in {-1, 0, 1}, k in {-4 .. 4} \\ {0}, sub in {-2 .. 2}: integers of magnitude <= 1766 < 2048 (fp16-exact)."""
    gen = _gen(N, C, H, W, K, stride, fp16)
    OH, OW = out_size(H, K, stride), out_size(W, K, stride)
    q, ax, ak, asub = (0, 1, 4, 2) if fp16 else (8, 255, 64, 255)
    d = dict(x=_image((N, C, H, W), q, ax, gen), k=draw_taps(N, K, ak, gen).reshape(N, K * K), sub=_image((N, C, OH, OW), q, asub, gen),
             dy=_image((N, C, OH, OW), q, ax, gen), dx0=_image((N, C, H, W), q, ax, gen))
    what = f"blur {N}x{C}x{H}x{W} K={K} s={stride}" + (" fp16" if fp16 else "")
    unit = 2.0 ** -q
    assert_sum_bound(K * K + 1, max(float(d["x"].abs().max()), float(d["dy"].abs().max()), float(d["sub"].abs().max()),
                                    float(d["dx0"].abs().max())), ak, unit, what)
    return d


@functools.lru_cache(maxsize=None)
def blur_fwd_reference(N, C, H, W, K, stride):
    """(case, {variant: fp64 reference}) of a csbsr_blur_fwd row, computed once and shared.  Variants: 'y32', 'y32_sub' on the rich
    draw; 'y16', 'both' (fp32 and fp16 output at once, with sub) on the fp16 draw."""
    c, h = blur_case(N, C, H, W, K, stride), blur_case(N, C, H, W, K, stride, fp16=True)
    y, yh = blur_ref(c["x"], c["k"], K, stride), blur_ref(h["x"], h["k"], K, stride)
    ref = {"y32": y, "y32_sub": y - c["sub"].double(), "y16": yh, "both": yh - h["sub"].double()}
    what = f"blur_fwd {N}x{C}x{H}x{W} K={K} s={stride}"
    for v in ("y32", "y32_sub"):
        assert_on_lattice(ref[v], 2.0 ** -8, what)
        assert_fp32_exact(ref[v], what)
    for v in ("y16", "both"):
        assert_on_lattice(ref[v], 1.0, what)
        assert_fp16_exact(ref[v], what + " fp16")
    return c, h, ref


@functools.lru_cache(maxsize=None)
def blur_dx_reference(N, C, H, W, K, stride):
    """(case, fp64 dx of the stored call); the accumulating call must give dx0 + dx, which is proved fp32-exact here too"""
    c = blur_case(N, C, H, W, K, stride)
    dx = blur_dx_ref(c["dy"], c["k"], K, stride, H, W)
    what = f"blur_bwd_input {N}x{C}x{H}x{W} K={K} s={stride}"
    assert_on_lattice(dx, 2.0 ** -8, what)
    assert_fp32_exact(dx, what)
    assert_fp32_exact(dx + c["dx0"].double(), what + " accumulate")
    return c, dx


def kgrad_case(N, C, H, W, K, stride):
    """integers |dy| <= 3, |x| <= 3: C OH OW 9 < 2^24 (asserted), so every partial row and both levels of the fold are exact"""
    gen = _gen(N, C, H, W, K, stride, 77)
    OH, OW = out_size(H, K, stride), out_size(W, K, stride)
    d = dict(x=_image((N, C, H, W), 0, 3, gen), dy=_image((N, C, OH, OW), 0, 3, gen))
    assert_sum_bound(C * OH * OW, 3, 3, 1.0, f"blur_bwd_kernel {N}x{C}x{H}x{W} K={K} s={stride}")
    return d


@functools.lru_cache(maxsize=None)
def blur_dk_reference(N, C, H, W, K, stride):
    c = kgrad_case(N, C, H, W, K, stride)
    dk = blur_dk_ref(c["dy"], c["x"], K, stride)
    what = f"blur_bwd_kernel {N}x{C}x{H}x{W} K={K} s={stride}"
    assert_on_lattice(dk, 1.0, what)
    assert_fp32_exact(dk, what)
    return c, dk


# ------------------------------------------------------------------------------------------- blur case tables
# (N, C, H, W, K, stride) -- the smallest shapes that cross each seam

S1_SHAPES = [
    (2, 3, 33, 131, 21, 1),         # stride-1 tiles (16 x 128): 3 x 2, the last one 1 row x 3 columns; W % 8 != 0 (the ix + e < W guard)
    (1, 1, 1, 1, 21, 1),            # tiny: one pixel, the centre tap alone
    (2, 3, 5, 3, 21, 1),            # tiny: smaller than the halo in both directions
]
BLUR_FWD = S1_SHAPES + [
    (2, 3, 70, 67, 21, 4),          # generic kernel: OH x OW = 18 x 17, ragged 16 x 16 tiles in both directions
    (1, 3, 35, 37, 21, 2),          # generic kernel, stride 2, odd sizes: 18 x 19 outputs
    (1, 3, 137, 130, 21, 8),        # generic kernel, stride 8: the > 48 KB LDS opt-in (141^2 window), 18 x 17 outputs
    (2, 3, 33, 40, 7, 1),           # K = 7: generic kernel at stride 1, 3 x 3 tiles
    (2, 3, 33, 40, 5, 1),           # K = 5: generic kernel at stride 1
    (2, 3, 68, 72, 7, 4),           # K = 7 at stride 4: 17 x 18 outputs
]
FWD_VARIANTS = ["y32", "y32_sub", "y16", "both"]
Y16_LD = 8                          # KBPN's NHWC pixels are 8 halves wide; lanes C .. 7 must keep their sentinel

BLUR_BWD_INPUT = S1_SHAPES + [
    (2, 3, 68, 72, 21, 4),          # stride-4 kernel: 17 x 18 low-resolution positions = 2 x 2 tiles of 16, ragged both ways
    (2, 3, 70, 67, 21, 4),          # H != 4 OH and W % 4 != 0: falls through to the generic kernel
    (2, 3, 68, 70, 21, 4),          # W != 4 OW alone: falls through to the generic kernel
    (1, 3, 35, 37, 21, 2),          # generic, stride 2
    (1, 3, 137, 130, 21, 8),        # generic, stride 8
    (2, 3, 33, 40, 7, 1),           # generic, K = 7
    (2, 3, 33, 40, 5, 1),           # generic, K = 5
    (2, 3, 68, 72, 7, 4),           # generic, K = 7 at stride 4 (the stride-4 kernel is built for 21 only)
    (1, 3, 840, 840, 7, 1),         # generic, grid-stride wrap: 2 116 800 elements > 8192 x 256 threads
]
BLUR_BWD_KERNEL = [
    (2, 3, 70, 97, 21, 1),          # stride-1 kernel, ragged 32 x 32 tiles (3 x 4)
    (2, 3, 585, 590, 21, 1),        # 3 x 19 x 19 = 1083 tiles -> tiles_per_wg = 2, 542 workgroups, the last holds one tile, one spans a channel boundary
    (2, 3, 585, 590, 7, 1),         # the same through the generic kernel
    (1, 3, 35, 37, 21, 2),          # generic, TO = 16
    (2, 3, 70, 67, 21, 4),          # generic, TO = 16
    (1, 3, 137, 130, 21, 8),        # generic, TO = 8: 18 x 17 outputs = 3 x 3 tiles
    (2, 3, 33, 40, 5, 1),           # generic, K = 5, TO = 32
]
REFUSED_K = 9                       # not built by BLUR_DISPATCH


def blur_geometry(entry, N, C, H, W, K, stride):
    """what a row exercises, from the transcription and the tile constants: kernel, tiles (y, x), tiles_per_wg, workgroups per sample,
    whether a workgroup spans a channel boundary, whether the last one is partly filled, whether the grid wraps"""
    t = tile_constants()
    name, tpw = blur_kernel_for(entry, K, stride, H, W, C)
    OH, OW = out_size(H, K, stride), out_size(W, K, stride)
    g = dict(kernel=name, tpw=tpw, OH=OH, OW=OW, wraps=False)
    if name.startswith("blur_bwd_input_s1"):
        g["tiles"] = ((H + t["TR"] - 1) // t["TR"], (W + t["TC"] - 1) // t["TC"])
        g["last_tile"] = (H - (g["tiles"][0] - 1) * t["TR"], W - (g["tiles"][1] - 1) * t["TC"])
    elif name == "blur_bwd_input_s4_kernel":
        g["tiles"] = ((OH + t["TL"] - 1) // t["TL"], (OW + t["TL"] - 1) // t["TL"])
    elif name == "blur_fwd_kernel":
        g["tiles"] = ((OH + t["FT"] - 1) // t["FT"], (OW + t["FT"] - 1) // t["FT"])
        g["lds_bytes"] = (K * K + (15 * stride + K) ** 2) * 4
    elif name == "blur_bwd_input_kernel":
        g["wraps"] = grid_wraps(N * C * H * W)
    else:
        TO = t["TO"][stride]
        g["tiles"] = ((OH + TO - 1) // TO, (OW + TO - 1) // TO)
        per_plane = g["tiles"][0] * g["tiles"][1]
        total = C * per_plane
        g["workgroups"] = (total + tpw - 1) // tpw
        g["last_wg_tiles"] = total - (g["workgroups"] - 1) * tpw
        g["spans_channels"] = any((w * tpw) // per_plane != (min(w * tpw + tpw, total) - 1) // per_plane for w in range(g["workgroups"]))
    return g


# ------------------------------------------------------------------------------------------- blur mutants

BLUR_MUTANTS = ["flip", "transpose", "other_sample", "replicate", "corner00", "cornerKK", "last_row", "last_col", "origin", "planes"]


def blur_mutant_applies(name, N, C, H, W, K, stride):
    """can this mutant change this row at all?  (a 1 x 1 image only ever meets the centre tap; one sample has no other sample ...)"""
    P = (K - 1) // 2
    OH, OW = out_size(H, K, stride), out_size(W, K, stride)
    if name == "other_sample":
        return N >= 2
    if name == "planes":
        return C >= 2
    if name == "flip":
        return H * W > 1
    if name == "transpose":
        return H > 1 and W > 1
    if name == "corner00":          # some window reaches its first tap inside the image
        return (OH - 1) * stride >= P and (OW - 1) * stride >= P
    if name == "cornerKK":          # output 0 reaches its last tap inside the image
        return H - 1 >= P and W - 1 >= P
    return True


def _mut_taps(name, k, K):
    k = _k3(k, K).clone()
    if name == "flip":
        return k.flip(1, 2)
    if name == "transpose":
        return k.transpose(1, 2)
    if name == "other_sample":
        return k.roll(1, 0)
    if name == "corner00":
        k[:, 0, 0] = 0
    if name == "cornerKK":
        k[:, K - 1, K - 1] = 0
    return k


def _drop_last(t, name):
    t = torch.as_tensor(t, dtype=torch.float64).clone()
    if name == "last_row":
        t[:, :, -1, :] = 0
    else:
        t[:, :, :, -1] = 0
    return t


def blur_mutant(op, name, case, K, stride, ref):
    """the result a subtly wrong kernel would give: ``op`` in 'fwd', 'dx', 'dk'; ``ref`` is the right result of the same case (a few
    mutants are transformations of it).  flip / transpose: taps flipped both ways / transposed; other_sample: the next sample's kernel;
    replicate: edge replication instead of zero padding; corner00 / cornerKK: that tap dropped; last_row / last_col: the last output
    row / column not produced (forward) or not read (adjoints); origin: the window starts one pixel early; planes: channel planes
    swapped."""
    x, k, dy = case["x"], case.get("k"), case["dy"]
    H, W = x.shape[-2:]
    ref = torch.as_tensor(ref, dtype=torch.float64)
    opt = dict(pad="replicate") if name == "replicate" else (dict(origin=1) if name == "origin" else {})
    tapm = name in ("flip", "transpose", "other_sample", "corner00", "cornerKK")
    if op == "fwd":
        if tapm:
            return blur_ref(x, _mut_taps(name, k, K), K, stride)
        if opt:
            return blur_ref(x, k, K, stride, **opt)
        return ref.flip(1) if name == "planes" else _drop_last(ref, name)
    if op == "dx":
        if tapm:
            return blur_dx_ref(dy, _mut_taps(name, k, K), K, stride, H, W)
        if opt:
            return blur_dx_ref(dy, k, K, stride, H, W, **opt)
        return ref.flip(1) if name == "planes" else blur_dx_ref(_drop_last(dy, name), k, K, stride, H, W)
    assert op == "dk"
    if tapm:          # the gradient of a mutated tap lands in the mutated place
        r = ref.clone()
        if name in ("corner00", "cornerKK"):
            i = 0 if name == "corner00" else K - 1
            r[:, i, i] = 0
            return r
        return _mut_taps(name, r, K)
    if opt:
        return blur_dk_ref(dy, x, K, stride, **opt)
    if name == "planes":
        return blur_dk_ref(dy, torch.as_tensor(x).flip(1), K, stride)
    return blur_dk_ref(_drop_last(dy, name), x, K, stride)


# ------------------------------------------------------------------------------------------- bicubic axis operators

def down_matrix(n, f, antialias, A=None, normalise=True, shift=0, fold=True):
    """fp64 [n // f, n]: the axis operator of the down-scale by f.  A / normalise / shift / fold exist for the mutants."""
    on = n // f
    M = np.zeros((on, n), dtype=np.float64)
    for o in range(on):
        if antialias:
            a = -0.5 if A is None else A
            c = f * (o + 0.5)
            lo, hi = max(int(c - 2 * f + 0.5) + shift, 0), min(int(c + 2 * f + 0.5) + shift, n)
            w = np.array([cub((j - c + 0.5) / f, a) for j in range(lo, hi)], dtype=np.float64)
            M[o, lo:hi] = w / w.sum() if normalise else w / f
        else:
            a = -0.75 if A is None else A
            s = (o + 0.5) * f - 0.5
            b = math.floor(s)
            t = s - b
            for j, wj in enumerate((cub(t + 1.0, a), cub(t, a), cub(1.0 - t, a), cub(2.0 - t, a))):
                i = b - 1 + j + shift
                if fold:
                    M[o, min(max(i, 0), n - 1)] += wj
                elif 0 <= i < n:
                    M[o, i] += wj
    return M


def up_add_matrix(n, s, A=-0.75, shift=0, fold=True):
    """fp64 [n s, n]: the axis operator of the up-scale by s (align_corners=False, four taps with clamped indices)"""
    M = np.zeros((n * s, n), dtype=np.float64)
    for o in range(n * s):
        c = (o + 0.5) / s - 0.5
        b = math.floor(c)
        t = c - b
        for j, wj in enumerate((cub(t + 1.0, A), cub(t, A), cub(1.0 - t, A), cub(2.0 - t, A))):
            i = b - 1 + j + shift
            if fold:
                M[o, min(max(i, 0), n - 1)] += wj
            elif 0 <= i < n:
                M[o, i] += wj
    return M


def sep(My, x, Mx):
    """M_y x M_x^T over the last two axes, fp64 numpy"""
    return My @ np.asarray(x, dtype=np.float64) @ Mx.T


def sep_adj(My, dy, Mx):
    """M_y^T dy M_x"""
    return My.T @ np.asarray(dy, dtype=np.float64) @ Mx


def sep32(My, x, Mx, reverse=False, adjoint=False):
    """the same in fp32, tap by tap -- rows first, then columns, each sum in ascending (or with reverse=True descending) tap order: an
    emulation of a kernel's arithmetic in a summation order of the caller's choice"""
    My, Mx = (My.T, Mx.T) if adjoint else (My, Mx)
    My32, Mx32, x = My.astype(np.float32), Mx.astype(np.float32), np.asarray(x, dtype=np.float32)
    assert np.array_equal(My32.astype(np.float64), My) and np.array_equal(Mx32.astype(np.float64), Mx), "weights are not fp32 values"
    order = (lambda n: range(n - 1, -1, -1)) if reverse else range
    r = np.zeros(x.shape[:-1] + (Mx.shape[0],), np.float32)
    for j in order(Mx.shape[1]):
        r = r + x[..., :, j:j + 1] * Mx32[:, j]
    y = np.zeros(x.shape[:-2] + (My.shape[0], Mx.shape[0]), np.float32)
    for j in order(My.shape[1]):
        y = y + My32[:, j:j + 1] * r[..., j:j + 1, :]
    return y


def abs_bound(My, x, Mx, adjoint=False):
    """|M_y| |x| |M_x|^T (or its adjoint form): what every per-element rounding bound is a multiple of"""
    return (sep_adj if adjoint else sep)(np.abs(My), np.abs(np.asarray(x, dtype=np.float64)), np.abs(Mx))


def _prove_exact(My, x, Mx, unit_w, unit_x, what, adjoint=False, extra=None):
    """both passes of a separable resize are exact in fp32 in any order: weights on unit_w, x on unit_x, the row pass below 2^24 units of
    unit_w unit_x and the result (plus |extra|) below 2^24 units of unit_w^2 unit_x -- and, as a cross-check, the fp64 results of both
    stages are fp32 values"""
    for M in (My, Mx):
        assert_on_lattice(torch.from_numpy(M), unit_w, what + " weights")
    assert_on_lattice(torch.as_tensor(np.asarray(x)), unit_x, what + " input")
    ax = np.abs(np.asarray(x, dtype=np.float64))
    row = ax @ np.abs(Mx) if adjoint else ax @ np.abs(Mx).T
    assert row.max() / (unit_w * unit_x) < FP32_EXACT, f"{what}: the row pass reaches {row.max() / (unit_w * unit_x):.3g} units >= 2^24"
    tot = abs_bound(My, x, Mx, adjoint) + (0 if extra is None else np.abs(np.asarray(extra, dtype=np.float64)))
    assert tot.max() / (unit_w * unit_w * unit_x) < FP32_EXACT, f"{what}: the result reaches {tot.max() / (unit_w ** 2 * unit_x):.3g} units >= 2^24"
    xr = np.asarray(x, np.float64) @ Mx if adjoint else np.asarray(x, np.float64) @ Mx.T
    assert_fp32_exact(torch.from_numpy(xr), what + " row pass")
    res = (sep_adj if adjoint else sep)(My, x, Mx) + (0 if extra is None else np.asarray(extra, np.float64))
    assert_fp32_exact(torch.from_numpy(res), what)
    return res


# ------------------------------------------------------------------------------------------- bicubic case tables

# (planes, H, W, f)
DOWN_CASES = [
    (6, 32, 40, 4),                 # the shape of test_bicubic_resizes
    (3, 12, 20, 2),                 # f = 2 (not antialiased: the one even factor whose first tap clamps)
    (3, 48, 24, 8),                 # f = 8
    (2, 8, 4, 4),                   # 2 x 1 outputs: every table candidate index clamped, every antialiased tap set cut
    (1, 2, 2, 2),                   # a single output
    (3, 1024, 768, 4),              # backward grid-stride wrap: 2 359 296 elements > 8192 x 256 threads
    (1, 24, 28, 2),                 # f = 2 with an interior in both directions (12 x 14 outputs): the antialiased bound is tightest there
    (1, 80, 88, 8),                 # f = 8 with an interior in both directions (10 x 11 outputs)
]
# (planes, H, W, scale)
UP_CASES = [(6, 9, 7, 4), (3, 5, 6, 2), (3, 1, 1, 4), (2, 5, 6, 8)]
FALLBACK_CASES = [(6, 32, 40, 4), (2, 8, 4, 4)]          # the per-pixel antialiased backward (no reduction scratch registered)
UP8_ROUNDINGS = 17          # per axis a 4-term dot product: 4 products + 4 additions (weights are exact multiples of 2^-14); + the add into out


def aa_roundings(f, border, accumulate=False):
    """n of the antialiased bound |got - ref| <= n 2^-24 |M_y| |x| |M_x|^T, by counting roundings.  Per axis a sum over at most 4 f + 1
    taps: at most 4 f + 1 additions and as many products on the way of any one term -> 2 (4 f + 1) per axis.  In the interior (outputs
    2 .. n / f - 3) that is all: the fp32 weights equal the fp64 ones bit for bit and the tap sum is exactly f.  A weight of a cut tap
    set adds, per axis, the 4 f + 1 additions of its normalising sum, the reciprocal, the product with it, and 6 operations of the
    cubic: 4 f + 9.  One more for the add into an existing gradient."""
    n = 2 * 2 * (4 * f + 1) + (2 * (4 * f + 9) if border else 0)
    return n + (1 if accumulate else 0)


def interior_mask(M, adjoint=False):
    """forward: outputs 2 .. on - 3 (the whole support inside the image); adjoint: the inputs that only such outputs touch"""
    on = M.shape[0]
    o_int = np.zeros(on, bool)
    o_int[2:max(on - 2, 2)] = True
    if not adjoint:
        return o_int
    return np.array([bool(o_int[np.nonzero(M[:, i])[0]].all()) for i in range(M.shape[1])])


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


@functools.lru_cache(maxsize=None)
def down_case(planes, H, W, f, antialias):
    """dict for one csbsr_aa_bicubic_down row: x, dy, dx0 (fp32), My, Mx, the fp64 references y, dx, and per direction either
    exact=True (proved) or the |M| |x| |M|^T arrays of the bound"""
    rng = _rng(planes, H, W, f, antialias)
    My, Mx = down_matrix(H, f, antialias), down_matrix(W, f, antialias)
    OH, OW = H // f, W // f
    what = f"down {planes}x{H}x{W} f={f} aa={antialias}"
    d = dict(My=My, Mx=Mx)
    if antialias:
        d["x"] = (rng.random((planes, H, W)) * 2 - 1).astype(np.float32)
        d["dy"] = (rng.random((planes, OH, OW)) * 2 - 1).astype(np.float32)
        d["dx0"] = (rng.random((planes, H, W)) * 2 - 1).astype(np.float32)
        d["y"], d["dx"] = sep(My, d["x"], Mx), sep_adj(My, d["dy"], Mx)
        d["y_abs"], d["dx_abs"] = abs_bound(My, d["x"], Mx), abs_bound(My, d["dy"], Mx, adjoint=True)
        d["exact"] = False
    else:
        lat = lambda shape: (rng.integers(-15, 16, size=shape) / 16.0).astype(np.float32)
        d["x"], d["dy"], d["dx0"] = lat((planes, H, W)), lat((planes, OH, OW)), lat((planes, H, W))
        d["y"] = _prove_exact(My, d["x"], Mx, 2.0 ** -5, 2.0 ** -4, what)
        d["dx"] = _prove_exact(My, d["dy"], Mx, 2.0 ** -5, 2.0 ** -4, what + " adjoint", adjoint=True)
        _prove_exact(My, d["dy"], Mx, 2.0 ** -5, 2.0 ** -4, what + " adjoint, accumulated", adjoint=True, extra=d["dx0"])
        d["exact"] = True
    for name, v in d.items():          # the shared references are read-only (the inputs go through torch, which wants writable arrays)
        if isinstance(v, np.ndarray) and name not in ("x", "dy", "dx0", "out0"):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def up_case(planes, H, W, s):
    """dict for one csbsr_bicubic_up_add row: x, out0, M_y, M_x, the fp64 reference out = out0 + M_y x M_x^T, exact or its bound"""
    rng = _rng(planes, H, W, s, 5)
    My, Mx = up_add_matrix(H, s), up_add_matrix(W, s)
    what = f"up_add {planes}x{H}x{W} s={s}"
    d = dict(My=My, Mx=Mx, exact=s in (2, 4))
    shape, oshape = (planes, H, W), (planes, H * s, W * s)
    if s == 2:
        d["x"], d["out0"] = rng.integers(-15, 16, size=shape).astype(np.float32), rng.integers(-15, 16, size=oshape).astype(np.float32)
        d["out"] = _prove_exact(My, d["x"], Mx, 2.0 ** -8, 1.0, what, extra=d["out0"])
    elif s == 4:
        d["x"], d["out0"] = rng.integers(-1, 2, size=shape).astype(np.float32), rng.integers(-2, 3, size=oshape).astype(np.float32)
        if H * W == 1:
            d["x"][:] = 1.0
        d["out"] = _prove_exact(My, d["x"], Mx, 2.0 ** -11, 1.0, what, extra=d["out0"])
    else:
        d["x"], d["out0"] = (rng.random(shape) * 2 - 1).astype(np.float32), (rng.random(oshape) * 2 - 1).astype(np.float32)
        d["out"] = sep(My, d["x"], Mx) + d["out0"].astype(np.float64)
        d["out_abs"] = abs_bound(My, d["x"], Mx) + np.abs(d["out0"].astype(np.float64))
    for name, v in d.items():          # the shared references are read-only (the inputs go through torch, which wants writable arrays)
        if isinstance(v, np.ndarray) and name not in ("x", "dy", "dx0", "out0"):
            v.setflags(write=False)
    return d


# ---- the kernel's weight formulas in fp32 (numpy scalars keep every operation in fp32)

def _aa_filter32(x):
    f32 = np.float32
    A, x = f32(-0.5), np.abs(f32(x))
    if x < f32(1):
        return ((A + f32(2)) * x - (A + f32(3))) * x * x + f32(1)
    if x < f32(2):
        return (((x - f32(5)) * x + f32(8)) * x - f32(4)) * A
    return f32(0)


def aa_weights32(n, f):
    """fp32 [n // f, n]: aa_range / aa_filter of csrc/image_ops.hip operation by operation (the taps' sum in ascending order)"""
    f32 = np.float32
    M = np.zeros((n // f, n), np.float32)
    for o in range(n // f):
        scale = f32(f)
        center = scale * (f32(o) + f32(0.5))
        support = f32(2) * scale
        lo, hi = max(int(center - support + f32(0.5)), 0), min(int(center + support + f32(0.5)), n)
        tot = f32(0)
        for k in range(lo, hi):
            tot = tot + _aa_filter32((f32(k) - center + f32(0.5)) / scale)
        norm = f32(1) / tot
        for k in range(lo, hi):
            M[o, k] = _aa_filter32((f32(k) - center + f32(0.5)) / scale) * norm
    return M


# ---- bicubic mutants: the reference with one thing wrong

BICUBIC_MUTANTS = ["wrong_A", "no_norm", "shift", "drop_clamped", "adjoint_M"]


def bicubic_mutant_applies(name, kind, n_y, n_x, f, antialias):
    """``kind`` in 'down', 'down_adj', 'up'.  no_norm: the antialiased filter only (its first and last tap sets are always cut).
    drop_clamped: where an index clamps -- every up-scale, the non-antialiased down-scale at f = 2 (taps 2 o - 1 .. 2 o + 2; at f >= 4
    the taps f o + f / 2 - 2 .. + 1 stay inside).  adjoint_M: the adjoint only."""
    if name == "no_norm" and not (antialias and kind != "up"):
        return False
    if name == "drop_clamped" and not (kind == "up" or (not antialias and f == 2)):
        return False
    if name == "adjoint_M" and kind != "down_adj":
        return False
    # ... and the mutant's operator has to differ from the right one at this size: a one-pixel axis has the single weight 1 under every
    # rule, a two-tap output is (.5, .5) by symmetry whatever A is, a tap range that covers the whole axis cannot shift
    right = (up_add_matrix(n_y, f), up_add_matrix(n_x, f)) if kind == "up" else (down_matrix(n_y, f, antialias), down_matrix(n_x, f, antialias))
    wrong = bicubic_mutant_matrices(name, kind, n_y, n_x, f, antialias)
    return not (np.allclose(right[0], wrong[0], rtol=0, atol=1e-12) and np.allclose(right[1], wrong[1], rtol=0, atol=1e-12))


def bicubic_mutant_matrices(name, kind, n_y, n_x, f, antialias):
    """(M_y, M_x) of the mutant.  wrong_A: A = -0.75 in the antialiased filter and -0.5 in the other rules; no_norm: weights divided by f,
    not by their in-image sum; shift: the tap range one pixel late; drop_clamped: an out-of-image tap dropped, not folded onto the
    border; adjoint_M: the adjoint built from the forward operator of the OPPOSITE resize (the up-scale's M in place of the down-scale's
    M^T -- the two differ everywhere: a down-scale's adjoint is not an up-scale), returned transposed so that sep_adj applies."""
    def m(n):
        if kind == "up":
            kw = dict(wrong_A=dict(A=-0.5), shift=dict(shift=1), drop_clamped=dict(fold=False))[name]
            return up_add_matrix(n, f, **kw)
        if name == "adjoint_M":
            return up_add_matrix(n // f, f).T / f
        kw = dict(wrong_A=dict(A=-0.75 if antialias else -0.5), no_norm=dict(normalise=False), shift=dict(shift=1), drop_clamped=dict(fold=False))[name]
        return down_matrix(n, f, antialias, **kw)
    return m(n_y), m(n_x)


# ------------------------------------------------------------------------------------------- coverage

# rows (test names of tests/test_image_exact_gpu.py) per C entry point and per __global__ kernel of the blur and bicubic sections
CASES = {
    "csbsr_blur_fwd": ["test_blur_fwd_exact", "test_blur_refuses_other_kernel_sizes", "test_blur_refuses_null"],
    "csbsr_blur_bwd_input": ["test_blur_bwd_input_exact", "test_blur_refuses_other_kernel_sizes", "test_blur_refuses_null"],
    "csbsr_blur_bwd_kernel": ["test_blur_bwd_kernel_exact", "test_blur_refuses_other_kernel_sizes", "test_blur_refuses_null"],
    "csbsr_bicubic_up_add": ["test_bicubic_up_add"],
    "csbsr_aa_bicubic_down_fwd": ["test_bicubic_down_fwd"],
    "csbsr_aa_bicubic_down_bwd": ["test_bicubic_down_bwd", "test_aa_down_bwd_without_scratch"],
    "blur_fwd_kernel": ["test_blur_fwd_exact"],
    "blur_bwd_input_kernel": ["test_blur_bwd_input_exact"],
    "blur_bwd_input_s1_kernel": ["test_blur_fwd_exact", "test_blur_bwd_input_exact"],
    "blur_bwd_input_s4_kernel": ["test_blur_bwd_input_exact"],
    "blur_bwd_kernel_kernel": ["test_blur_bwd_kernel_exact"],
    "blur_bwd_kernel_s1_kernel": ["test_blur_bwd_kernel_exact"],
    "bicubic_up_add_kernel": ["test_bicubic_up_add"],
    "aa_down_fwd_kernel": ["test_bicubic_down_fwd"],
    "aa_down_bwd_kernel": ["test_bicubic_down_bwd", "test_aa_down_bwd_without_scratch"],
    "aa_weight_tables_kernel": ["test_bicubic_down_bwd"],
    "aa_down_bwd_tab_kernel": ["test_bicubic_down_bwd"],
}
NOT_COVERED = {}          # name -> the written reason (six words at least) why it has no row
# A branch no row can reach, for the record: the ``wide`` path of aa_down_bwd_kernel needs more than seven candidate outputs for one
# input pixel, but the candidates are i / f - 3 .. i / f + 3 and the border rules of the non-antialiased resize only narrow that range
# (to 0 .. 3 or OW - 4 .. OW - 1), so ``ox_hi - ox_lo > 6`` is false for every shape; the 8 x 4 and 2 x 2 rows run the clamped-border
# code next to it.


def covered_names():
    """every extern "C" blur / bicubic-down / up_add entry point of image_ops.hip and every __global__ kernel of the blur and bicubic sections"""
    entries = [n for n in re.findall(r'extern "C" int (csbsr_\w+)', source())
               if n.startswith("csbsr_blur_") or n.startswith("csbsr_aa_bicubic_down_") or n == "csbsr_bicubic_up_add"]
    kernels = re.findall(r"__global__(?: __launch_bounds__\(\d+\))? void (\w+)\(", blur_section() + bicubic_section())
    assert len(kernels) == (blur_section() + bicubic_section()).count("__global__"), "a __global__ line the pattern does not parse"
    return entries, kernels


def missing_names(cases=None, not_covered=None):
    cases, not_covered = CASES if cases is None else cases, NOT_COVERED if not_covered is None else not_covered
    entries, kernels = covered_names()
    return [n for n in entries + kernels if not cases.get(n) and n not in not_covered]
