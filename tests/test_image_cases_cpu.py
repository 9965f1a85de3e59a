"""The references, input builders, case tables and mutants of tests/image_cases.py, checked before any kernel is involved (no GPU):

  * the fp64 references agree, to fp64 rounding, with independent ones: the oracle's blur_down and its autograd, a per-sample
    F.conv2d, and F.interpolate(bicubic, antialias=...) in fp64 with its autograd, for every table row;
  * every lattice builder's proof passes for every row, and an fp32 evaluation in ANOTHER summation order (taps in descending order)
    gives the same bits as the fp64 reference -- the property the GPU module's bit-equality rests on;
  * an fp32 evaluation of the kernel's antialiased weight formulas equals the fp64 weights bit for bit in the interior (outputs
    2 .. n / f - 3) and stays within 1.7e-8 at the cut borders;
  * every mutant of the references changes the result of every row it applies to: at least one element on the exact classes, more than
    10 x the row's tolerance on the bounded ones -- so the inputs can tell a subtly wrong kernel from a right one;
  * the case tables cross the seams they name (tile sizes read from csrc/image_ops.hip), the dispatch restatement visits every blur
    kernel, reaches tiles_per_wg >= 2 in both kernel-gradient kernels and the grid-stride wrap of the generic input gradient;
  * every entry point and every __global__ kernel of the blur and bicubic sections has a row in CASES or a written reason.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_cases as I
from exact_lattice import mismatch

HEAVY = 200 * 200          # rows above this many pixels per plane take the cheaper of two equivalent checks where one is offered


def _id(r):
    return "x".join(str(v) for v in r)


# ------------------------------------------------------------------------------------------- tables and dispatch

def test_tile_constants_are_the_ones_the_tables_assume():
    t = I.tile_constants()
    assert (t["TR"], t["TC"], t["TL"], t["FT"]) == (16, 128, 16, 16), f"retiled: {t}: rebuild the case tables of tests/image_cases.py"
    assert t["TO"] == {1: 32, 2: 16, 4: 16, 8: 8} and (t["BLOCK"], t["CAP"], t["WGS"]) == (256, 8192, 1024), f"retiled: {t}"


def test_forward_rows_cross_their_seams():
    g = {r: I.blur_geometry("fwd", *r) for r in I.BLUR_FWD}
    for r in I.S1_SHAPES:
        assert g[r]["kernel"] == "blur_bwd_input_s1_kernel<FWD>"
    a = g[(2, 3, 33, 131, 21, 1)]
    assert a["tiles"] == (3, 2) and a["last_tile"] == (1, 3) and 131 % 8 != 0
    for r in I.BLUR_FWD[3:]:
        assert g[r]["kernel"] == "blur_fwd_kernel"
    b = g[(2, 3, 70, 67, 21, 4)]
    assert (b["OH"], b["OW"]) == (18, 17) and b["tiles"] == (2, 2)
    assert g[(1, 3, 137, 130, 21, 8)]["lds_bytes"] > 48 * 1024 and all(g[r]["lds_bytes"] <= 48 * 1024 for r in I.BLUR_FWD[3:] if r[5] != 8)
    assert {(r[4], r[5]) for r in I.BLUR_FWD} >= {(21, 1), (21, 2), (21, 4), (21, 8), (7, 1), (5, 1), (7, 4)}


def test_input_gradient_rows_cross_their_seams():
    g = {r: I.blur_geometry("bwd_input", *r) for r in I.BLUR_BWD_INPUT}
    want = ["blur_bwd_input_s1_kernel<BWD>"] * 3 + ["blur_bwd_input_s4_kernel"] + ["blur_bwd_input_kernel"] * 8
    assert [g[r]["kernel"] for r in I.BLUR_BWD_INPUT] == want
    assert g[(2, 3, 33, 131, 21, 1)]["tiles"] == (3, 2)
    s4 = g[(2, 3, 68, 72, 21, 4)]
    assert s4["tiles"] == (2, 2) and s4["OH"] % 16 and s4["OW"] % 16
    assert [r for r in I.BLUR_BWD_INPUT if g[r]["wraps"]] == [(1, 3, 840, 840, 7, 1)]
    assert {(r[4], r[5]) for r in I.BLUR_BWD_INPUT if g[r]["kernel"] == "blur_bwd_input_kernel"} >= {(21, 4), (21, 2), (21, 8), (7, 1), (5, 1), (7, 4)}


def test_kernel_gradient_rows_cross_their_seams():
    g = {r: I.blur_geometry("bwd_kernel", *r) for r in I.BLUR_BWD_KERNEL}
    a = g[(2, 3, 70, 97, 21, 1)]
    assert a["kernel"] == "blur_bwd_kernel_s1_kernel" and a["tiles"] == (3, 4) and 70 % 32 and 97 % 32 and a["tpw"] == 1
    for r, name in (((2, 3, 585, 590, 21, 1), "blur_bwd_kernel_s1_kernel"), ((2, 3, 585, 590, 7, 1), "blur_bwd_kernel_kernel")):
        b = g[r]
        assert b["kernel"] == name and b["tiles"] == (19, 19) and b["tpw"] == 2 and b["workgroups"] == 542
        assert b["last_wg_tiles"] == 1 and b["spans_channels"]
    assert {r[5] for r in I.BLUR_BWD_KERNEL if g[r]["kernel"] == "blur_bwd_kernel_kernel"} == {1, 2, 4, 8}
    assert (2, 3, 33, 40, 5, 1) in g


def test_dispatch_restatement_visits_every_kernel():
    seen = {I.blur_kernel_for(e, r[4], r[5], r[2], r[3], r[1])[0]
            for e, rows in (("fwd", I.BLUR_FWD), ("bwd_input", I.BLUR_BWD_INPUT), ("bwd_kernel", I.BLUR_BWD_KERNEL)) for r in rows}
    assert seen == set(I.BLUR_KERNEL_NAMES)
    tpw = {}
    for r in I.BLUR_BWD_KERNEL:
        name, t = I.blur_kernel_for("bwd_kernel", r[4], r[5], r[2], r[3], r[1])
        tpw[name] = max(tpw.get(name, 0), t)
    assert tpw == {"blur_bwd_kernel_s1_kernel": 2, "blur_bwd_kernel_kernel": 2}
    with pytest.raises(AssertionError):
        I.blur_kernel_for("fwd", I.REFUSED_K, 1, 8, 8, 3)
    assert "case 21" in I.source() and "case 7" in I.source() and "case 5" in I.source() and f"case {I.REFUSED_K}:" not in I.source()


def test_bicubic_rows_cross_their_seams():
    assert {r[3] for r in I.DOWN_CASES} == {2, 4, 8} and {r[3] for r in I.UP_CASES} == {2, 4, 8}
    assert any(r[1] // r[3] < 7 and r[2] // r[3] < 7 for r in I.DOWN_CASES) and (1, 2, 2, 2) in I.DOWN_CASES
    big = [r for r in I.DOWN_CASES if I.grid_wraps(r[0] * r[1] * r[2])]
    assert big == [(3, 1024, 768, 4)]
    assert not any(I.grid_wraps(r[0] * (r[1] // r[3]) * (r[2] // r[3])) for r in I.DOWN_CASES)          # the forward's grid never wraps at a testable size
    assert set(I.FALLBACK_CASES) <= set(I.DOWN_CASES)
    for f in (2, 4, 8):          # every factor has a row with interior outputs AND interior inputs: the tighter bound is exercised both ways
        for adjoint in (False, True):
            assert any(r[3] == f and all(I.interior_mask(I.down_matrix(n, f, True), adjoint).any() for n in r[1:3]) for r in I.DOWN_CASES), (f, adjoint)


def test_coverage_table_has_no_missing_entry():
    entries, kernels = I.covered_names()
    assert len(entries) == 6 and len(kernels) == 11, (entries, kernels)
    assert I.missing_names() == []
    assert I.missing_names(cases={}, not_covered={}) == entries + kernels
    for name, why in I.NOT_COVERED.items():
        assert len(why.split()) >= 6, f"NOT_COVERED[{name}]: write the reason out"
    with open(os.path.join(I.ROOT, "tests", "test_image_exact_gpu.py")) as f:
        src = f.read()
    for name, rows in I.CASES.items():
        for r in rows:
            assert f"\ndef {r}(" in src, f"CASES[{name}] names {r}, which tests/test_image_exact_gpu.py does not define"
        if name.startswith("csbsr_"):
            assert f'"{name}"' in src, f"tests/test_image_exact_gpu.py never calls {name}"


# ------------------------------------------------------------------------------------------- blur references

def _conv_per_sample(x, k, K, s):
    P = (K - 1) // 2
    return torch.stack([F.conv2d(x[n].unsqueeze(1), k[n].reshape(1, 1, K, K), stride=s, padding=P).squeeze(1) for n in range(x.shape[0])])


@pytest.mark.parametrize("row", sorted(set(I.BLUR_FWD + I.BLUR_BWD_INPUT + I.BLUR_BWD_KERNEL)), ids=_id)
def test_blur_references_agree_with_the_oracle_and_conv2d(row):
    """blur_ref / blur_dx_ref / blur_dk_ref against the oracle's blur_down with autograd, and against one F.conv2d per sample, on
    fp64 noise.  On the lattice inputs fp64 is exact, so there the agreement is asked bit for bit (forward)."""
    from oracle import csbsr_oracle as O
    N, C, H, W, K, s = row
    gen = torch.Generator().manual_seed(H * W + K)
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64).requires_grad_(True)
    k = torch.randn(N, K * K, generator=gen, dtype=torch.float64).requires_grad_(True)
    y = O.blur_down(x, k, K, s)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(dy)
    mine = I.blur_ref(x.detach(), k.detach(), K, s)
    scale = float(y.detach().abs().max())
    assert mine.shape == y.shape and float((mine - y.detach()).abs().max()) <= 1e-12 * scale
    assert float((mine - _conv_per_sample(x.detach(), k.detach(), K, s)).abs().max()) <= 1e-12 * scale
    dx = I.blur_dx_ref(dy, k.detach(), K, s, H, W)
    assert float((dx - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    dk = I.blur_dk_ref(dy, x.detach(), K, s).reshape(N, K * K)
    assert float((dk - k.grad).abs().max()) <= 1e-12 * float(k.grad.abs().max())
    c = I.blur_case(N, C, H, W, K, s)
    assert torch.equal(I.blur_ref(c["x"], c["k"], K, s), O.blur_down(c["x"].double(), c["k"].double(), K, s))


def _blur32_descending(x, k, K, s):
    """fp32 accumulation over the taps from the last to the first"""
    N, C, H, W = x.shape
    P = (K - 1) // 2
    OH, OW = I.out_size(H, K, s), I.out_size(W, K, s)
    xp = F.pad(x.float(), (P, P, P, P))
    k = k.float().reshape(N, K, K)
    y = torch.zeros(N, C, OH, OW, dtype=torch.float32)
    for ky in reversed(range(K)):
        for kx in reversed(range(K)):
            y = y + xp[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] * k[:, ky, kx].view(N, 1, 1, 1)
    return y


@pytest.mark.parametrize("row", I.BLUR_FWD, ids=_id)
def test_blur_forward_builders_and_another_order(row):
    N, C, H, W, K, s = row
    c, h, ref = I.blur_fwd_reference(*row)
    y = _blur32_descending(c["x"], c["k"], K, s)
    assert torch.equal(y.double(), ref["y32"]), mismatch(y, ref["y32"])
    assert torch.equal((y - c["sub"]).double(), ref["y32_sub"])
    yh = _blur32_descending(h["x"], h["k"], K, s)
    assert torch.equal(yh.half().double(), ref["y16"]) and torch.equal((yh - h["sub"]).half().double(), ref["both"])
    if H * W >= 64:
        assert float(ref["y16"].abs().max()) > K, "the fp16 draw never leaves the small integers: denser taps"


@pytest.mark.parametrize("row", I.BLUR_BWD_INPUT, ids=_id)
def test_blur_input_gradient_builders_and_another_order(row):
    """the adjoint as a gather from the zero-stuffed dy, in fp32, descending tap order"""
    N, C, H, W, K, s = row
    c, dx = I.blur_dx_reference(*row)
    OH, OW = c["dy"].shape[-2:]
    P = (K - 1) // 2
    Z = torch.zeros(N, C, s * (OH - 1) + 1, s * (OW - 1) + 1)
    Z[:, :, ::s, ::s] = c["dy"]
    Zp = F.pad(Z, (K - 1, K - 1 + s, K - 1, K - 1 + s))
    k = c["k"].reshape(N, K, K)
    y = torch.zeros(N, C, H, W)
    for ky in reversed(range(K)):          # dx[iy, ix] = sum Z[iy + P - ky, ix + P - kx] k[ky, kx]
        for kx in reversed(range(K)):
            a, b = P - ky + K - 1, P - kx + K - 1
            y = y + Zp[:, :, a:a + H, b:b + W] * k[:, ky, kx].view(N, 1, 1, 1)
    assert torch.equal(y.double(), dx), mismatch(y, dx)
    assert torch.equal((c["dx0"] + y).double(), dx + c["dx0"].double())


@pytest.mark.parametrize("row", I.BLUR_BWD_KERNEL, ids=_id)
def test_blur_kernel_gradient_builders_and_another_order(row):
    """fp32 sums over the pixels in torch's own (pairwise, vectorised) order, planes in descending order"""
    N, C, H, W, K, s = row
    c, dk = I.blur_dk_reference(*row)
    OH, OW = c["dy"].shape[-2:]
    P = (K - 1) // 2
    xp = F.pad(c["x"], (P, P, P, P))
    got = torch.zeros(N, K, K)
    taps = [(0, 0), (K - 1, K - 1), (P, P), (3, K - 2)] if H * W > HEAVY else [(a, b) for a in range(K) for b in range(K)]
    for ky, kx in taps:
        prod = xp[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] * c["dy"]
        acc = torch.zeros(N)
        for ch in reversed(range(C)):
            acc = acc + prod[:, ch].sum((1, 2), dtype=torch.float32)
        got[:, ky, kx] = acc
    for ky, kx in taps:
        assert torch.equal(got[:, ky, kx].double(), dk[:, ky, kx]), (ky, kx)
    assert float(dk.abs().max()) > 3, "a kernel gradient of small integers only"


# ------------------------------------------------------------------------------------------- blur mutants

def _differs(a, b):
    return a.shape != b.shape or not torch.equal(torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64))


def _blur_mutants(op, row, case, ref):
    N, C, H, W, K, s = row
    applied = []
    for name in I.BLUR_MUTANTS:
        if not I.blur_mutant_applies(name, *row):
            continue
        assert _differs(I.blur_mutant(op, name, case, K, s, ref), ref), f"{op} {row}: the mutant '{name}' survives these inputs"
        applied.append(name)
    return applied


@pytest.mark.parametrize("row", I.BLUR_FWD, ids=_id)
def test_no_blur_forward_mutant_survives(row):
    c, h, ref = I.blur_fwd_reference(*row)
    _blur_mutants("fwd", row, c, ref["y32"])
    applied = _blur_mutants("fwd", row, h, ref["y16"])
    assert len(applied) >= (2 if row[2] * row[3] == 1 else 8)


@pytest.mark.parametrize("row", I.BLUR_BWD_INPUT, ids=_id)
def test_no_blur_input_gradient_mutant_survives(row):
    c, dx = I.blur_dx_reference(*row)
    assert len(_blur_mutants("dx", row, c, dx)) >= (2 if row[2] * row[3] == 1 else 8)


@pytest.mark.parametrize("row", I.BLUR_BWD_KERNEL, ids=_id)
def test_no_blur_kernel_gradient_mutant_survives(row):
    c, dk = I.blur_dk_reference(*row)
    assert len(_blur_mutants("dk", row, c, dk)) == len(I.BLUR_MUTANTS) - (row[0] < 2)


def test_every_blur_mutant_applies_somewhere_at_every_entry_point():
    for rows in (I.BLUR_FWD, I.BLUR_BWD_INPUT, I.BLUR_BWD_KERNEL):
        for name in I.BLUR_MUTANTS:
            assert sum(I.blur_mutant_applies(name, *r) for r in rows) >= len(rows) - 4, name


# ------------------------------------------------------------------------------------------- bicubic references

def _interpolate_down(x, OH, OW, aa):
    """F.interpolate(bicubic) to (OH, OW).  The CPU implementation of the antialiased resize returns OH copies of one row when the
    OUTPUT is one pixel wide (8 x 1 -> 2 x 1 gives two equal values for any input), so that shape is resized one axis at a time, the
    second through a transposition (a pass at scale 1 is the identity: the cubic is 1 at 0 and 0 at the other integers)."""
    kw = dict(mode="bicubic", align_corners=False, antialias=aa)
    if not (aa and OW == 1 and OH > 1):
        return F.interpolate(x, size=(OH, OW), **kw)
    rows = F.interpolate(x, size=(OH, x.shape[-1]), **kw)
    return F.interpolate(rows.transpose(-1, -2).contiguous(), size=(OW, OH), **kw).transpose(-1, -2)


@pytest.mark.parametrize("aa", [1, 0])
@pytest.mark.parametrize("row", I.DOWN_CASES, ids=_id)
def test_down_reference_agrees_with_interpolate(row, aa):
    planes, H, W, f = row
    d = I.down_case(planes, H, W, f, aa)
    x = torch.from_numpy(d["x"].astype(np.float64)).unsqueeze(0).requires_grad_(True)
    y = _interpolate_down(x, H // f, W // f, bool(aa))
    y.backward(torch.from_numpy(d["dy"].astype(np.float64)).unsqueeze(0))
    assert np.abs(y.detach().numpy()[0] - d["y"]).max() <= 1e-13 * max(np.abs(d["y"]).max(), 1.0)
    assert np.abs(x.grad.numpy()[0] - d["dx"]).max() <= 1e-13 * max(np.abs(d["dx"]).max(), 1.0)


@pytest.mark.parametrize("row", I.UP_CASES, ids=_id)
def test_up_reference_agrees_with_interpolate(row):
    planes, H, W, s = row
    d = I.up_case(*row)
    up = F.interpolate(torch.from_numpy(d["x"].astype(np.float64)).unsqueeze(0), scale_factor=s, mode="bicubic", align_corners=False)
    assert np.abs(up.numpy()[0] + d["out0"] - d["out"]).max() <= 1e-13 * np.abs(d["out"]).max()


@pytest.mark.parametrize("f", [2, 4, 8])
def test_non_antialiased_weights_are_dyadic(f):
    M = I.down_matrix(12 * f, f, False)
    rows = {tuple(np.round(r[r != 0] * 32).astype(int)) for r in M}
    assert rows <= {(-3, 19, 19, -3), (16, 19, -3), (-3, 19, 16)} and np.array_equal(M * 32, np.round(M * 32))


@pytest.mark.parametrize("f", [2, 4, 8])
@pytest.mark.parametrize("n_out", [1, 2, 5, 12])
def test_antialiased_weights_fp32_equal_fp64_in_the_interior(f, n_out):
    n = n_out * f
    M, M32 = I.down_matrix(n, f, True), I.aa_weights32(n, f)
    inner = I.interior_mask(M)
    assert np.array_equal(M32[inner].astype(np.float64), M[inner]), "an interior weight rounds in fp32: the interior bound is not justified"
    assert np.abs(M32.astype(np.float64) - M).max() <= 1.7e-8
    nz = M != 0
    assert np.array_equal(M32 != 0, nz)
    rel = (np.abs(M32.astype(np.float64) - M)[nz] / np.abs(M[nz])).max() / I.U
    print(f"f={f} n={n}: border weights within {rel:.3g} x 2^-24 relative; the bound allows {4 * f + 9}")
    assert rel <= 4 * f + 9          # what aa_roundings() charges a border weight
    if n_out >= 5:
        assert inner.sum() == n_out - 4 and np.allclose(M[inner].sum(1), 1.0, rtol=0, atol=0)


@pytest.mark.parametrize("aa", [1, 0])
@pytest.mark.parametrize("row", I.DOWN_CASES, ids=_id)
def test_down_builders_and_another_order(row, aa):
    """exact class: an fp32 evaluation with the taps in descending order gives the reference's bits, both directions.  Bounded class:
    the same evaluation stays inside the bound, interior and border -- the bound is wide enough for an honest kernel."""
    planes, H, W, f = row
    d = I.down_case(planes, H, W, f, aa)
    if d["exact"]:
        assert np.array_equal(I.sep32(d["My"], d["x"], d["Mx"], reverse=True).astype(np.float64), d["y"])
        assert np.array_equal(I.sep32(d["My"], d["dy"], d["Mx"], reverse=True, adjoint=True).astype(np.float64), d["dx"])
        return
    My32, Mx32 = I.aa_weights32(H, f).astype(np.float64), I.aa_weights32(W, f).astype(np.float64)
    for adjoint, x, ref, ab in ((False, d["x"], d["y"], d["y_abs"]), (True, d["dy"], d["dx"], d["dx_abs"])):
        got = I.sep32(My32, x, Mx32, reverse=True, adjoint=adjoint).astype(np.float64)
        iy, ix = I.interior_mask(d["My"], adjoint), I.interior_mask(d["Mx"], adjoint)
        inner = iy[:, None] & ix[None, :]
        err = np.abs(got - ref)
        assert (err <= I.aa_roundings(f, True) * I.U * ab).all()
        assert (err[:, inner] <= I.aa_roundings(f, False) * I.U * ab[:, inner]).all()


@pytest.mark.parametrize("row", I.UP_CASES, ids=_id)
def test_up_builders_and_another_order(row):
    d = I.up_case(*row)
    got = (I.sep32(d["My"], d["x"], d["Mx"], reverse=True) + d["out0"]).astype(np.float64)
    if d["exact"]:
        assert np.array_equal(got, d["out"])
    else:
        assert (np.abs(got - d["out"]) <= I.UP8_ROUNDINGS * I.U * d["out_abs"]).all()


# ------------------------------------------------------------------------------------------- bicubic mutants

def _bicubic_mutants(kind, n_y, n_x, f, aa, x, ref, exact, tol, extra=0.0):
    applied = []
    for name in I.BICUBIC_MUTANTS:
        if not I.bicubic_mutant_applies(name, kind, n_y, n_x, f, aa):
            continue
        My, Mx = I.bicubic_mutant_matrices(name, kind, n_y, n_x, f, aa)
        got = (I.sep_adj if kind == "down_adj" else I.sep)(My, x, Mx) + extra
        dev = np.abs(got - ref)
        if exact:
            assert (dev > 0).any(), f"{kind} {n_y}x{n_x} f={f} aa={aa}: the mutant '{name}' survives these inputs"
        else:
            assert (dev > 10 * tol).any(), f"{kind} {n_y}x{n_x} f={f} aa={aa}: the mutant '{name}' stays within 10 x the tolerance"
        applied.append(name)
    return applied


@pytest.mark.parametrize("aa", [1, 0])
@pytest.mark.parametrize("row", I.DOWN_CASES, ids=_id)
def test_no_down_mutant_survives(row, aa):
    planes, H, W, f = row
    d = I.down_case(planes, H, W, f, aa)
    n = I.aa_roundings(f, True, accumulate=True) * I.U
    fwd = _bicubic_mutants("down", H, W, f, aa, d["x"], d["y"], d["exact"], None if d["exact"] else n * d["y_abs"])
    adj = _bicubic_mutants("down_adj", H, W, f, aa, d["dy"], d["dx"], d["exact"],
                           None if d["exact"] else n * (d["dx_abs"] + np.abs(d["dx0"])))
    if min(H // f, W // f) >= 3:
        assert set(fwd) == {"wrong_A", "shift"} | ({"no_norm"} if aa else set()) | ({"drop_clamped"} if not aa and f == 2 else set())
        assert set(adj) == set(fwd) | {"adjoint_M"}
    else:
        assert fwd and adj


@pytest.mark.parametrize("row", I.UP_CASES, ids=_id)
def test_no_up_mutant_survives(row):
    planes, H, W, s = row
    d = I.up_case(*row)
    applied = _bicubic_mutants("up", H, W, s, 0, d["x"], d["out"], d["exact"], None if d["exact"] else I.UP8_ROUNDINGS * I.U * d["out_abs"],
                               extra=d["out0"].astype(np.float64))
    assert set(applied) == ({"drop_clamped"} if H * W == 1 else {"wrong_A", "shift", "drop_clamped"})          # one pixel: the folded weights of every rule sum to 1
