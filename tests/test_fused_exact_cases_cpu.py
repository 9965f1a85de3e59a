"""The cases of tests/test_fused_exact_gpu.py without a GPU: every row's operands and reference are built here, so every bound the
builders assert (lattice, output format, sum |terms| / unit < 2^24 of every fp32 sum) is checked on the CPU, and the share of 2^24 each
sum uses is printed.  The inputs must also be able to tell a subtly wrong kernel from a right one: the discriminating elements are
asserted to be present (exact zeros in the gating activation under a nonzero gradient, ``pre == 0``, pixels of every border class), and
small mutants of the reference -- ``>=`` for ``>``, one border class dropped, the d(res) sign flipped, one tile's partial omitted -- are
shown to differ from it on those very inputs (the method of tests/test_split_planes_cpu.py)."""
import pytest
import torch

import fused_exact_cases as FC
from fused_exact_cases import BUILDERS, FUSED_ROWS


def _rows(*groups):
    rows = [r for r in FUSED_ROWS if r.group in groups]
    return pytest.mark.parametrize("row", rows, ids=[r.name for r in rows])


def test_rows_are_well_formed():
    names = [r.name for r in FUSED_ROWS]
    assert len(names) == len(set(names)), "duplicate row names"
    for r in FUSED_ROWS:
        assert r.group in BUILDERS and r.entry and r.why, r.name
        if r.budget:
            assert r.group in ("tp_dact", "folded_fwd", "pair"), f"{r.name}: only the persistent grids run under CU budgets"
    assert set(BUILDERS) == {r.group for r in FUSED_ROWS}, "a builder without a row"


@pytest.mark.parametrize("row", FUSED_ROWS, ids=[r.name for r in FUSED_ROWS])
def test_every_case_builds_within_its_bounds(row):
    c = FC.build(row)
    for what, s in c.share.items():
        assert 0.0 <= s < 1.0, (row.name, what, s)
    print(f"{row.name}: " + (", ".join(f"{k} {v:.4f} x 2^24" for k, v in c.share.items()) or "K-term sums only (assert_sum_bound)"))


def test_a_draw_that_breaks_the_sum_bound_fails():
    """the issue's measurement: with negatives at 1/16 a 16 x 64 dPre puts the slope sum at 1.4 x 2^24 -- the builder must refuse it"""
    row = next(r for r in FUSED_ROWS if r.name == "tp_dact")
    with pytest.raises(AssertionError, match="slope sum"):
        FC.build_tp_dact(row, H=16, W=64, neg=1.0 / 16)


@_rows("tp_dact")
def test_tp_dact_inputs_tell_the_mutants_apart(row):
    c = FC.build(row)
    zeros = (c.y == 0) & (c.tot != 0)
    assert int(zeros.sum()) >= 16 and int((c.y < 0).sum()) >= 1000, "the draw has no zeros / negatives under a nonzero gradient"
    assert c.H % FC.TP_TILE[0] == 0 and c.W % FC.TP_TILE[1] == 0 and (c.H // FC.TP_TILE[0]) * (c.W // FC.TP_TILE[1]) >= 2, "more than one whole tile"
    dz, db, da, dres = FC.tp_dact_ref(c)
    assert torch.equal(dz, c.dz) and torch.equal(db, c.db) and torch.equal(da, c.da)
    # >= for >: the zeros pass the gradient through unmasked
    dz_m, db_m, _, _ = FC.tp_dact_ref(c, strict=False)
    assert not torch.equal(dz_m, dz) and not torch.equal(db_m, db)
    # one tile's partial row left out of the fold
    for tile in ((0, 0, 0), (c.N - 1, 0, c.W // FC.TP_TILE[1] - 1)):
        _, db_m, da_m, _ = FC.tp_dact_ref(c, skip_tile=tile)
        assert not torch.equal(db_m, db) and not torch.equal(da_m, da), tile
    if c.res_mode is not None:
        assert bool(c.dres.any())
        assert torch.equal(dres, -c.tot if c.res_mode == "sub" else c.tot)
        assert not torch.equal(FC.tp_dact_ref(c, dres_sign=1.0 if c.res_mode == "sub" else -1.0)[3], dres)
        # the activation is rebuilt from saved -+ res: with the sign of the residual wrong the gate is another one
        y_wrong = c.saved - c.res if c.res_mode == "sub" else c.saved + c.res
        assert not torch.equal(y_wrong > 0, c.y > 0)


@_rows("thin_dact")
def test_thin_dact_inputs_tell_the_mutants_apart(row):
    c = FC.build(row)
    assert int(((c.y == 0) & (c.tot != 0)).sum()) >= 16 and int((c.y < 0).sum()) >= 1000
    dz, da, dres = FC.thin_dact_ref(c)
    assert not torch.equal(FC.thin_dact_ref(c, strict=False)[0], dz)
    assert not torch.equal(FC.thin_dact_ref(c, dres_sign=-1.0 if c.res_mode == "add" else 1.0)[2], dres)
    assert torch.equal(dres, c.tot if c.res_mode == "add" else -c.tot)


@_rows("kbup")
def test_kbup_inputs_tell_the_mutants_apart(row):
    c = FC.build(row)
    z = (c.pre == 0) & (c.dout != 0)
    assert int(z.sum()) >= 16, "pre == 0 under a nonzero gradient does not occur: the sign convention at zero is not pinned"
    assert int((c.pre < 0).sum()) >= 16 and int((c.pre > 0).sum()) >= 16
    dpre_m, da_m = FC.kbup_ref(c, strict=False)
    assert not torch.equal(dpre_m, c.dpre) and torch.equal(da_m, c.da)      # (at pre == 0 the slope term is zero either way)


FOLD_CLASSES = {(12, 20): {0, 1, 2, 4, 5, 6, 8, 9, 10}, (1, 7): {12, 13, 14}, (2, 5): {4, 5, 6, 8, 9, 10}, (3, 3): {0, 1, 2, 4, 5, 6, 8, 9, 10},
                (32, 32): {0, 1, 2, 4, 5, 6, 8, 9, 10}, (40, 33): {0, 1, 2, 4, 5, 6, 8, 9, 10}}


@_rows("folded_bwd")
def test_folded_bwd_inputs_tell_the_mutants_apart(row):
    c = FC.build(row)
    assert set(c.classes) == FOLD_CLASSES[(c.H, c.W)]
    assert int((c.out < 0).sum()) >= 16 and int((c.out == 0).sum()) >= 1
    for k in c.classes:          # every border class that occurs carries a gradient the result depends on
        dk, dwc, _ = FC.folded_bwd_ref(c, drop=k)
        assert not torch.equal(dk, c.dk) and not torch.equal(dwc, c.dw[:, c.cf:]), f"dropping class {k} goes unnoticed"
    assert FC.folded_bwd_ref(c, drop=15 if 15 not in c.classes else 3)[0].equal(c.dk)          # (a class the map does not have)


@_rows("fillsums")
def test_fillsums_inputs_tell_the_mutants_apart(row):
    c = FC.build(row)
    assert set(c.classes) == FOLD_CLASSES[(c.H, c.W)]
    assert int(((c.x == 0) & (c.din != 0)).sum()) >= 4 and int((c.x < 0).sum()) >= 16
    for k in c.classes:
        sums, dw, _ = FC.fillsums_ref(c, drop=k)
        assert not torch.equal(sums, c.sums) and not torch.equal(dw, c.dw), f"dropping class {k} goes unnoticed"
    assert not torch.equal(FC.fillsums_ref(c, strict=False)[2], c.din)


@_rows("pair")
def test_pair_inputs_tell_the_mutants_apart(row):
    c = FC.build(row)
    assert int(((c.x == 0) & (c.din != 0)).sum()) >= 4 and int((c.x < 0).sum()) >= 16
    assert not torch.equal(FC.pair_ref(c, strict=False), c.din)
    if c.cin_tot > c.cin:
        assert bool(c.w[:, c.cin:].any()) and not bool(c.dw[:, c.cin:].any())


@_rows("shuffle")
def test_the_identity_behind_shuffle_conv(row):
    """conv3x3 + PixelShuffle(s) is a transposed conv (3s x 3s, stride s, pad s) with the weight permutation of ShuffleConv._remap
    (written out here from the class's docstring: no engine needed), and the un-permutation inverts it"""
    import torch.nn.functional as F
    c = FC.build(row)
    s, C, cin = c.s, c.C, c.cin
    Wt = c.Wm.reshape(C, s, s, cin, 3, 3).flip(4, 5).permute(3, 0, 4, 1, 5, 2).reshape(cin, C, 3 * s, 3 * s)
    assert torch.equal(F.conv_transpose2d(c.x, Wt, None, s, s), F.pixel_shuffle(F.conv2d(c.x, c.Wm, None, 1, 1), s))
    back = Wt.reshape(cin, C, 3, s, 3, s).permute(1, 3, 5, 0, 2, 4).flip(4, 5).reshape(C * s * s, cin, 3, 3)
    assert torch.equal(back, c.Wm)
