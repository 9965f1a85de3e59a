"""The case tables of tests/elementwise_cases.py, checked without a GPU: every builder proves its lattice bounds on the reference
(assert_sum_bound / assert_on_lattice / assert_fp16_exact / assert_fp32_exact run inside the builders, so building a row IS the proof),
every mutant differs from the reference on every row it applies to (by more than one bound where the row carries a bound), a plain fp32
evaluation sits at least four times inside every counted bound, every dispatch branch has a row, and every entry point and kernel of
csrc/elementwise.hip is accounted for."""
import numpy as np
import pytest

import elementwise_cases as E


def _id(r):
    return "x".join(str(v) for v in r)


def _differs(a, b):
    return a.shape == b.shape and bool((np.asarray(a) != np.asarray(b)).any())


def test_constants_parse_and_tables_cross_the_seams():
    k = E.constants()
    assert k["SEG"] == 8 and k["BIG"] == 1024 and k["CHUNK"] == 512 and k["WP"] == 1024
    assert [E.border_path(H, W) for H, W in E.SMALL_SHAPES] == ["small"] * len(E.SMALL_SHAPES)
    assert [E.border_path(H, W) for H, W in E.LARGE_SHAPES] == ["large"] * len(E.LARGE_SHAPES)
    assert (31 * 33 == k["BIG"] - 1) and (3 * 341 == k["BIG"] - 1) and (32 * 32 == k["BIG"]) and (3 * 342 > k["BIG"])
    assert E.border_chunks(23 * 45) == 3 and (23 * 45) % 3 == 0 and E.border_chunks(70 * 66) == 10
    assert 4 - 2 < k["SEG"] and 3 - 2 == 1                                  # column edges shorter than the segment count
    # the weighted pool's hw values sit on both sides of its chunk size; the epilogue's shapes take one block and several
    assert {hw for _, hw, _ in E.WPOOL_SHAPES} >= {k["WP"] - 1, k["WP"], k["WP"] + 1}
    assert sorted(E.epi_blocks(*s)[1] for s in E.EPI_SHAPES) == [1, 1, 3, 6]
    assert E.epi_blocks(300, 264)[0] == 7 and E.epi_blocks(100, 24)[0] == 85


# ------------------------------------------------------------------------------------------- class sums and fills

@pytest.mark.parametrize("row", E.BORDER_SHAPES, ids=_id)
def test_border_rows(row):
    N, H, W, c = row
    kinds = ["sums", "mask_sums"] + (["negdot"] if E.border_path(H, W) == "large" else [])
    for kind in kinds:
        for preset in (False, True):
            ref = E.class_reference(kind, N, H, W, c, preset)
            for m in E.CLASS_MUTANTS:
                if E.class_mutant_applies(m, kind, N, H, W, c, preset):
                    assert _differs(E.class_mutant(m, kind, N, H, W, c, preset), ref), f"{m} does not change {kind} {row} preset={preset}"
    fill, masked = E.class_reference("fill", N, H, W, c), E.class_reference("fill_masked", N, H, W, c)
    assert fill.shape == (N, H, W, c) and _differs(fill, masked)
    d = E.class_case(N, H, W, c, ring=False)
    assert len({tuple(v) for v in d["V"][0, :, :2]}) == 16                  # a pixel filled from the wrong class shows


@pytest.mark.parametrize("row", E.RING_SHAPES, ids=_id)
def test_ring_rows(row):
    for preset in (False, True):
        ref = E.class_reference("ring", *row, preset)
        assert _differs(E.class_mutant("ring_typ_off_by_one", "ring", *row, preset), ref)
    assert sorted(set(E.ring_cls(row[1], row[2]).ravel())) == list(range(25))


def test_class_mutants_all_apply_somewhere():
    used = set()
    for kind, shapes in (("sums", E.BORDER_SHAPES), ("negdot", [s for s in E.BORDER_SHAPES if E.border_path(s[1], s[2]) == "large"]), ("ring", E.RING_SHAPES)):
        for s in shapes:
            used |= {m for m in E.CLASS_MUTANTS if E.class_mutant_applies(m, kind, *s, True)}
    assert used == set(E.CLASS_MUTANTS)


# ------------------------------------------------------------------------------------------- weighted pool

@pytest.mark.parametrize("row", E.WPOOL_SHAPES, ids=_id)
def test_wpool_rows(row):
    d = E.wpool_case(*row)
    for m in E.WPOOL_MUTANTS:
        if E.wpool_mutant_applies(m, *row):
            assert _differs(E.wpool_mutant(m, *row), d["out"])
    assert any(E.wpool_mutant_applies("seam_twice", *r) for r in E.WPOOL_SHAPES)


# ------------------------------------------------------------------------------------------- adaptive pool

def _aap_fwd32(x, OH, OW):
    N, H, W, c = x.shape
    y = np.zeros((N, OH, OW, c), np.float32)
    for oy, (y0, y1) in enumerate(E.aap_windows(H, OH)):
        for ox, (x0, x1) in enumerate(E.aap_windows(W, OW)):
            a = np.zeros((N, c), np.float32)
            for iy in range(y0, y1):
                for ix in range(x0, x1):
                    a = a + x[:, iy, ix].astype(np.float32)
            y[:, oy, ox] = a * (np.float32(1) / np.float32((y1 - y0) * (x1 - x0)))
    return y


def _aap_bwd32(dy, H, W, dx0):
    N, OH, OW, c = dy.shape
    dx = np.zeros((N, H, W, c), np.float32)
    for oy, (y0, y1) in enumerate(E.aap_windows(H, OH)):
        for ox, (x0, x1) in enumerate(E.aap_windows(W, OW)):
            inv = np.float32(1) / np.float32((y1 - y0) * (x1 - x0))
            dx[:, y0:y1, x0:x1] += (dy[:, oy, ox].astype(np.float32) * inv)[:, None, None]
    return dx + dx0.astype(np.float32)


@pytest.mark.parametrize("row", E.AAP_EXACT + E.AAP_RAGGED, ids=_id)
def test_aap_rows(row):
    N, H, W, OH, OW, c = row
    d = E.aap_case(*row)
    assert d["exact"] or row in E.AAP_RAGGED          # (8 x 8 -> 6: overlapping windows of four pixels are exact too, and asked so)
    mf, mb = E.aap_mutant("window_end", "fwd", *row), E.aap_mutant("window_end", "bwd", *row)
    if d["exact"]:
        if E.aap_mutant_applies("window_end", *row):
            assert _differs(mf, d["y"]) and _differs(mb, d["dx"])
        return
    bf = E.aap_fwd_roundings(d["cnt"])[None, :, :, None] * E.U * d["y_abs"] + E.H16 * np.abs(d["y"])
    bb = E.AAP_BWD_ROUNDINGS * E.U * (d["dx_abs"] + np.abs(d["dx0"])) + E.H16 * np.abs(d["dx"] + d["dx0"])
    assert (np.abs(_aap_fwd32(d["x"], OH, OW) - d["y"]) * E.MARGIN <= E.aap_fwd_roundings(d["cnt"])[None, :, :, None] * E.U * d["y_abs"]).all()
    assert (np.abs(_aap_bwd32(d["dy"], H, W, d["dx0"]) - (d["dx"] + d["dx0"])) * E.MARGIN <= E.AAP_BWD_ROUNDINGS * E.U * (d["dx_abs"] + np.abs(d["dx0"]))).all()
    assert (np.abs(mf - d["y"]) > bf).any() and (np.abs(mb - d["dx"]) > bb).any(), "window_end stays inside the bound"


def test_aap_tables_reach_both_kernels():
    ks = {(E.aap_kernel_for(*s[1:5]), E.aap_case(*s)["exact"]) for s in E.AAP_EXACT + E.AAP_RAGGED}
    assert ks == {("aap_fwd_block_kernel", True), ("aap_fwd_kernel", True), ("aap_fwd_block_kernel", False), ("aap_fwd_kernel", False)}


# ------------------------------------------------------------------------------------------- bilinear

@pytest.mark.parametrize("row", E.BIL_EXACT, ids=_id)
def test_bilinear_rows(row):
    d = E.bilinear_case(*row)
    for direction, ref in (("fwd", d["y"]), ("bwd", d["dx"])):
        for drop in (0, 1):
            right = ref * d["drop"][:, None, None, :] if drop else ref
            for m in E.BIL_MUTANTS:
                if E.bilinear_mutant_applies(m, direction, drop, *row):
                    assert _differs(E.bilinear_mutant(m, direction, drop, *row), right), f"{m} does not change {direction} {row} drop={drop}"


def test_bilinear_tables_reach_every_kernel():
    reached = {k for r in E.rows() if r["entry"] in ("csbsr_bilinear_fwd", "csbsr_bilinear_bwd") for k in r["kernels"]}
    assert reached == set(E.BIL_KERNELS)
    assert {s[5] for s in E.BIL_EXACT} == {0, 1}
    for want in ("bilinear_fwd_cols_kernel", "bilinear_bwd_cols_kernel"):          # the column kernels with and without align_corners
        assert {r["shape"][5] for r in E.rows() if want in r["kernels"]} == {0, 1}


# ------------------------------------------------------------------------------------------- epilogue backward

@pytest.mark.parametrize("shape", E.EPI_SHAPES, ids=_id)
def test_epilogue_rows(shape):
    used = set()
    for cfg in E.EPI_CONFIGS:
        row = shape + cfg
        ref = E.epi_ref(*row)
        d = E.epi_case(*row)
        assert ("dprelu" in ref) == (cfg[0] == E.ACT_PRELU) and ("dpre_abs" in ref) == (cfg[0] == E.ACT_SIGMOID)
        assert ("dres" in ref) == bool(cfg[2]) and ("dres2" in ref) == bool(cfg[3])
        if cfg[0] == E.ACT_RELU and cfg[1] == E.RES_NONE:
            assert (d["pre"] <= 0).any() and (d["out"][d["pre"] <= 0] == 0).all()          # saved outputs hold exact zeros
        for m in E.EPI_MUTANTS:
            if E.epi_mutant_applies(m, *row):
                used.add(m)
                mut = E.epi_mutant(m, *row)
                assert any(_differs(mut[k], ref[k]) for k in ref if k != "dpre_abs"), f"{m} does not change {row}"
    assert "relu_one_at_zero" in used


def test_epilogue_configs_cover_the_issue():
    assert {(a, r) for a, r, _, _ in E.EPI_CONFIGS} >= {(a, r) for a in (0, 1, 2, 3) for r in (0, 1, 2, 4)}
    assert {c[2] for c in E.EPI_CONFIGS} == {0, 1, 2} and {c[3] for c in E.EPI_CONFIGS} == {0, 1, 2}
    assert any(E.epi_mutant_applies("dbias_last_partial", *(s + E.EPI_CONFIGS[0])) for s in E.EPI_SHAPES)
    assert 264 in {c for _, c in E.EPI_SHAPES}


# ------------------------------------------------------------------------------------------- small kernels

@pytest.mark.parametrize("kind,table", [("axpby", E.AXPBY), ("sum_act", E.SUM_ACT), ("to_nchw", E.TO_NCHW), ("to_nhwc", E.TO_NHWC), ("dc_bias", E.DC_BIAS)])
def test_small_rows(kind, table):
    for row in table:
        d = E.small_case(kind, *row)
        assert np.isfinite(d["ref"]).all()
    if kind == "to_nhwc":
        d = E.small_case(kind, 2, 3, 5, 7, 16, 1)
        assert (d["ref"][..., 3:] == 0).all() and (d["ref"][..., :3] != 0).any()
    if kind == "dc_bias":
        assert {r[1] % 4 for r in table} == {1, 0} and {r[4] > 0 for r in table} == {False, True}


# ------------------------------------------------------------------------------------------- batch norm

@pytest.mark.parametrize("shape", E.BN_SHAPES, ids=_id)
def test_bn_rows(shape):
    npix = shape[0] * shape[1]
    for cfg in E.BN_CONFIGS:
        row = shape + cfg
        d = E.bn_case(*row)
        bound = E.BN_DX_ROUNDINGS * E.U * d["dx_abs"]
        err = np.abs(E.bn_dx32(d, npix) - d["dx"])
        assert (err * E.MARGIN <= bound).all(), f"bn dx {row}: an fp32 evaluation is not {E.MARGIN:g} times inside the bound"
        for m in E.BN_MUTANTS:
            if E.bn_mutant_applies(m, *row):
                assert _differs(E.bn_mutant_red(m, *row), d["red"]), f"{m} does not change red of {row}"
    assert sorted({E.bn_blocks(s[0] * s[1], s[2]) for s in E.BN_SHAPES}) == [1, 2, 3]


def test_bn_finalize_rows():
    for row in E.BN_FINALIZE:
        d = E.bn_finalize_case(*row)
        assert (d["invstd"] > 0).all() and row[2] & (row[2] - 1) == 0


def test_channel_mean_rows():
    assert sorted(E.cmean_slices(*r[1:])[1] for r in E.CMEAN) == [1, 1, 1, 1, 2, 3]
    assert [E.cmean_case(*r)["exact"] for r in E.CMEAN] == [True] * 5 + [False]
    d = E.cmean_case(2, 15, 15, 8, 2)
    assert _differs(d["ref"], d["x"][:, :14:2, :14:2].sum((1, 2)) / 64)          # the last sampled row and column count


# ------------------------------------------------------------------------------------------- rows added with a counted bound

def _inside(err, bound, what):
    assert (err[bound == 0] == 0).all() and (err * E.MARGIN <= bound).all(), f"{what}: an fp32 evaluation is not {E.MARGIN:g} times inside the bound"


@pytest.mark.parametrize("row", E.INSTNORM, ids=_id)
def test_instnorm_rows(row):
    N, C, hw = row
    d = E.instnorm_case(*row)
    assert "(hw + 65535) / %d)" % E.INSTNORM_CHUNK in E.source().split("csbsr_instnorm_bwd(")[1]
    for acc in (0, 1):
        ref, bound = d["dx"] + (d["dx0"] if acc else 0.0), E.instnorm_bound(d, acc)
        _inside(np.abs(E.instnorm_dx32(d, hw, acc) - ref), bound, f"instnorm {row} accumulate={acc}")
        wrong = d["invstd"][..., None] * (d["g"] - d["red"][..., 0:1] / hw)          # a backward without the xh term
        assert (np.abs(wrong + (d["dx0"] if acc else 0.0) - ref) > bound).any()


@pytest.mark.parametrize("row", E.BIL_BOUNDED, ids=_id)
def test_bilinear_bounded_rows(row):
    N, H, W, OH, OW, al, c = row
    d = E.bilinear_bounded_case(*row)
    for direction, emu in (("fwd", d["y32"]), ("bwd", d["dx32"])):
        ref, b32 = E.bilinear_bounds(d, direction, 0, 0, H, W)
        _inside(np.abs(emu - ref), b32, f"bilinear {direction} {row}")
        for m in ("no_half_pixel", "bwd_misses_last"):
            if E.bilinear_mutant_applies(m, direction, 0, *row):
                away = np.abs(E.bilinear_bounded_mutant(m, direction, *row) - ref) > b32 + E.H16 * np.abs(ref)
                assert away.any(), f"{m} stays inside the bound of {direction} {row}"
        drop_ref, drop_b = E.bilinear_bounds(d, direction, 1, 0, H, W)
        wrong = ref * np.roll(d["drop"], 1, 0)[:, None, None, :]          # the scale row of the other sample
        assert (np.abs(wrong - drop_ref) > drop_b + E.H16 * np.abs(drop_ref)).any()
    assert any(r[3] < r[1] for r in E.BIL_BOUNDED)          # a down-scale
    assert "bilinear_fwd_cols_kernel" in {k for r in E.BIL_BOUNDED for k in E.bilinear_kernel_for("fwd", *r[:5], r[6])}


@pytest.mark.parametrize("row", E.BIL32_EXACT + E.BIL32_BOUNDED, ids=_id)
def test_bilinear32_rows(row):
    d = E.bilinear32_case(*row)
    assert d["exact"] == (row in E.BIL32_EXACT)
    if not d["exact"]:
        _inside(np.abs(d["y32"] - d["y"]), d["y_bound"], f"bilinear32 fwd {row}")
        _inside(np.abs(d["dx32"] - d["dx"]), d["dx_bound"], f"bilinear32 bwd {row}")


@pytest.mark.parametrize("row", E.MAXPOOL, ids=_id)
def test_maxpool_rows(row):
    d = E.maxpool_case(*row)
    y, dx_last = E.maxpool_ref(d["x"], d["dy"], last=True)
    assert np.array_equal(y, d["y"])
    if row[1] * row[2] > 1:
        assert _differs(dx_last, d["dx"]), "no tie decides a gradient in this row"
    assert abs(d["dx"].sum() - d["dy"].sum()) < 1e-9          # every window's gradient lands exactly once
    assert {1} <= {r[1] for r in E.MAXPOOL} and {1} <= {r[2] for r in E.MAXPOOL}


def test_epilogue_two_level_fold_row():
    row = E.EPI_FOLD2
    assert E.epi_blocks(*row[:2])[1] == E.constants()["RPC"] + 1 <= E.constants()["EPI_CAP"]          # one row more than a single level folds
    ref = E.epi_ref(*row)
    assert _differs(E.epi_mutant("dbias_last_partial", *row)["dbias"], ref["dbias"])
    assert all(E.epi_blocks(*s)[1] <= E.constants()["RPC"] for s in E.EPI_SHAPES)


def test_epilogue_sigmoid_rows():
    for shape in E.EPI_SHAPES:
        for cfg in [c for c in E.EPI_CONFIGS if c[0] == E.ACT_SIGMOID]:
            ref = E.epi_ref(*(shape + cfg))
            bound = E.EPI_SIGMOID_ROUNDINGS * E.U * ref["dpre_abs"]
            _inside(np.abs(ref["dpre"].astype(np.float32).astype(np.float64) - ref["dpre"]), bound, f"sigmoid {shape}")          # exact in fp32
            mut = E.epi_mutant("sigmoid_linear", *(shape + cfg))
            assert (np.abs(mut["dpre"] - ref["dpre"]) > bound + E.H16 * np.abs(ref["dpre"])).any()


# ------------------------------------------------------------------------------------------- coverage

def test_every_entry_point_and_kernel_is_accounted_for():
    assert E.missing_names() == []
    for name, why in E.NOT_COVERED.items():
        assert len(why.split()) >= 6, f"{name}: a reason, please"
    entries, kernels = E.source_names()
    known = set(entries + kernels)
    with open(E.os.path.join(E.CSRC, "image_ops.hip")) as f:          # the fp32 bilinear pair lives there; its rows name it
        image_ops = f.read()
    for n in ("csbsr_bilinear32_fwd", "csbsr_bilinear32_bwd", "bilinear32_fwd_kernel", "bilinear32_bwd_kernel"):
        assert n + "(" in image_ops
        known.add(n)
    for table in (E.COVERED_ELSEWHERE, E.NOT_COVERED):
        assert set(table) <= known, f"names that csrc/elementwise.hip no longer has: {sorted(set(table) - known)}"
    named = {r["entry"] for r in E.rows()} | {k for r in E.rows() for k in r["kernels"]}
    assert named <= known, f"rows name what csrc/elementwise.hip does not have: {sorted(named - known)}"
    assert not (named & set(E.NOT_COVERED)), "a name with rows is listed as not covered"


def test_coverage_check_notices():
    without = [r for r in E.rows() if "rcs_lines_kernel" not in r["kernels"]]
    assert set(E.missing_names(table=without)) == {"csbsr_ring_class_sums", "rcs_lines_kernel", "rcs_finish_kernel"}
    grown = E.source() + "\n__global__ __launch_bounds__(256) void brand_new_kernel(float* p) {}\nextern \"C\" int csbsr_brand_new(float* p) { return 0; }\n"
    assert E.missing_names(text=grown) == ["csbsr_brand_new", "brand_new_kernel"]
    assert "csbsr_plane_reduce" in E.missing_names(elsewhere={}) and "csbsr_round_weights" in E.missing_names(not_covered={})
