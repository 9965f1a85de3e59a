"""Every convolution kernel has an exact-parity row (no GPU needed): the forward kernel IDs (``enum CONVK_*``, csrc/conv_common.h) and
the weight-gradient kernel IDs (``enum WGRADK_*``, csrc/conv_wgrad.h) are parsed from the sources and each must be the ``kid`` of a row
of tests/conv_exact_cases.py -- or be listed in its EXCLUDED with a reason.  A new kernel therefore arrives with an exact test.  The same
holds for the template instances the dispatchers build (REQUIRED_VARIANTS), the engine's entry points into the kernels (Conv's fwd* /
bwd* methods and subclasses, read from csbsr_amd/engine.py; the public functions of csbsr_amd/modeling/kp_bwd.py other than its ``*_ok``
predicates) and the sigmoid / split / high-precision-dgrad operand modes: each has a row -- here, in tests/fused_exact_cases.py or in
tests/split_conv_cases.py (the split-fp16 paths), whose rows name their entry point -- or a NOT_COVERED reason, so what the tables leave out is written down next to them.  The debug-mode defaults the GPU test restores are checked against
the sources' initial values."""
import os
import re

import pytest

from conv_exact_cases import DEFAULT_MODES, EXCLUDED, NOT_COVERED, REQUIRED_MODES, REQUIRED_VARIANTS, ROW_ENTRY, ROWS
from fused_exact_cases import FUSED_ROWS
from split_conv_cases import SPLIT_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csbsr_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def parse_enum(text, prefix):
    """{name: value} of the C enum whose enumerators start with ``prefix`` (implicit values count up from the last explicit one)"""
    m = re.search(r"enum\s*\{([^}]*\b" + prefix + r"\w*[^}]*)\}", text)
    assert m, f"no enum of {prefix}* found"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    out, nxt = {}, 0
    for item in (s.strip() for s in body.split(",")):
        if not item:
            continue
        name, _, val = (p.strip() for p in item.partition("="))
        assert name.startswith(prefix), name
        nxt = int(val, 0) if val else nxt
        out[name] = nxt
        nxt += 1
    return out


def kernel_ids():
    return {"fwd": parse_enum(_read("conv_common.h"), "CONVK_"), "wgrad": parse_enum(_read("conv_wgrad.h"), "WGRADK_")}


def missing_ids(rows, excluded, ids=None):
    """names of the kernel IDs without a row and without an exclusion"""
    ids = kernel_ids() if ids is None else ids
    have = {("wgrad" if r.op == "wgrad" else "fwd", r.kid) for r in rows}
    miss = []
    for kind, table in ids.items():
        for name, v in table.items():
            if (kind, v) not in have and name not in excluded:
                miss.append(f"{name} = {v}")
    return miss


def test_enums_parse():
    ids = kernel_ids()
    assert ids["fwd"]["CONVK_IGEMM32"] == 0 and ids["fwd"]["CONVK_X3N"] == 20
    assert ids["wgrad"]["WGRADK_REG128"] == 0 and ids["wgrad"]["WGRADK_HR"] == 8 and ids["wgrad"]["WGRADK_GLDS512"] == 9


def test_every_kernel_id_has_an_exact_row():
    miss = missing_ids(ROWS, EXCLUDED)
    assert not miss, "kernel IDs without a row in tests/conv_exact_cases.py (add one, or an EXCLUDED entry with the reason): " + ", ".join(miss)


def entry_points():
    """Conv's public fwd* / bwd* methods and the subclasses of Conv, read from csbsr_amd/engine.py"""
    with open(os.path.join(ROOT, "csbsr_amd", "engine.py")) as f:
        src = f.read()
    body = re.search(r"^class Conv\b.*?(?=^class |\Z)", src, re.S | re.M).group(0)
    meths = ["Conv." + m for m in re.findall(r"^    def ((?:fwd|bwd)\w*)\(", body, re.M)]
    subs = re.findall(r"^class (\w+)\(Conv\)", src, re.M)
    with open(os.path.join(ROOT, "csbsr_amd", "modeling", "kp_bwd.py")) as f:
        kp = ["kp_bwd." + m for m in re.findall(r"^def ([a-z]\w*)\(", f.read(), re.M) if not m.endswith("_ok")]
    return meths + subs + kp


def _instances(rows, fused, split=SPLIT_ROWS):
    """(kernel ID, template instance) pairs the rows of the three tables assert"""
    return ({(r.kid, r.var) for r in rows if r.op != "wgrad"} | {(r.kid, r.var) for r in fused if isinstance(r.kid, int)}
            | {(r.kid, r.var) for r in split})


def missing_paths(rows, not_covered, fused=FUSED_ROWS, split=SPLIT_ROWS):
    """the template instances (REQUIRED_VARIANTS), entry points and operand modes with neither a row nor a NOT_COVERED reason"""
    have = _instances(rows, fused, split)
    miss = []
    for fam, (kid, vars_) in REQUIRED_VARIANTS.items():
        for v in vars_:
            if (kid, v) not in have and f"{fam}/{v}" not in not_covered:
                miss.append(f"{fam}/{v}")
    # (a split row covers its instance and its mode, not its entry point: the plain-operand row of that entry point stays required)
    ops = {ROW_ENTRY[r.op] for r in rows} | {r.entry for r in fused}
    for ep in entry_points():
        if ep not in ops and ep not in not_covered:
            miss.append(ep)
    epis = {m for r in rows for m in r.epi.split("_")} | {r.mode for r in split}
    for m in REQUIRED_MODES:
        if m not in epis and m not in not_covered:
            miss.append(m)
    return miss


def test_every_instance_and_entry_point_has_a_row_or_a_reason():
    miss = missing_paths(ROWS, NOT_COVERED)
    assert not miss, "paths without a row in tests/conv_exact_cases.py and without a NOT_COVERED reason: " + ", ".join(miss)


def test_not_covered_is_current():
    """every NOT_COVERED entry names a real path that really has no row (a row added later must take its entry out)"""
    eps = set(entry_points())
    have = _instances(ROWS, FUSED_ROWS)
    for name, why in NOT_COVERED.items():
        assert isinstance(why, str) and len(why.split()) >= 6, f"NOT_COVERED[{name}] needs a written reason"
        if "/" in name:
            fam, v = name.split("/")
            kid, vars_ = REQUIRED_VARIANTS[fam]
            assert int(v) in vars_ and (kid, int(v)) not in have, f"NOT_COVERED[{name}]: not a required instance, or it has a row"
        elif name in REQUIRED_MODES:
            assert name not in {m for r in ROWS for m in r.epi.split("_")} | {r.mode for r in SPLIT_ROWS}, f"NOT_COVERED[{name}] has a row"
        else:
            assert name in eps and name not in {ROW_ENTRY[r.op] for r in ROWS} | {r.entry for r in FUSED_ROWS}, \
                f"NOT_COVERED[{name}]: no such entry point, or it has a row"


SPLIT_INSTANCES = [f"{fam}/{v}" for fam in ("GLDS64", "GLDS128", "GLDS256", "GLDS256W") for v in (1, 3)]


def test_nothing_is_left_uncovered():
    """the split-precision entries were the last ones: every fused-split instance, the split mode and the high-precision dgrad have rows in
    tests/split_conv_cases.py, and it is those rows that cover them"""
    assert NOT_COVERED == {}
    assert missing_paths(ROWS, NOT_COVERED, split=[]) == SPLIT_INSTANCES + ["split", "Conv.hp_dgrad"]
    entries = {r.entry for r in SPLIT_ROWS}
    assert {"Conv.fwd", "Conv.fwd_folded", "Conv.fwd_const_1x1", "Conv.bwd_input"} <= entries
    fwd = [r for r in SPLIT_ROWS if r.mode == "split"]
    assert {r.blocks for r in fwd} == {1, 2, 3} and {r.plan for r in fwd} == {1, 2, 3, 4, 5} and {r.fused for r in fwd} == {0, 1}
    assert any(len(r.out_c0) > 1 and r.mode == "split" for r in SPLIT_ROWS), "no split output slice row"
    assert any(r.epi == "bn" for r in fwd) and any(r.epi.endswith("_fma") for r in fwd)


def test_fused_rows_name_real_entry_points():
    eps = set(entry_points())
    for r in FUSED_ROWS:
        assert r.entry in eps, f"{r.name}: {r.entry} is no entry point of csbsr_amd/engine.py or csbsr_amd/modeling/kp_bwd.py"


def test_the_path_check_names_what_is_missing():
    """dropping a row, a reason, or a new Conv method shows up by name"""
    assert missing_paths([r for r in ROWS if r.name != "x3n_narrow_bn"], NOT_COVERED, split=[r for r in SPLIT_ROWS if r.name != "fs2_x3n_bn"]) == ["X3N/3"]
    assert missing_paths(ROWS, NOT_COVERED, split=[r for r in SPLIT_ROWS if r.mode != "split"]) == SPLIT_INSTANCES + ["split"]
    assert missing_paths(ROWS, NOT_COVERED, split=[r for r in SPLIT_ROWS if r.mode != "Conv.hp_dgrad"]) == ["Conv.hp_dgrad"]
    assert missing_paths(ROWS, NOT_COVERED, split=[r for r in SPLIT_ROWS if r.name != "fs_glds256w_gk"]) == ["GLDS256W/3"]
    assert missing_paths(ROWS, {"split": "a reason"}, split=[r for r in SPLIT_ROWS if r.mode != "split"]) == SPLIT_INSTANCES
    assert "Conv.fwd_classbias" in entry_points() and "Conv.bwd_weights_folded" in entry_points()
    # ... and so does dropping the rows of the second table, or one of them, or a new public function of kp_bwd.py
    assert missing_paths(ROWS, NOT_COVERED, fused=[]) == ["TP/14", "TP/13", "Conv.fwd_folded", "Conv.fwd_const_1x1", "Conv.bwd_weights_folded",
                                                         "Conv.bwd_thin_tp_fused", "ShuffleConv", "kp_bwd.fold_const_wgrad", "kp_bwd.pair1x1_backward"]
    assert missing_paths(ROWS, NOT_COVERED, fused=[r for r in FUSED_ROWS if r.group != "shuffle"]) == ["ShuffleConv"]
    assert missing_paths(ROWS, NOT_COVERED, fused=[r for r in FUSED_ROWS if r.name != "tp_dact"]) == ["TP/14"]
    assert "kp_bwd.pair1x1_ok" not in entry_points() and "kp_bwd.const_wgrad_ok" not in entry_points()


def test_exclusions_carry_a_reason():
    ids = kernel_ids()
    names = set(ids["fwd"]) | set(ids["wgrad"])
    for name, why in EXCLUDED.items():
        assert name in names, f"EXCLUDED names {name}, which is no kernel ID"
        assert isinstance(why, str) and len(why.split()) >= 4, f"EXCLUDED[{name}] needs a written reason"


def test_the_check_names_a_missing_id():
    """removing the rows of one ID, or a new enumerator, makes the coverage check fail with that ID's name"""
    ids = kernel_ids()
    rows = [r for r in ROWS if not (r.op != "wgrad" and r.kid == ids["fwd"]["CONVK_HR"])]
    assert missing_ids(rows, EXCLUDED, ids) == ["CONVK_HR = 8"]
    text = _read("conv_common.h").replace("CONVK_X3N };", "CONVK_X3N, CONVK_NEXT };")
    grown = {"fwd": parse_enum(text, "CONVK_"), "wgrad": ids["wgrad"]}
    assert missing_ids(ROWS, EXCLUDED, grown) == ["CONVK_NEXT = 21"]
    text = _read("conv_wgrad.h").replace("WGRADK_GLDS512 };", "WGRADK_GLDS512, WGRADK_NEXT };")
    grown = {"fwd": ids["fwd"], "wgrad": parse_enum(text, "WGRADK_")}
    assert missing_ids(ROWS, EXCLUDED, grown) == ["WGRADK_NEXT = 10"]


def test_rows_are_well_formed():
    names = [r.name for r in ROWS]
    assert len(names) == len(set(names)), "duplicate row names"
    for r in ROWS:
        assert r.op in ROW_ENTRY, r.name
        assert r.kid >= 0, f"{r.name}: no kernel ID"
        assert r.why, f"{r.name}: say why the row reaches its kernel"
        for name, _ in r.modes:
            assert name.startswith(("eng.", "arg.")) or name in DEFAULT_MODES, f"{r.name}: mode {name} has no default to restore"


@pytest.mark.parametrize("name,src,var", [
    ("conv_x3", "conv_x3.hip", "g_conv_x3_mode"), ("conv_x3n", "conv_x3n.hip", "g_conv_x3n_mode"),
    ("conv_x3w", "conv_x3w.hip", "g_conv_x3w_mode"), ("conv_tp", "conv_tp.hip", "g_conv_tp_mode"),
    ("wgrad_hr", "conv_wgrad_hr.hip", "g_wgrad_hr"), ("conv_glds", "conv_igemm_glds.hip", "g_glds_mode"),
    ("wgrad_tr", "conv_wgrad.hip", "g_wgrad_use_tr"),
])
def test_restored_modes_are_the_library_defaults(name, src, var):
    """the value the GPU test restores is the mode variable's initial value (conv_glds / wgrad_tr: the other bits of those setters only
    switch off what is on by default, so the default call is the plain initial mode)"""
    m = re.search(r"static int " + var + r"\s*=\s*(\d+)\s*;", _read(src))
    assert m, f"{var} not found in {src}"
    assert DEFAULT_MODES[name] == int(m.group(1)), (name, DEFAULT_MODES[name], int(m.group(1)))
