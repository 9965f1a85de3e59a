"""The convolution dispatch of csbsr_amd/engine.py, characterised without a GPU: which library entry points ``Conv`` calls, in which
order, with which descriptor fields and packed operands, for every row of tests/conv_exact_cases.py under three eligibility tables, the
tie-breaks between the kernel families, the split / folded / class-bias / head forms, the fused epilogue-backward variants, the weight
gradients and every engine flag -- replayed against tests/golden/conv_dispatch_trace.json, which tests/golden/make_dispatch_golden.py
recorded (the library is a stub there: see its docstring for the patch points and the format).  The environment hooks of
``_lib.load`` / ``Engine.__init__`` are pinned the same way."""
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_dispatch_golden as G  # noqa: E402

with open(G.PATH) as _f:
    GOLDEN = G.loads(_f.read())
CASES = G.all_cases()


def _plain(x):
    return json.loads(json.dumps(x))


def test_the_case_list_is_the_recorded_one():
    assert [n for n, _ in CASES] == list(GOLDEN["cases"]), "regenerate with tests/golden/make_dispatch_golden.py ON THE PARENT of a dispatch change"


@pytest.mark.parametrize("name,thunk", CASES, ids=[n for n, _ in CASES])
def test_dispatch_trace(name, thunk, monkeypatch):
    G.install(monkeypatch)
    got = _plain(thunk().result())
    want = GOLDEN["cases"][name]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{name}: call {i} differs"
    assert len(got["calls"]) == len(want["calls"]), (name, [c[0] for c in got["calls"]], [c[0] for c in want["calls"]])
    assert got == want


def test_timing_off_makes_the_same_calls(monkeypatch):
    """``eng.timing = None`` (the product setting) changes nothing but the timing list"""
    G.install(monkeypatch)
    init = G.Ctx.__init__

    def quiet(self, *a, **kw):
        init(self, *a, **kw)
        self.eng.timing = None
    monkeypatch.setattr(G.Ctx, "__init__", quiet)
    monkeypatch.setattr(G.Ctx, "result", lambda self: self.rec.calls)
    for name, thunk in CASES:
        if name.startswith(("flags/default", "head1/use1", "strided/all", "thin_tp/fused")):
            assert _plain(thunk().result()) == GOLDEN["cases"][name]["calls"], name


def test_flags_and_eligibility_are_read_at_every_launch(monkeypatch):
    """one layer, launched again and again while the engine flags, ``Conv.winograd`` and the library's answers change under it: nothing
    about a family's choice may be remembered from an earlier launch"""
    G.install(monkeypatch)
    c = G.Ctx(G.ALL1)
    conv = c.conv(128, 128, 3, 1, 1)

    def launched():
        del c.rec.calls[:]
        conv.fwd(c.fm(128))
        return [e[0] for e in c.rec.calls if e[0].endswith("_forward")]
    assert launched() == ["csbsr_conv_hr_forward"]
    c.stub.elig["x3n"] = 2
    assert launched() == ["csbsr_conv_x3n_forward"]
    c.stub.elig["x3n"] = 1
    c.eng.use_hr = False
    assert launched() == ["csbsr_conv_x3n_forward"]
    c.eng.use_x3n = False
    assert launched() == ["csbsr_conv_x3_forward"]
    c.eng.use_x3w = 1
    assert launched() == ["csbsr_conv_x3_forward"]
    conv.winograd = True
    assert launched() == ["csbsr_conv_x3w_forward"]
    c.stub.elig["x3w"] = 0
    assert launched() == ["csbsr_conv_x3_forward"]
    c.eng.use_x3 = False
    assert launched() == ["csbsr_conv_forward"]
    c.eng.use_hr = True
    assert launched() == ["csbsr_conv_hr_forward"]


def test_environment_hooks(monkeypatch):
    assert G.env_vars_in_sources() == set(G.ENV_VARS), "a CSBSR_* hook of _lib.py / engine.py is missing from make_dispatch_golden.ENV_VARS (or gone)"
    got = _plain(G.env_cases(monkeypatch))
    assert list(got) == list(GOLDEN["env"])
    for key, want in GOLDEN["env"].items():
        assert got[key] == want, key


def test_every_kernel_entry_point_of_the_engine_is_in_the_trace():
    """a stub can hide a branch by never reaching it: every launch / pack symbol engine.py names occurs in the recorded trace"""
    with open(os.path.join(G.ROOT, "csbsr_amd", "engine.py")) as f:
        src = f.read()
    named = set(re.findall(r"\"(csbsr_(?:\w+_forward|pack_weights\w*|head1_\w+|conv_wgrad|unpack_wgrad|thin_tp_backward))\"", src))
    assert {"csbsr_conv_forward", "csbsr_conv_hr_forward", "csbsr_conv_x3_forward", "csbsr_conv_x3n_forward", "csbsr_conv_x3w_forward",
            "csbsr_conv_tp_forward", "csbsr_pack_weights_x3_strided", "csbsr_head1_fwd", "csbsr_head1_bwd_input"} <= named
    seen = {c[0] for case in GOLDEN["cases"].values() for c in case["calls"]}
    assert not named - seen, sorted(named - seen)
    fused = {n for n, case in GOLDEN["cases"].items() if any(c[:2] == ["last_fused", True] for c in case["calls"])}
    assert {"dact/tp", "dact/tp_dres", "dact/thin_dres"} <= fused and "dact/neither" not in fused and "dact/thin" not in fused
