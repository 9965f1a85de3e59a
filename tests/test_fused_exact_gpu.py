"""Bit-exact parity of the fused-backward, folded-segment, pixel-shuffle and kernel-predictor paths on exact-lattice operands: the rows
of tests/fused_exact_cases.py, by the method of tests/test_conv_exact_gpu.py.  These kernels write SECOND outputs -- d(res), bias and
PReLU-slope gradient sums through per-workgroup partial rows in the reduction scratch, weight-gradient slabs -- which a tolerance on the
main output does not see.  On the lattice each has an exact answer (the bounds are proved on the reference by the case builders), so
every output is compared with ``torch.equal``.  Per row:
  * the kernel ID and instance reached, where the path records one;
  * operands as channel slices of NaN-filled wider buffers, outputs as NaN-prefilled slices of canary-filled buffers with a guard row;
  * the reduction scratch, the slab workspace and every uninitialised fp32 buffer the engine hands out refilled with NaN before a launch;
  * accumulators zeroed before the run, and a second launch that must give exactly twice the sums;
  * the persistent-grid rows again under CU budgets 1, 3 and 7 (the number of partial rows / slabs follows the budget): bit-identical."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

import exact_lattice as XL
import fused_exact_cases as FC
from fused_exact_cases import BUDGETS, FUSED_ROWS, SLOPE
from test_conv_exact_gpu import Budget, Guarded, _L, _apply_modes, _fm, _from_fm, _poison_scratch, _restore_modes, pad8

pytestmark = pytest.mark.gpu

BY_GROUP = {}
for _r in FUSED_ROWS:
    BY_GROUP.setdefault(_r.group, []).append(_r)


def _rows(group):
    return pytest.mark.parametrize("row", BY_GROUP[group], ids=[r.name for r in BY_GROUP[group]])


def _eng():
    from csbsr_amd.engine import Engine
    return Engine("cuda:0")


@contextlib.contextmanager
def poisoned(eng):
    """NaN in the reduction scratch, in the slab workspace and in every uninitialised fp32 buffer the engine hands out"""
    ws, f32 = type(eng).workspace, type(eng).f32

    def workspace(nfloat):
        t = ws(eng, nfloat)
        t.fill_(float("nan"))
        return t

    def f32_(*shape, zero=True):
        t = f32(eng, *shape, zero=zero)
        if not zero:
            t.fill_(float("nan"))
        return t
    eng.workspace, eng.f32 = workspace, f32_
    _poison_scratch()
    try:
        yield
        torch.cuda.synchronize()
    finally:
        del eng.workspace, eng.f32


def _kid(lib):
    k = int(lib.csbsr_debug_last_conv_kernel())
    return k & 255, k >> 8


def _check_kid(lib, row, what, kid=None, var=None):
    kid, var = row.kid if kid is None else kid, row.var if var is None else var
    got = _kid(lib)
    assert got[0] == kid and (var is None or got[1] == var), \
        f"{row.name} {what}: reached conv kernel {got[0]} instance {got[1]}, the table says {kid} / {var} ({row.why})"


def _eq(got, ref, what):
    assert torch.equal(got, ref), f"{what}: {XL.mismatch(got, ref)}"


def _gacc(p):
    g = getattr(p, "gacc", None)
    return None if g is None else g.detach().cpu().clone()


def _zero_acc(*ps):
    for p in ps:
        if getattr(p, "gacc", None) is not None:
            p.gacc.zero_()


def _runs(row):
    """(what, output channel offset, input channel offset, CU budget): the plain launch, NaN around the operands, the CU budgets"""
    runs = [("plain", 0, None, 0), ("output at channel 128, inputs at channel 64 (NaN around them)", 128, 64, 0)]
    return runs + ([(f"CU budget {n}", 0, None, n) for n in BUDGETS] if row.budget else [])


@contextlib.contextmanager
def _budget(ncu):
    if ncu:
        with Budget(ncu):
            yield
    else:
        yield


# ---------------------------------------------------------------------------------------------------------------- conv_tp + dact

def _tp_layers(eng, c, frozen):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    conv = Conv(eng, "l", {"l.weight": c.w.cuda()}, 8, 4, 2, 1, bias=False, act=L.ACT_NONE)
    pb = {"b.weight": torch.zeros(c.C, c.C, 8, 8).cuda(), "b.bias": c.bias0.cuda(), "a": torch.tensor([SLOPE]).cuda()}
    below = Conv(eng, "b", pb, 8, 4, 2, 1, transposed=True, bias=True, act=L.ACT_PRELU, prelu="a")
    below.frozen = frozen
    return conv, below, pb


def _tp_launch(eng, c, conv, below, out_c0, in_c0):
    from csbsr_amd import _lib as L
    gd = Guarded(c.N, c.IH, c.IW, c.C, out_c0, c.old)
    gr, kw = None, {}
    if c.res_mode is not None:
        gr = Guarded(c.N, c.IH, c.IW, c.C, out_c0)
        kw["dres"] = (_fm(c.res, in_c0), gr.fm, L.RES_SUB if c.res_mode == "sub" else L.RES_ADD)
    with poisoned(eng):
        conv.bwd_input(_fm(c.dpre, in_c0), out=gd.fm, accumulate=c.acc, in_hw=(c.IH, c.IW), dact=(below, _fm(c.saved, in_c0)), **kw)
    return gd, gr


@_rows("tp_dact")
def test_tp_dgrad_with_the_layer_belows_sums(row):
    lib = _L().load()
    c = FC.build(row)
    eng = _eng()
    conv, below, pb = _tp_layers(eng, c, False)
    lib.csbsr_debug_set_conv_tp(2)
    try:
        base = None
        for what, out_c0, in_c0, ncu in _runs(row):
            what = f"{row.name} {what}"
            _zero_acc(pb["b.bias"], pb["a"])
            for rep in (1, 2):          # the second launch adds to the accumulators: exactly twice
                with _budget(ncu):
                    gd, gr = _tp_launch(eng, c, conv, below, out_c0, in_c0)
                assert conv.last_fused, what
                _check_kid(lib, row, what)
                got = [_from_fm(gd.fm), _gacc(pb["b.bias"]), _gacc(pb["a"]).reshape(()), None if gr is None else _from_fm(gr.fm)]
                _eq(got[0], c.dz, what + ": dz")
                gd.check(what)
                _eq(got[1], rep * c.db, what + f": bias gradient sums after launch {rep}")
                _eq(got[2], rep * c.da, what + f": slope gradient sum after launch {rep}")
                if gr is not None:
                    _eq(got[3], c.dres, what + ": d(res)")
                    gr.check(what + ": d(res)")
                if rep == 1:
                    if base is None:
                        base = got
                    for a, b in zip(got, base):
                        assert a is None or torch.equal(a, b), f"{what}: differs from the plain launch: {XL.mismatch(a, b)}"
    finally:
        _restore_modes(lib)


def test_tp_dgrad_below_a_frozen_layer():
    """a frozen layer below: the gradient is masked, no sums are taken (instance 6), no accumulator is created"""
    lib = _L().load()
    row = BY_GROUP["tp_dact"][0]
    c = FC.build(row)
    eng = _eng()
    conv, below, pb = _tp_layers(eng, c, True)
    lib.csbsr_debug_set_conv_tp(2)
    try:
        gd, _ = _tp_launch(eng, c, conv, below, 0, None)
        _check_kid(lib, row, "frozen", 9, 6)
        _eq(_from_fm(gd.fm), c.dz, "frozen layer below: dz")
        gd.check("frozen layer below")
        assert _gacc(pb["b.bias"]) is None and _gacc(pb["a"]) is None
    finally:
        _restore_modes(lib)


def test_tp_dgrad_declines_the_sums_on_part_tiles():
    """a 12 x 32 dPre is not whole 8 x 32 tiles: the launch declines (``last_fused`` False), the gradient leaves unmasked for the
    stand-alone pass and the accumulators are untouched"""
    lib = _L().load()
    row = BY_GROUP["tp_dact"][0]
    c = FC.build_tp_dact(row, H=12, W=32)
    eng = _eng()
    conv, below, pb = _tp_layers(eng, c, False)
    lib.csbsr_debug_set_conv_tp(2)
    try:
        gd, _ = _tp_launch(eng, c, conv, below, 0, None)
        assert not conv.last_fused
        _eq(_from_fm(gd.fm), c.tot, "part tiles: the unmasked gradient")
        gd.check("part tiles")
        for p in (pb["b.bias"], pb["a"]):
            g = _gacc(p)
            assert g is None or not bool(g.any()), "part tiles: an accumulator was written"
    finally:
        _restore_modes(lib)


# ---------------------------------------------------------------------------------------------------------------- thin DACT

@_rows("thin_dact")
def test_thin_input_dgrad_with_the_layer_belows_sums(row):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    lib = L.load()
    c = FC.build(row)
    eng = _eng()
    eng.thin_dact = True
    head = Conv(eng, "l", {"l.weight": c.w.cuda()}, 3, 1, 1, 1, bias=False)
    pb = {"b.weight": torch.zeros(8, c.cout, 8, 8).cuda(), "b.a": torch.tensor([SLOPE]).cuda()}
    below = Conv(eng, "b", pb, 8, 4, 2, 1, transposed=True, bias=False, act=L.ACT_PRELU, prelu="b.a")
    below.frozen = False
    for what, out_c0, in_c0, _ in _runs(row):
        what = f"{row.name} {what}"
        _zero_acc(pb["b.a"])
        for rep in (1, 2):
            gd, gr = Guarded(c.N, c.H, c.W, c.cout, out_c0, c.old), Guarded(c.N, c.H, c.W, c.cout, out_c0)
            with poisoned(eng):
                head.bwd_input(_fm(c.dimg, in_c0), out=gd.fm, accumulate=True, dact=(below, _fm(c.saved, in_c0)),
                               dres=(_fm(c.res, in_c0), gr.fm, L.RES_ADD if c.res_mode == "add" else L.RES_SUB))
            assert head.last_fused, what
            _check_kid(lib, row, what)
            _eq(_from_fm(gd.fm), c.dz, what + ": dz")
            _eq(_from_fm(gr.fm), c.dres, what + ": d(res)")
            gd.check(what)
            gr.check(what + ": d(res)")
            _eq(_gacc(pb["b.a"]).reshape(()), rep * c.da, what + f": slope gradient sum after launch {rep}")


# ---------------------------------------------------------------------------------------------------------------- conv_kbup

def _kbup_layer(eng, c):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    params = {"l.weight": c.wt.cuda(), "l.a": torch.tensor([SLOPE]).cuda()}
    return Conv(eng, "l", params, 8, 4, 2, 1, transposed=True, bias=False, act=L.ACT_PRELU, prelu="l.a"), params


@_rows("kbup")
def test_one_pass_backward_of_the_thin_transposed_prelu_layer(row):
    c = FC.build(row)
    eng = _eng()
    for what, out_c0, in_c0, _ in _runs(row):
        what = f"{row.name} {what}"
        conv, params = _kbup_layer(eng, c)
        for rep in (1, 2):
            fx, fd = _fm(c.x, in_c0), _fm(c.dout, in_c0)
            assert conv.thin_tp_fused_ok(fx)
            before = fd.t.clone()
            gd = Guarded(c.N, 4 * c.h, 4 * c.w, c.cout, out_c0)
            with poisoned(eng):
                conv.bwd_thin_tp_fused(fd, fx, gd.fm)
            _eq(_from_fm(gd.fm), c.dpre, what + ": dPre")
            gd.check(what)
            assert torch.equal(fd.t.view(torch.int16), before.view(torch.int16)), what + ": dOut was written"
            _eq(_gacc(params["l.weight"]), rep * c.dw, what + f": weight gradient after launch {rep}")
            _eq(_gacc(params["l.a"]).reshape(()), rep * c.da, what + f": slope gradient after launch {rep}")
    # a frozen layer: dPre alone, no accumulator
    conv, params = _kbup_layer(eng, c)
    gd = Guarded(c.N, 4 * c.h, 4 * c.w, c.cout, 0)
    with poisoned(eng):
        conv.bwd_thin_tp_fused(_fm(c.dout), _fm(c.x), gd.fm, frozen=True)
    _eq(_from_fm(gd.fm), c.dpre, row.name + " frozen: dPre")
    gd.check(row.name + " frozen")
    assert _gacc(params["l.weight"]) is None and _gacc(params["l.a"]) is None


# ---------------------------------------------------------------------------------------------------------------- folded constant segment

@_rows("folded_fwd")
def test_forward_with_folded_constant_segment(row):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    lib = L.load()
    c = FC.build(row)
    eng = _eng()
    mtap = FC.border_tap_mask().cuda()
    try:
        _apply_modes(lib, eng, c.modes)
        conv = Conv(eng, "l", {"l.weight": c.w.cuda(), "l.bias": c.b.cuda()}, 3, 1, 1, 1, bias=True, act=L.ACT_LRELU, slope=SLOPE,
                    split=(c.cf, c.cc))
        base = None
        for what, out_c0, in_c0, ncu in _runs(row):
            what = f"{row.name} {what}"
            gd = Guarded(c.N, c.H, c.W, c.cout, out_c0)
            with _budget(ncu), poisoned(eng):
                conv.fwd_folded(_fm(c.x, in_c0), c.kvec.cuda(), mtap, out=gd.fm)
            _check_kid(lib, row, what)
            got = _from_fm(gd.fm)
            _eq(got, c.ref, what)
            gd.check(what)
            base = got if base is None else base
            _eq(got, base, what + ": against the plain launch")
    finally:
        _restore_modes(lib)


@_rows("folded_bwd")
def test_weight_gradient_with_folded_constant_segment(row):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    c = FC.build(row)
    eng = _eng()
    mtap = FC.border_tap_mask().cuda()

    def layer():
        params = {"l.weight": c.w.cuda(), "l.bias": torch.zeros(c.cout).cuda()}
        if not c.prelu:
            return Conv(eng, "l", params, 3, 1, 1, 1, bias=True, act=L.ACT_LRELU, slope=SLOPE, split=(c.cf, c.cc)), params
        params["l.a"] = torch.tensor([SLOPE]).cuda()
        return Conv(eng, "l", params, 3, 1, 1, 1, bias=True, act=L.ACT_PRELU, prelu="l.a", split=(c.cf, c.cc)), params
    for what, _, in_c0, _ in _runs(row):
        what = f"{row.name} {what}"
        conv, params = layer()
        for rep in (1, 2):
            with poisoned(eng):
                dk = conv.bwd_weights_folded(_fm(c.dpre, in_c0), _fm(c.x, in_c0), (conv.w[:, c.cf:], c.kvec.cuda()), mtap, bias_grad=True,
                                             prelu_out=_fm(c.out, in_c0) if c.prelu else None)
            _eq(dk.cpu(), c.dk, what + ": dL/dk")
            _eq(_gacc(params["l.weight"]), rep * c.dw, what + f": weight gradient (both halves) after launch {rep}")
            _eq(_gacc(params["l.bias"]), rep * c.db, what + f": bias gradient after launch {rep}")
            if c.prelu:
                _eq(_gacc(params["l.a"]).reshape(()), rep * c.da, what + f": slope gradient after launch {rep}")
    conv, params = layer()
    with poisoned(eng):
        dk = conv.bwd_weights_folded(_fm(c.dpre), _fm(c.x), (conv.w[:, c.cf:], c.kvec.cuda()), mtap, frozen=True, bias_grad=True,
                                     prelu_out=_fm(c.out) if c.prelu else None)
    _eq(dk.cpu(), c.dk, row.name + " frozen: dL/dk")
    assert all(_gacc(p) is None for p in params.values()), row.name + " frozen: an accumulator was created"


def test_slope_sum_of_the_folded_backward_refuses_small_maps():
    """``prelu_out`` has a kernel from 1024 pixels on (the callers test that): below, the library reports an error -- no silent fall-back,
    no accumulator written"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    c = FC.build(BY_GROUP["folded_bwd"][0])
    assert c.H * c.W < 1024
    eng = _eng()
    params = {"l.weight": c.w.cuda(), "l.a": torch.tensor([SLOPE]).cuda()}
    conv = Conv(eng, "l", params, 3, 1, 1, 1, bias=False, act=L.ACT_PRELU, prelu="l.a", split=(c.cf, c.cc))
    with pytest.raises(L.CsbsrHipError, match="1024 pixels"):
        conv.bwd_weights_folded(_fm(c.dpre), _fm(c.x), (conv.w[:, c.cf:], c.kvec.cuda()), FC.border_tap_mask().cuda(), prelu_out=_fm(c.out))
    torch.cuda.synchronize()
    assert _gacc(params["l.a"]) is None


@_rows("const_1x1")
def test_1x1_with_constant_first_segment(row):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    lib = L.load()
    c = FC.build(row)
    eng = _eng()
    params = {"l.weight": c.w.cuda()}
    if c.b is not None:
        params["l.bias"] = c.b.cuda()
    conv = Conv(eng, "l", params, 1, 1, 0, 1, bias=c.b is not None, act=L.ACT_NONE if c.stat else L.ACT_LRELU, slope=SLOPE, split=(c.c0, c.c1))
    for what, out_c0, in_c0, _ in _runs(row):
        what = f"{row.name} {what}"
        gd = Guarded(c.N, c.H, c.W, c.cout, out_c0)
        stat = torch.zeros(2, pad8(c.cout), device="cuda") if c.stat else None
        with poisoned(eng):
            conv.fwd_const_1x1(c.cvec.cuda(), _fm(c.x, in_c0), out=gd.fm, stat=stat, stat_mode=L.STAT_BN if c.stat else L.STAT_NONE)
        _check_kid(lib, row, what)
        _eq(_from_fm(gd.fm), c.ref, what)
        gd.check(what)
        if c.stat:
            _eq(stat[:, :c.cout].cpu(), c.ref_stat, what + ": BatchNorm sums")


# ---------------------------------------------------------------------------------------------------------------- ShuffleConv

def _shuffle_layer(eng, c, W):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import ShuffleConv
    params = {"l.weight": W.clone().cuda(), "l.a": torch.tensor([SLOPE]).cuda()}
    return ShuffleConv(eng, "l", params, c.s, act=L.ACT_PRELU, prelu="l.a"), params


@_rows("shuffle")
def test_pixel_shuffle_conv(row):
    lib = _L().load()
    c = FC.build(row)
    eng = _eng()
    s = c.s
    conv, params = _shuffle_layer(eng, c, c.Wm)
    assert torch.equal(conv._unmap(conv._remap(params["l.weight"])), params["l.weight"])
    for what, out_c0, in_c0, _ in _runs(row):
        what = f"{row.name} {what}"
        gd = Guarded(c.N, s * c.H, s * c.W, c.C, out_c0)
        conv.fwd(_fm(c.x, in_c0), out=gd.fm)
        torch.cuda.synchronize()
        _check_kid(lib, row, what + " forward", row.kid[0], row.var[0])
        _eq(_from_fm(gd.fm), c.ref, what + ": forward")
        gd.check(what)
    # the weight gradient, in the master layout; the derived accumulator is drained
    for rep in (1, 2):
        with poisoned(eng):
            conv.bwd_weights(_fm(c.dpre_w, 64), _fm(c.x, 64))
        _eq(_gacc(params["l.weight"]), rep * c.dW, f"{row.name}: weight gradient in the master layout after launch {rep}")
        assert int(lib.csbsr_debug_last_wgrad_kernel()) == row.kid[2], (row.name, int(lib.csbsr_debug_last_wgrad_kernel()), row.why)
        assert not bool(conv.w.gacc.any()), f"{row.name}: the derived weight's accumulator is not zero"
    # an optimiser step: new master weights + invalidate(); a stale derived weight or pack would give the old forward
    params["l.weight"].copy_(c.Wm2.cuda())
    conv.invalidate()
    gd = Guarded(c.N, s * c.H, s * c.W, c.C, 0)
    conv.fwd(_fm(c.x), out=gd.fm)
    torch.cuda.synchronize()
    _eq(_from_fm(gd.fm), c.ref2, f"{row.name}: forward after invalidate()")
    # dgrad (its own, sparser weights)
    conv, params = _shuffle_layer(eng, c, c.Wd)
    for what, out_c0, in_c0, _ in _runs(row):
        what = f"{row.name} {what}"
        gd = Guarded(c.N, c.H, c.W, c.cin, out_c0)
        conv.bwd_input(_fm(c.dpre, in_c0), out=gd.fm, in_hw=(c.H, c.W))
        torch.cuda.synchronize()
        _check_kid(lib, row, what + " dgrad", row.kid[1], row.var[1])
        _eq(_from_fm(gd.fm), c.dx, what + ": dgrad")
        gd.check(what)


# ---------------------------------------------------------------------------------------------------------------- kp_bwd

@_rows("pair")
def test_pair_1x1_backward(row):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    from csbsr_amd.modeling.kp_bwd import pair1x1_backward, pair1x1_ok
    c = FC.build(row)
    eng = _eng()
    split = (c.cin, c.cin_tot - c.cin) if c.cin_tot > c.cin else None
    ref_conv = Conv(eng, "l", {"l.weight": c.w.cuda()}, 1, 1, 0, 1, bias=False, act=L.ACT_NONE, split=split)
    two = ref_conv.bwd_input(_fm(c.dpre), seg=0, mask=(_fm(c.x), SLOPE))
    torch.cuda.synchronize()
    _eq(_from_fm(two), c.din, row.name + ": Conv.bwd_input(mask=)")
    for what, _, in_c0, ncu in _runs(row):
        what = f"{row.name} {what}"
        p = {"l.weight": c.w.cuda()}
        conv = Conv(eng, "l", p, 1, 1, 0, 1, bias=False, act=L.ACT_NONE, split=split)
        for rep in (1, 2):
            dfm, xfm = _fm(c.dpre, in_c0), _fm(c.x, in_c0)
            assert pair1x1_ok(conv, dfm, xfm)
            with _budget(ncu), poisoned(eng):
                din = pair1x1_backward(conv, dfm, xfm, SLOPE)
            _eq(_from_fm(din), c.din, what + ": dIn")
            assert torch.equal(din.t.view(torch.int16), two.t.view(torch.int16)), what + ": dIn (pad channels included) differs from Conv.bwd_input(mask=)"
            assert not bool(din.t[..., c.cin:].any()), what + ": pad channels [49, 56) not zero"
            # (the 98-column case: columns from 49 on belong to another writer and stay zero, as in the reference)
            _eq(_gacc(p["l.weight"]), rep * c.dw, what + f": weight gradient after launch {rep}")


@_rows("fillsums")
def test_masked_fill_with_class_sums_and_the_fold(row):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    from csbsr_amd.modeling.kbpn import KBPN, border_tap_mask
    from csbsr_amd.modeling.kp_bwd import const_wgrad_ok, fold_const_wgrad
    c = FC.build(row)
    eng = _eng()
    assert torch.equal(border_tap_mask(), FC.border_tap_mask())
    stub = SimpleNamespace(eng=eng, Mtap=border_tap_mask().cuda())
    for what, _, in_c0, _ in _runs(row):
        what = f"{row.name} {what}"
        p = {"l.weight": c.w.cuda()}
        conv = Conv(eng, "l", p, 3, 1, 1, 1, bias=False, act=L.ACT_LRELU, slope=SLOPE)
        assert const_wgrad_ok(conv)
        for rep in (1, 2):
            xfm = _fm(c.x, in_c0)
            sums = torch.zeros(c.N, 16, xfm.cp, device="cuda")
            with poisoned(eng):
                out = KBPN._fold_const_dgrad(stub, conv, c.g.cuda(), (xfm, SLOPE), c.H, c.W, sums=sums)
                fold_const_wgrad(conv, c.g.cuda(), sums, stub.Mtap)
            _eq(sums[:, :, :c.cin].cpu(), c.sums, what + ": border-class sums")
            _eq(_from_fm(out), c.din, what + ": masked fill")
            _eq(_gacc(p["l.weight"]), rep * c.dw, what + f": folded weight gradient after launch {rep}")
