"""Kernel-level accuracy of the split-fp16 (hi + lo) launch paths of csrc/elementwise.hip, every case with lo != 0 and in two layouts: a
whole [hi | lo] map (lo == cp) and channels [8, 8 + c) of a split buffer c + 24 channels wide (ld = 2 cp_total, lo = cp_total), where
every element outside the slice holds a canary that must survive the launch.  Inputs, fp64 references, fp32 emulations and the case table
come from tests/split_cases.py; test_split_planes_cpu.py shows that a kernel which drops a lo plane cannot meet the bounds asserted here.

Bit-exact cases (both planes equal the emulation's split_store): layout conversion, max pool forward / backward, axpby with unit
coefficients, sum_act.  Bounded cases: |got - ref64| <= |ref64| 2^-22 + 2^-25 + 4 E_op, E_op = max |fp32 emulation - ref64| on the case's
inputs (fp32 output of the weighted pool: |ref64| 2^-24 + 4 E_op).

entry point / wrapper                  kernel                       cases
Engine.nchw32_to_fm                    nchw32_to_nhwc16_kernel      convert-*
csbsr_maxpool3x3s2_fwd_split           maxpool_fwd_kernel           maxpool-*
csbsr_maxpool3x3s2_bwd_split           maxpool_bwd_kernel           maxpool_bwd-*
csbsr_axpby_split                      axpby_kernel                 axpby-* (toplain: the y_lo == 0 branch)
hrnet_ocr.sum_act                      sum_act_kernel               sum_act-*
BatchNorm.apply / .backward            bn_apply_kernel, bn_bwd_reduce_kernel, bn_bwd_apply_kernel     bn-*
csbsr_adaptive_avgpool_fwd_split       aap_fwd_kernel               aap-8x8-{2,3,6}, aap-11x14-3x5
                                       aap_fwd_block_kernel         aap-8x8-1, aap-{20x20-2,17x19-2,24x24-3,16x16-1}-c{24,136}, the chain
Engine.bilinear                        bilinear_fwd_kernel          bilinear-{8x8-16x16,5x7-20x21-drop,6x6-1x1}
                                       bilinear_fwd_cols_kernel     bilinear-{23x31-50x70-drop,32x32-64x64}
csbsr_weighted_pool_fwd_split          wpool_fwd_kernel             wpool-*

Measured E_op (host, the inputs of split_cases.make_inputs; the assertion uses the value computed in the run, not this table; on the
MI355X the worst |error| / bound of any bounded case was 0.30):
  axpby-scaled 3.4e-07
  bn-3x16x9x10  none 5.9e-07 / drop 6.1e-07   relu 5.8e-07 / drop 7.6e-07   prelu 3.8e-07 / drop 5.9e-07
  bn-2x40x5x7   none 4.1e-07 / drop 5.2e-07   relu 3.8e-07 / drop 6.4e-07   prelu 6.3e-07 / drop 6.4e-07
  bn cancel rows: 3x16x9x10-relu-drop0 4.0e-07  3x16x9x10-prelu-drop1 6.4e-07  2x40x5x7-relu-drop1 9.0e-07  2x40x5x7-prelu-drop0 2.6e-07
  aap c24:  8x8-1 4.0e-08  8x8-2 1.0e-07  8x8-3 1.2e-07  8x8-6 1.5e-07  11x14-3x5 1.3e-07
            20x20-2 4.8e-08  17x19-2 3.6e-08  24x24-3 6.5e-08  16x16-1 2.7e-08
  aap c136: 20x20-2 7.8e-08  17x19-2 5.7e-08  24x24-3 9.5e-08  16x16-1 2.8e-08
  bilinear (align False / True): 8x8-16x16 2.9e-07 / 4.0e-07   5x7-20x21-drop 6.2e-07 / 5.2e-07   6x6-1x1 1.8e-07 / 0
                                 23x31-50x70-drop 2.9e-06 / 2.0e-06   32x32-64x64 4.6e-07 / 1.8e-06
  wpool: 1023-c64 2.1e-07  1023-c320 1.4e-07  2100-c64 7.1e-08  2100-c320 3.9e-07
  chain stages: convert 0, bn 2.4e-07, maxpool 0, aap 3.3e-07, bilinear 1.9e-07, axpby 2.4e-07 -> propagated bound 1.3e-05

The backward's mask (bn_bwd_* recompute z as ((x - mean) invstd) gamma + beta + res, bn_apply as (x - mean) (invstd gamma) + beta + res): on
random inputs it never disagreed with the sign of the forward's output; on the cancel rows (a quarter of z within ~2^-23 |x| of 0) it
disagreed at 233 of 4320, 157 of 3420, 87 of 1925 and 149 of 2800 elements, every one of them with |z64| <= E_op.
"""
import pytest
import torch
import torch.nn.functional as F

import split_cases as S

pytestmark = pytest.mark.gpu

LAYOUTS = ("whole", "slice")
I16 = torch.int16


def _eng():
    from csbsr_amd.engine import Engine
    return Engine("cuda:0")


def P(t):
    from csbsr_amd.engine import _ptr
    return _ptr(t)


def _kw(c, layout):
    return {} if layout == "whole" else {"c_total": c + S.SLICE_EXTRA, "c0": S.SLICE_C0}


def up(eng, pair, layout):
    return S.to_split_fm(eng, pair, **_kw(pair.hi.shape[1], layout))


def new_out(eng, N, H, W, c, layout, split=True):
    return S.empty_split_fm(eng, N, H, W, c, split=split, **_kw(c, layout))


def cases(op, **where):
    return [pytest.param(c, id=c.id) for c in S.CASES if c.op == op and all(c.p.get(k) == v for k, v in where.items())]


def check_exact(fm, out32, what=""):
    """both planes bit for bit the split_store of the emulation (a plain map: hi == fp16 of it)"""
    hi, lo = S.planes(fm)
    eh, el = S.split_store(out32)
    n = int((hi.view(I16) != eh.view(I16)).sum())
    assert n == 0, f"{what}: {n} of {hi.numel()} hi elements differ"
    if fm.lo:
        n = int((lo.view(I16) != el.view(I16)).sum())
        assert n == 0, f"{what}: {n} of {lo.numel()} lo elements differ"


def check_bounded(got64, ref64, e_op, what, rel=S.FMT_REL, abs_=S.FMT_ABS):
    err = (got64 - ref64).abs()
    bound = ref64.abs() * rel + abs_ + S.MARGIN * e_op
    msg = (f"{what}: E_op {e_op:.3g} x {S.MARGIN:g}, worst |error| {float(err.max()):.3g}, worst error / bound {float((err / bound).max()):.3f}, "
           f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound")
    print(msg)
    assert (err <= bound).all(), msg


def finish(*fms):
    torch.cuda.synchronize()
    S.assert_canaries(*fms)


# ------------------------------------------------------------------------------------------------- bit-exact cases
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("convert"))
def test_convert(case, layout):
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    o = new_out(eng, N, H, W, C, layout)
    src = h.ins["src"].cuda()
    mean, invstd = (None, None) if h.ins["mean"] is None else (h.ins["mean"].reshape(-1).cuda(), h.ins["invstd"].reshape(-1).cuda())
    eng.nchw32_to_fm(src, mean=mean, invstd=invstd, out=o)
    finish(o)
    check_exact(o, h.out32, case.id)
    hi, lo = S.planes(o, padded=True)
    assert o.cp == S.pad8(C) and (hi[:, C:].view(I16) == 0).all() and (lo[:, C:].view(I16) == 0).all()     # padding channels: +0 in both planes


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("maxpool"))
def test_maxpool_fwd(case, layout):
    from csbsr_amd import _lib as L
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    x = up(eng, h.ins["x"], layout)
    o = new_out(eng, N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, layout)
    L.call("csbsr_maxpool3x3s2_fwd_split", P(x.t), x.ld, x.lo, P(o.t), o.ld, o.lo, N, H, W, C, eng.stream)
    finish(x, o)
    assert h.e_op == 0.0                # the emulation IS the true maximum of hi + lo
    check_exact(o, h.out32, case.id)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("maxpool_bwd"))
def test_maxpool_bwd(case, layout):
    """dx = dy scattered to the first maximum, in scan order, of the full hi + lo value"""
    from csbsr_amd import _lib as L
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    x64 = S.load(h.ins["x"], torch.float64).requires_grad_(True)
    F.max_pool2d(x64, 3, 2, 1).backward(h.ins["dy"].double())
    assert torch.equal(x64.grad, h.ref64)
    x = up(eng, h.ins["x"], layout)
    y = new_out(eng, N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, layout)          # (the saved output: an argument the kernel does not read)
    dy = S.to_split_fm(eng, S.SP(h.ins["dy"], None))
    dx = S.empty_split_fm(eng, N, H, W, C, split=False)
    L.call("csbsr_maxpool3x3s2_bwd_split", P(x.t), x.ld, x.lo, P(y.t), y.ld, y.lo, P(dy.t), P(dx.t), N, H, W, C, eng.stream)
    finish(x, y)
    got = S.planes(dx)[0]
    want = h.ref64.half()
    n = int((got.view(I16) != want.view(I16)).sum())
    assert n == 0, f"{case.id}: {n} of {got.numel()} gradient elements differ"
    assert torch.equal(h.out32.half().view(I16), want.view(I16))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("axpby"))
def test_axpby(case, layout):
    from csbsr_amd import _lib as L
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    x = up(eng, h.ins["x"], layout)
    z = None if h.ins["z"] is None else up(eng, h.ins["z"], layout)
    y = new_out(eng, N, H, W, C, layout, split=case.out == "split")
    assert y.lo == (0 if case.out == "plain" else y.ld // 2) and (z is None or bool(z.lo) == (case.p["variant"] != "mixed"))
    L.call("csbsr_axpby_split", N * H * W, C, P(x.t), x.ld, x.lo, h.ins["a"], None if z is None else P(z.t), 0 if z is None else z.ld,
           0 if z is None else z.lo, h.ins["b"], P(y.t), y.ld, y.lo, eng.stream)
    finish(x, y, *([] if z is None else [z]))
    if case.kind == "exact":
        check_exact(y, h.out32, case.id)
    else:
        check_bounded(S.from_split_fm(y), h.ref64, h.e_op, case.id)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("sum_act"))
def test_sum_act(case, layout):
    from csbsr_amd.modeling.hrnet_ocr import sum_act
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    terms = [up(eng, t, layout) for t in h.ins["terms"]]
    assert [bool(t.lo) for t in terms] == [bool(s) for s in case.p["split_terms"]]
    y = new_out(eng, N, H, W, C, layout)
    sum_act(eng, terms, case.p["relu"], out=y)
    finish(y, *terms)
    check_exact(y, h.out32, case.id)


# ------------------------------------------------------------------------------------------------- bounded cases
ACT = {"none": 0, "relu": 1, "prelu": 3}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("bn"))
def test_batchnorm(case, layout):
    """BatchNorm.apply on a split x and a split residual, then BatchNorm.backward on the same maps: plain-fp16 gradients against fp64
    autograd, and the backward's ReLU / PReLU mask against the sign of the forward's own output"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import BatchNorm
    assert (L.ACT_NONE, L.ACT_RELU, L.ACT_PRELU) == (ACT["none"], ACT["relu"], ACT["prelu"])
    eng, h, i = _eng(), S.host(case), S.host(case).ins
    N, C, H, W = case.p["shape"]
    act = case.p["act"]
    params = {"b.weight": i["gamma"].cuda(), "b.bias": i["beta"].cuda(), "b.running_mean": torch.zeros(C).cuda(),
              "b.running_var": torch.ones(C).cuda(), "b.num_batches_tracked": torch.zeros((), dtype=torch.long).cuda()}
    bn = BatchNorm(eng, "b", params, C)
    mean, invstd = i["mean"].cuda(), i["invstd"].cuda()
    slope = torch.tensor([i["slope"]], device="cuda") if act == "prelu" else None
    drop = None if i["drop"] is None else i["drop"].cuda()
    x, res = up(eng, i["x"], layout), up(eng, i["res"], layout)
    y = new_out(eng, N, H, W, C, layout)
    bn.apply(x, mean, invstd, act=ACT[act], prelu=slope, res=res, drop=drop, out=y)
    finish(x, res, y)
    y64 = S.from_split_fm(y)
    check_bounded(y64, h.ref64, h.e_op, case.id)

    # backward: fp64 autograd of train-mode batch norm on the uploaded values (its batch statistics are the mean / invstd handed in)
    x64, r64 = S.load(i["x"], torch.float64).requires_grad_(True), S.load(i["res"], torch.float64).requires_grad_(True)
    g64, b64 = i["gamma"].double().requires_grad_(True), i["beta"].double().requires_grad_(True)
    s64 = torch.tensor([i["slope"]], dtype=torch.float64, requires_grad=True)
    z64 = F.batch_norm(x64, None, None, g64, b64, True, 0.0, 1e-5) + r64
    yr = {"none": lambda v: v, "relu": F.relu, "prelu": lambda v: F.prelu(v, s64)}[act](z64)
    if drop is not None:
        yr = yr * i["drop"].double()[:, :, None, None]
    yr.backward(i["dy"].double())
    dy = S.to_split_fm(eng, S.SP(i["dy"], None))
    dres = eng.new(N, H, W, C)
    dpr = torch.zeros(1, device="cuda")
    dx = bn.backward(dy, x, mean, invstd, act=ACT[act], prelu=slope, res=res, drop=drop, dres=dres, dprelu=dpr if act == "prelu" else None)
    finish(x, res, y)
    relmax = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-20))
    if not case.p["cancel"]:        # (the cancel rows put a quarter of z within rounding of 0: there the fp64 mask is not the fp32 one, by design)
        assert relmax(S.from_split_fm(dx), x64.grad) < 5e-3
        assert relmax(params["b.weight"].gacc.cpu().double(), g64.grad) < 5e-3
        assert relmax(params["b.bias"].gacc.cpu().double(), b64.grad) < 5e-3
        assert relmax(S.from_split_fm(dres), r64.grad) < 3e-3
        if act == "prelu":
            assert abs(float(dpr) - float(s64.grad)) < 1e-2 * abs(float(s64.grad)) + 1e-2
    if act == "none":
        return
    # The mask the backward applied, recovered from dres = fp16(dz): dz = dy drop where it saw z > 0, else 0 (relu) / dy drop slope (prelu).
    # It must agree with the sign of the forward's own z (the device y: y > 0 iff z > 0 where drop > 0) except within E_op of z = 0.
    gg = i["dy"].float() * (1.0 if i["drop"] is None else i["drop"][:, :, None, None])
    pos, neg = gg.half(), (gg * (i["slope"] if act == "prelu" else 0.0)).half()
    got = S.planes(dres)[0]
    valid = gg != 0
    assert ((got == pos) | (got == neg))[valid].all()
    bwd_pos, fwd_pos = got == pos, y64 > 0
    z_ref = S.op_bn(x64.detach(), r64.detach(), i["mean"].double(), i["invstd"].double(), g64.detach(), b64.detach(), "none", 0.0, None)
    differ = valid & (bwd_pos != fwd_pos)
    near = valid & (z_ref.abs() <= h.e_op)
    far = differ & ~near
    print(f"{case.id} [{layout}]: backward mask != sign of the forward output at {int(differ.sum())} of {int(valid.sum())} elements "
          f"({int(near.sum())} have |z| <= E_op = {h.e_op:.3g}); {int(far.sum())} of them beyond E_op, worst |z| there "
          f"{float(z_ref.abs()[far].max()) if far.any() else 0.0:.3g}")
    assert not far.any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("aap"))
def test_adaptive_avgpool(case, layout):
    from csbsr_amd import _lib as L
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    OH, OW = case.p["osize"]
    x = up(eng, h.ins["x"], layout)
    y = new_out(eng, N, OH, OW, C, layout)
    L.call("csbsr_adaptive_avgpool_fwd_split", P(x.t), x.ld, x.lo, P(y.t), y.ld, y.lo, N, H, W, C, OH, OW, eng.stream)
    finish(x, y)
    check_bounded(S.from_split_fm(y), h.ref64, h.e_op, f"{case.id} ({'block' if case.p['block'] else 'per-bin'} kernel)")


@pytest.mark.parametrize("case", cases("aap", block=True))
def test_adaptive_avgpool_block_kernel_plain(case):
    """the plain entry point (lo = 0) at the block kernel's shapes, against torch at the plain-fp16 tolerance"""
    from csbsr_amd import _lib as L
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    OH, OW = case.p["osize"]
    x = S.to_split_fm(eng, S.SP(h.ins["x"].hi, None))
    y = S.empty_split_fm(eng, N, OH, OW, C, split=False)
    L.call("csbsr_adaptive_avgpool_fwd", P(x.t), x.ld, P(y.t), N, H, W, C, OH, OW, eng.stream)
    torch.cuda.synchronize()
    ref = F.adaptive_avg_pool2d(h.ins["x"].hi.float(), (OH, OW))
    assert float((S.planes(y)[0].float() - ref).abs().max() / ref.abs().max()) < 2e-3


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("bilinear"))
def test_bilinear(case, layout):
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    OH, OW = case.p["osize"]
    x = up(eng, h.ins["x"], layout)
    y = new_out(eng, N, OH, OW, C, layout)
    drop = None if h.ins["drop"] is None else h.ins["drop"].cuda()
    eng.bilinear(x, OH, OW, case.p["align"], out=y, drop=drop)
    finish(x, y)
    check_bounded(S.from_split_fm(y), h.ref64, h.e_op, f"{case.id} ({'column' if case.p['cols'] else 'row'} kernel)")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", cases("wpool"))
def test_weighted_pool(case, layout):
    from csbsr_amd import _lib as L
    eng, h = _eng(), S.host(case)
    N, C, H, W = case.p["shape"]
    x = up(eng, h.ins["x"], layout)
    w = h.ins["w"].cuda()
    out = torch.zeros(N, C, device="cuda")
    L.call("csbsr_weighted_pool_fwd_split", P(x.t), x.ld, x.lo, P(w), P(out), N, H * W, C, eng.stream)
    finish(x)
    check_bounded(out.cpu().double(), h.ref64, h.e_op, case.id, rel=2.0 ** -24, abs_=0.0)


# ------------------------------------------------------------------------------------------------- the composed chain
@pytest.mark.parametrize("layout", LAYOUTS)
def test_chain(layout):
    """layout conversion -> BN (relu) -> max pool -> adaptive pool to 2 -> bilinear back -> axpby onto the pooled map, every map split, against
    the same chain in fp64; the bound is propagated from the per-stage E_op (split_cases.chain_host)"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import BatchNorm
    eng = _eng()
    ins, r, em, e_op, e = S.chain_host()
    N, C, H, W = S.CHAIN_SHAPE
    cp, PH, PW = S.CHAIN_CP, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    params = {"b.weight": ins["gamma"].cuda(), "b.bias": ins["beta"].cuda(), "b.running_mean": torch.zeros(cp).cuda(),
              "b.running_var": torch.ones(cp).cuda(), "b.num_batches_tracked": torch.zeros((), dtype=torch.long).cuda()}
    mean, invstd, src = ins["mean"].cuda(), ins["invstd"].cuda(), ins["src"].cuda()
    m = {"convert": eng.nchw32_to_fm(src, out=new_out(eng, N, H, W, C, layout))}
    m["bn"] = BatchNorm(eng, "b", params, cp).apply(m["convert"], mean, invstd, act=L.ACT_RELU, out=new_out(eng, N, H, W, cp, layout))
    m["maxpool"], m["aap"] = new_out(eng, N, PH, PW, cp, layout), new_out(eng, N, 2, 2, cp, layout)
    a, b = m["bn"], m["maxpool"]
    L.call("csbsr_maxpool3x3s2_fwd_split", P(a.t), a.ld, a.lo, P(b.t), b.ld, b.lo, N, H, W, cp, eng.stream)
    a, b = m["maxpool"], m["aap"]
    L.call("csbsr_adaptive_avgpool_fwd_split", P(a.t), a.ld, a.lo, P(b.t), b.ld, b.lo, N, PH, PW, cp, 2, 2, eng.stream)
    m["bilinear"] = eng.bilinear(m["aap"], PH, PW, False, out=new_out(eng, N, PH, PW, cp, layout))
    m["axpby"] = new_out(eng, N, PH, PW, cp, layout)
    a, b, y = m["bilinear"], m["maxpool"], m["axpby"]
    L.call("csbsr_axpby_split", N * PH * PW, cp, P(a.t), a.ld, a.lo, 1.0, P(b.t), b.ld, b.lo, 1.0, P(y.t), y.ld, y.lo, eng.stream)
    finish(*m.values())
    for name, fm in m.items():
        got = torch.zeros_like(r[name])
        got[:, :fm.c] = S.from_split_fm(fm)
        err = float((got - r[name]).abs().max())
        msg = f"chain [{layout}] {name}: E_op {e_op[name]:.3g} x {S.MARGIN:g}, |device - fp64| {err:.3g}, propagated bound {e[name]:.3g}"
        print(msg)
        assert err <= e[name], msg
