"""Exact / bounded parity of the tail of a training step through the C ABI: the two multi-tensor optimiser steps of csrc/multi_tensor.hip
(csbsr_sgd_step, its four template instances; csbsr_adam_step) and the 1-channel head kernels of csrc/image_ops.hip (csbsr_head1_fwd
<8>, <16>, <32>; csbsr_head1_bwd_input; csbsr_sigmoid_bwd_to_nhwc8).  References, inputs, case tables, comparisons and the mutants that
show the inputs discriminate: tests/step_tail_cases.py (validated without a GPU by tests/test_step_tail_cases_cpu.py).  The guarded call
harness is tests/abi_harness.py: every input inside a NaN-filled allocation, every output inside a sentinel-filled one whose margins
(and, for a channel slice, other channels) are checked, tables and index arrays (abi_harness.Raw) compared byte for byte after the
call, every row twice with identical bits.

What is exact, what carries a bound, and why:

  sgd_step        operands on 2^-6, lr = 2^-3, momentum 1/2, weight decay 2^-4: every intermediate of two steps with decay (four
                  without) is fp32-exact, so the device's contracted multiply-adds have one result: p and buf BIT FOR BIT, per tensor,
                  for the list 0, 1, 3, 4, 5, 1023, 1028, 8191, 8192, 8193, 16387, 20000 and a vec = 0 tensor of 8197 elements whose p, g
                  and buf start 4 bytes into their allocations; the table's rows forward and reversed, the block list permuted, two
                  blocks past their tensor's end; the four (momentum != 0, weight_decay != 0) instances, buf = NULL without momentum.
  adam_step       beta1 = 1/2, beta2 = 3/4, eps = 2^-10, step_size and bc2_sqrt powers of two per tensor: every product that feeds an
                  add is exact; sqrt, / and the adds round once, correctly: p, m, v of three steps BIT FOR BIT against the float32
                  restatement.  This rests on fp32 / and sqrtf being correctly rounded on the device; see "Measured" below.
  rounded rows    the training hyper-parameters, one step from random state, against fp64: n 2^-24 sum|terms| with n = 6 (buf), 9 (p)
                  for SGD and 4 (m), 6 (v), 16 (p) for Adam, counted at step_tail_cases.SGD_N / ADAM_N.
  head1_fwd       lattice operands: the pre-activation t is exact in fp32 in any fold order: sigmoid = 0 BIT FOR BIT; sigmoid = 1 within
                  (|t| + 4) 2^-24 sigmoid64(t) (step_tail_cases.HEAD1_T_MAX: |t| <= 8, so within 7.2e-7 absolute).  c = 64, 128, 256;
                  whole maps and channel slices; hi alone and hi + lo (both planes in one NaN-filled allocation); npix on both sides of a
                  block, and one row per instance whose grid-stride loop takes a second turn (262 177, 131 089, 65 545 pixels).
  head1_bwd_input one fp32 product and the fp16 store: BIT FOR BIT against numpy float32 -> float16, lattice and random fp32 weights.
  sigmoid_bwd     ((dp p) (1 - p)) scale in float32 and the fp16 store: channels 1 .. 7 +0.0 bits; channel 0 BIT FOR BIT one of the two
                  roundings of the last product (to fp32 and then fp16, or once to fp16: see "Measured"), and against fp64 within
                  (3 x 2^-24 + 2^-11) |ref|.

The wrappers: csbsr_amd.optim.SGD and .Adam run three steps on lattice hyper-parameters with one parameter whose gradient is None in
step 2 (its step count lags), bit for bit against the restatement fed the host's Python-double formulas for step_size and bc2_sqrt.
Adam's step_size = lr / (1 - beta1^t) is no power of two from t = 2 on, so the last operation p - step_size q has two legitimate
results (fused or not); p is held to the sequences over {fused, unfused}^steps, m and v to their one result.  optim.Adam refuses a
tensor that is not 16-byte aligned before it creates state.

Measured on the MI355X: every bit-for-bit row identical, the three wrapper-level runs included (optim.Adam's p matched a fused /
unfused sequence in every element).  The assumption that fp32 / and sqrtf are correctly rounded HELD: the exact Adam rows agree with
numpy float32 in every element of p, m and v over three steps, inexact roots and quotients included.  One assumption of the design did
not hold: "no multiply feeds an add" does not keep csbsr_sigmoid_bwd_to_nhwc8 from contracting -- the compiler folds the product with
``scale`` and the fp16 store into one v_fma_mixlo_f16 (addend +0), which rounds once where the statement rounds twice and turns a -0
result into +0; step_tail_cases.sigb_compare accepts the two roundings per element and does not ask the sign of a zero (at scale 0.3,
113 of 2 097 155 elements take the once-rounded value; at scale 1 and 2^-3 the two are the same).  No kernel defect was found.
Worst error / bound of the bounded rows:
  sgd_step rounded        buf 0.38 (n = 6)   p 0.20 (n = 9)
  adam_step rounded       m 0.48 (n = 4)   v 0.45 (n = 6)   p 0.0625 (n = 16)
  head1_fwd sigmoid       n = |t| + 4;  c = 64: 0.44 (hi), 0.44 (hi + lo), wrap 0.44;  c = 128: 0.35, 0.43, wrap 0.55;  c = 256: 0.37, 0.40, wrap 0.55
  sigmoid_bwd against fp64  n = 3 and 2^-11 for the store: 0.96 (255 pixels), 0.95 (257), 0.999 (2 097 155), the same at every scale: the
                          store alone uses the whole 2^-11 |ref| at the bottom of a binade
Wall time of this module on the MI355X: 4.3 s for its 57 tests, the slowest 1.6 s (the first optimiser construction), a wrap row 0.25 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import step_tail_cases as S
from abi_harness import SENT, In16, In16Split, Out, Out16, Raw, _ptr, call, inp, same_bits, twice

pytestmark = pytest.mark.gpu
f32 = np.float32
FRONT_OUT, FRONT_IN = 0.5, 0.25          # the element in front of an unaligned view (an output's, an input's)


def _measured(what, ratios):
    for k, r in (ratios.items() if isinstance(ratios, dict) else [("", ratios)]):
        print(f"MEASURED {what} {k}: error / bound {r:.3g}")


def _addr(t, unaligned):
    return t.data_ptr() + (4 if unaligned else 0)


# ------------------------------------------------------------------------------------------- the optimiser steps

class _List:
    """the tensor list of one optimiser row on the device: per tensor one guarded output per state name (preset with the row's values)
    and one guarded input per step; the last tensor of an SGD list is a view that starts 4 bytes into each of its allocations"""

    def __init__(self, kind, state, gs):
        self.sizes = S.opt_sizes(kind)
        self.un = len(self.sizes) - 1 if kind == "sgd" else -1
        self.state = {k: [Out(n + (t == self.un), init=np.concatenate([[FRONT_OUT] * (t == self.un), v]))
                          for t, (n, v) in enumerate(zip(self.sizes, S.split(flat, self.sizes)))] for k, flat in state.items()}
        self.g_host = [[np.concatenate([[FRONT_IN] * (t == self.un), v]).astype(f32) for t, v in enumerate(S.split(g, self.sizes))] for g in gs]
        self.g = [[inp(v) for v in step] for step in self.g_host]

    def ptr(self, name, t, step=None):
        buf = self.state[name][t].v if step is None else self.g[step][t]
        return _addr(buf, t == self.un) if self.sizes[t] else buf.data_ptr()

    def flat(self, name):
        return np.concatenate([o.get()[(t == self.un):] for t, o in enumerate(self.state[name])])

    def check_guards(self, entry):
        for name, outs in self.state.items():
            for t, o in enumerate(outs):
                assert o.margins_intact(), f"{entry} wrote outside {name} of tensor {t}"
            if self.un >= 0:
                assert outs[self.un].get()[0] == FRONT_OUT, f"{entry} changed the element in front of the unaligned {name}"
        for step, host in zip(self.g, self.g_host):
            for t, (dev, h) in enumerate(zip(step, host)):
                assert same_bits(dev.cpu().numpy(), h), f"{entry} changed g of tensor {t}"


def _launch(entry, table, bt, bc, *scalars):
    """one guarded launch: the table and the two index arrays are the same bytes afterwards"""
    raws = [Raw(table.view(np.uint8)), Raw(bt), Raw(bc)]
    call(entry, *(r.ptr for r in raws), int(bt.size), *scalars)
    for r, what in zip(raws, ("the table", "block_tensor", "block_chunk")):
        assert r.unchanged(), f"{entry} changed {what}"


def run_sgd(row):
    from csbsr_amd.optim import _SGD_DT
    d = S.sgd_row_case(row)
    mom = row["momentum"] != 0
    L_ = _List("sgd", dict(p=d["p"], buf=d["buf"]) if mom else dict(p=d["p"]), d["g"])
    idx, bt, bc = S.block_map(L_.sizes, row["order"])
    for step in range(row["steps"]):
        tab = np.zeros(len(idx), dtype=_SGD_DT)
        for r, t in enumerate(idx):
            ptrs = (L_.ptr("p", t), L_.ptr("g", t, step), L_.ptr("buf", t) if mom else 0)
            vec = int(all(a % 16 == 0 for a in ptrs))
            assert vec == (t != L_.un)
            tab[r] = (*ptrs, L_.sizes[t], vec, 0)
        _launch("csbsr_sgd_step", tab, bt, bc, row["lr"], row["momentum"], row["weight_decay"])
    L_.check_guards("csbsr_sgd_step")
    return dict(p=L_.flat("p"), buf=L_.flat("buf") if mom else np.zeros(0, f32))


def _sgd_rows(kind):
    return [r for r in S.rows() if r["entry"] == "csbsr_sgd_step" and r["kind"] == kind]


@pytest.mark.parametrize("row", _sgd_rows("exact"), ids=lambda r: f"mom{r['momentum']}-wd{r['weight_decay']}-{r['order']}")
def test_sgd_step_exact(row):
    """p and buf bit for bit after two steps (with decay) or four (without); step 2 reads the buf step 1 wrote"""
    got = twice(lambda: run_sgd(row))
    S.sgd_compare(row, got["p"], got["buf"], f"sgd_step {row['instance']} {row['order']}")


def test_sgd_step_rounded():
    """lr 1e-2, momentum 0.9, weight decay 5e-4 on random operands, one step, against fp64: buf within 6, p within 9 roundings of the
    sum of the magnitudes of their terms (step_tail_cases.SGD_N)"""
    (row,) = _sgd_rows("rounded")
    got = twice(lambda: run_sgd(row))
    _measured("sgd_step rounded", S.sgd_compare(row, got["p"], got["buf"], "sgd_step rounded"))


def run_adam(row, nblocks=None):
    from csbsr_amd.optim import _DT
    d = S.adam_case(row["kind"])
    L_ = _List("adam", dict(p=d["p"], m=d["m"], v=d["v"]), d["g"])
    idx, bt, bc = S.block_map(L_.sizes, row["order"])
    for step in range(row["steps"]):
        tab = np.zeros(len(idx), dtype=_DT)
        for r, t in enumerate(idx):
            ptrs = (L_.ptr("p", t), L_.ptr("g", t, step), L_.ptr("m", t), L_.ptr("v", t))
            assert all(a % 16 == 0 for a in ptrs)
            tab[r] = (*ptrs, L_.sizes[t], *d["table"][t])
        _launch("csbsr_adam_step", tab, bt, bc, row["betas"][0], row["betas"][1], row["eps"])
    L_.check_guards("csbsr_adam_step")
    return dict(p=L_.flat("p"), m=L_.flat("m"), v=L_.flat("v"))


def _adam_rows(kind):
    return [r for r in S.rows() if r["entry"] == "csbsr_adam_step" and r["kind"] == kind]


@pytest.mark.parametrize("row", _adam_rows("exact"), ids=lambda r: r["order"])
def test_adam_step_exact(row):
    """p, m and v bit for bit after three steps against the float32 restatement (correctly rounded sqrt and /, exact products)"""
    got = twice(lambda: run_adam(row))
    S.adam_compare(row, got["p"], got["m"], got["v"], f"adam_step {row['order']}")


def test_adam_step_rounded():
    """lr 2e-5, betas (0.9, 0.999), eps 1e-8 with the bias corrections of step 3 on random operands, one step, against fp64: m within 4,
    v within 6, p within 16 roundings (step_tail_cases.ADAM_N)"""
    (row,) = _adam_rows("rounded")
    got = twice(lambda: run_adam(row))
    _measured("adam_step rounded", S.adam_compare(row, got["p"], got["m"], got["v"], "adam_step rounded"))


@pytest.mark.parametrize("entry", ["csbsr_sgd_step", "csbsr_adam_step"])
def test_no_blocks_is_a_no_op(entry):
    """nblocks = 0 returns 0 and touches nothing (the table names real tensors)"""
    from csbsr_amd import optim
    assert [r["kind"] for r in S.rows() if r["entry"] == entry].count("empty") == 1
    outs = [Out(8) for _ in range(4)]
    g = inp(np.ones(8))
    if entry == "csbsr_sgd_step":
        tab = np.zeros(1, dtype=optim._SGD_DT)
        tab[0] = (outs[0].v.data_ptr(), g.data_ptr(), outs[1].v.data_ptr(), 8, 1, 0)
        scalars = (0.125, 0.5, 0.0625)
    else:
        tab = np.zeros(1, dtype=optim._DT)
        tab[0] = (outs[0].v.data_ptr(), g.data_ptr(), outs[1].v.data_ptr(), outs[2].v.data_ptr(), 8, 0.25, 0.5)
        scalars = (0.5, 0.75, 2.0 ** -10)
    raws = [Raw(tab.view(np.uint8)), Raw(np.zeros(1, np.int32)), Raw(np.zeros(1, np.int32))]
    call(entry, *(r.ptr for r in raws), 0, *scalars)
    assert all(o.untouched() for o in outs) and all(r.unchanged() for r in raws)


def test_sgd_step_refuses_negative_hyper_parameters():
    """negative momentum or weight decay: status 1, csbsr_last_error set, nothing written"""
    from csbsr_amd import _lib as L
    from csbsr_amd.optim import _SGD_DT
    rows = _sgd_rows("refused")
    assert len(rows) == 2
    for row in rows:
        p, buf, g = Out(8), Out(8), inp(np.ones(8))
        tab = np.zeros(1, dtype=_SGD_DT)
        tab[0] = (p.v.data_ptr(), g.data_ptr(), buf.v.data_ptr(), 8, 1, 0)
        raws = [Raw(tab.view(np.uint8)), Raw(np.zeros(1, np.int32)), Raw(np.zeros(1, np.int32))]
        with pytest.raises(L.CsbsrHipError, match=r"\(1\): .*momentum and weight_decay must not be negative"):
            call("csbsr_sgd_step", *(r.ptr for r in raws), 1, 0.125, row["momentum"], row["weight_decay"])
        assert b"must not be negative" in L.load().csbsr_last_error()
        torch.cuda.synchronize()
        assert p.untouched() and buf.untouched()


# ------------------------------------------------------------------------------------------- the wrappers

def _params(case):
    return [torch.nn.Parameter(torch.from_numpy(c["p"]).float().cuda()) for c in case]


def _three_steps(opt, ps, case):
    for step in range(S.WRAP_STEPS):
        for k, (p, c) in enumerate(zip(ps, case)):
            p.grad = torch.from_numpy(c["g"][step]).float().cuda() if S.wrap_has_grad(k, step) else None
        opt.step()
    torch.cuda.synchronize()


def test_optim_sgd_three_steps_bit_for_bit():
    from csbsr_amd.optim import SGD
    case = S.wrap_case("sgd")
    ps = _params(case)
    opt = SGD(ps, **S.WRAP_SGD)
    _three_steps(opt, ps, case)
    for k, (p, c) in enumerate(zip(ps, case)):
        S.check_bits(p.detach().cpu().numpy(), c["ref_p"].astype(f32), f"optim.SGD parameter {k}")
        S.check_bits(opt.state[p]["momentum_buffer"].cpu().numpy(), c["ref_buf"].astype(f32), f"optim.SGD momentum buffer {k}")


def test_optim_adam_three_steps_bit_for_bit():
    from csbsr_amd.optim import Adam
    case = S.wrap_case("adam")
    ps = _params(case)
    opt = Adam(ps, **S.WRAP_ADAM)
    _three_steps(opt, ps, case)
    for k, (p, c) in enumerate(zip(ps, case)):
        st = opt.state[p]
        assert float(st["step"]) == c["t"] == (2 if k == 1 else 3)
        S.check_bits(st["exp_avg"].cpu().numpy(), c["ref_m"], f"optim.Adam exp_avg {k}")
        S.check_bits(st["exp_avg_sq"].cpu().numpy(), c["ref_v"], f"optim.Adam exp_avg_sq {k}")
        got = p.detach().cpu().numpy()
        ok = np.zeros(got.shape, bool)
        for cand in c["ref_p_any"]:
            ok |= S.bits(got) == S.bits(cand)
        assert ok.all(), f"optim.Adam parameter {k}: {int((~ok).sum())} elements match no fused / unfused sequence, first at {int(np.argmax(~ok))}"


@pytest.mark.parametrize("which", ["p", "grad"])
def test_optim_adam_refuses_an_unaligned_tensor(which):
    """a parameter (or gradient) that is a view one element into its allocation: CsbsrHipError naming it, the parameter unchanged, no
    state created, no step counted -- the kernel's float4 accesses are never launched on it"""
    from csbsr_amd import _lib as L
    from csbsr_amd.optim import Adam
    base = torch.arange(9, dtype=torch.float32, device="cuda")
    good = torch.nn.Parameter(torch.ones(8, device="cuda"))
    p = torch.nn.Parameter(base[1:] if which == "p" else torch.arange(1, 9, dtype=torch.float32, device="cuda"))
    assert (p.data_ptr() % 16 != 0) == (which == "p") and p.is_contiguous()
    opt = Adam([good, p], lr=0.125)
    good.grad = torch.ones(8, device="cuda")
    p.grad = torch.ones(9, device="cuda")[1:] if which == "grad" else torch.ones(8, device="cuda")
    with pytest.raises(L.CsbsrHipError, match=f"{which} of parameter 1 .*16-byte aligned"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach().cpu(), torch.arange(1, 9, dtype=torch.float32)) and torch.equal(good.detach().cpu(), torch.ones(8))
    assert "step" not in opt.state.get(p, {}) and "step" not in opt.state.get(good, {})
    p.grad = None          # the aligned parameter alone steps
    opt.step()
    assert float(opt.state[good]["step"]) == 1.0 and "step" not in opt.state.get(p, {})


# ------------------------------------------------------------------------------------------- head1_fwd

def _head1_rows(c, wrap, **kw):
    return [r for r in S.rows() if r["entry"] == "csbsr_head1_fwd" and "refused" not in r and r["c"] == c and r["wrap"] == wrap
            and all(r[k] == v for k, v in kw.items())]


def _run_head1_group(rows):
    """rows that share (c, npix, split, layout): one upload of the map, every (bias, sigmoid) of the group called twice"""
    r0 = rows[0]
    c, npix = r0["c"], r0["npix"]
    d = S.head1_case(c, npix, r0["split"])
    ld, c0 = S.layout(r0["layout"], c)
    x = In16Split(d["hi"], d["lo"], ld, c0) if r0["split"] else In16(d["hi"], ld, c0)
    w, bias = inp(d["w"]), inp(np.array([S.HEAD1_BIAS]))
    worst = 0.0
    for row in rows:
        def once():
            out = Out(npix)
            call("csbsr_head1_fwd", x.ptr, ld, x.lo if row["split"] else 0, c, _ptr(w), _ptr(bias) if row["bias"] else None, row["sigmoid"], out.ptr, npix)
            assert out.margins_intact(), "csbsr_head1_fwd wrote outside out"
            return dict(out=out.get())
        got = twice(once)
        worst = max(worst, S.head1_compare(row, got["out"], f"head1_fwd c={c} npix={npix} split={row['split']} {row['layout']} bias={row['bias']} sigmoid={row['sigmoid']}"))
    return worst


@pytest.mark.parametrize("lay", S.LAYOUTS)
@pytest.mark.parametrize("split", [0, 1], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("c", S.HEAD1_C)
def test_head1_fwd(c, split, lay):
    worst, n = 0.0, 0
    for npix in S.head1_npix(c):
        rows = _head1_rows(c, False, split=split, layout=lay, npix=npix)
        assert len(rows) == 4          # bias absent / given x sigmoid off / on
        worst = max(worst, _run_head1_group(rows))
        n += len(rows)
    assert n == 16
    _measured(f"head1_fwd sigmoid c={c} split={split} {lay}", worst)


@pytest.mark.parametrize("c", S.HEAD1_C)
def test_head1_fwd_grid_stride_wrap(c):
    """8192 ppb + ppb + 1 pixels: the workgroups of the capped grid take a second pixel block, one of them a third"""
    rows = _head1_rows(c, True)
    assert [r["sigmoid"] for r in rows] == [0, 1] and rows[0]["npix"] == S.head1_wrap_npix(c)
    _measured(f"head1_fwd sigmoid wrap c={c}", _run_head1_group(rows))
    S.head1_case.cache_clear()
    torch.cuda.empty_cache()


def test_head1_refusals():
    from csbsr_amd import _lib as L
    refused = [r for r in S.rows() if r["entry"] in ("csbsr_head1_fwd", "csbsr_head1_bwd_input") and "refused" in r]
    assert [(r["entry"][6:], r["refused"], r["c"]) for r in refused] == [("head1_fwd", "c", 32), ("head1_fwd", "ld", 64), ("head1_bwd_input", "c", 12)]
    x, w, out = In16(np.ones((4, 64)), 64, 0), inp(np.ones(64)), Out(4)
    for r in refused[:2]:
        with pytest.raises(L.CsbsrHipError, match=r"\(1\): .*head1_fwd: bad arguments"):
            call("csbsr_head1_fwd", x.ptr, r["ld"], 0, r["c"], _ptr(w), None, 0, out.ptr, 4)
    d, dx = In16(np.ones((4, 1)), 8, 0), Out16(4, 16)
    with pytest.raises(L.CsbsrHipError, match=r"\(1\): .*head1_bwd_input: bad arguments"):
        call("csbsr_head1_bwd_input", d.ptr, 8, _ptr(w), refused[2]["c"], dx.ptr, 16, 4)
    torch.cuda.synchronize()
    assert out.untouched() and dx.intact() and (dx.get() == SENT).all()


# ------------------------------------------------------------------------------------------- head1_bwd_input

def _run_head1_bwd(row):
    c, npix = row["c"], row["npix"]
    d = S.head1b_case(c, npix, row["weights"])
    ld, c0 = S.layout(row["layout"], c)
    dpre, w = In16(d["d"].reshape(npix, 1), row["dpre_ld"], 0), inp(d["w"])

    def once():
        dx = Out16(npix, c, ld, c0)
        call("csbsr_head1_bwd_input", dpre.ptr, row["dpre_ld"], _ptr(w), c, dx.ptr, ld, npix)
        assert dx.intact(), "csbsr_head1_bwd_input wrote outside dx"
        return dict(dx=dx.get())
    got = twice(once)
    S.head1b_compare(row, got["dx"], f"head1_bwd_input c={c} npix={npix} dpre_ld={row['dpre_ld']} {row['layout']} {row['weights']}")


@pytest.mark.parametrize("weights", ["lattice", "random"])
@pytest.mark.parametrize("c", S.HEAD1B_C)
def test_head1_bwd_input(c, weights):
    rows = [r for r in S.rows() if r["entry"] == "csbsr_head1_bwd_input" and "refused" not in r and r["c"] == c and r["weights"] == weights and not r["wrap"]]
    assert len(rows) == 8          # dpre_ld 8 / 16 x whole / slice x 1 / 33 pixels
    for row in rows:
        _run_head1_bwd(row)


@pytest.mark.parametrize("weights", ["lattice", "random"])
def test_head1_bwd_input_grid_stride_wrap(weights):
    (row,) = [r for r in S.rows() if r["entry"] == "csbsr_head1_bwd_input" and r.get("wrap") and r["weights"] == weights]
    _run_head1_bwd(row)
    S.head1b_case.cache_clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- sigmoid_bwd_to_nhwc8

@pytest.mark.parametrize("scale", S.SIGB_SCALES)
@pytest.mark.parametrize("npix", [1, 255, 257, S.sigb_wrap_npix()])
def test_sigmoid_bwd_to_nhwc8(npix, scale):
    (row,) = [r for r in S.rows() if r["entry"] == "csbsr_sigmoid_bwd_to_nhwc8" and r["npix"] == npix and r["scale"] == scale]
    d = S.sigb_case(npix, scale)
    dp, p = inp(d["dp"]), inp(d["p"])

    def once():
        out = Out(npix * 8, dtype=torch.float16)
        call("csbsr_sigmoid_bwd_to_nhwc8", _ptr(dp), _ptr(p), out.ptr, npix, C.c_float(scale))
        assert out.margins_intact(), "csbsr_sigmoid_bwd_to_nhwc8 wrote outside out"
        return dict(out=out.get(npix, 8))
    got = twice(once)
    _measured(f"sigmoid_bwd_to_nhwc8 npix={npix} scale={scale:g}", S.sigb_compare(row, got["out"], f"sigmoid_bwd_to_nhwc8 npix={npix} scale={scale:g}"))
    if row["wrap"]:
        S.sigb_case.cache_clear()
        torch.cuda.empty_cache()
