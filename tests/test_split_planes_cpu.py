"""The host side of the split-fp16 kernel tests (tests/split_cases.py), checked without a GPU: the format bound every GPU assertion builds
on, that the bounds of the case table are conditions a hi-only kernel cannot meet, and that the shapes meant for one of two dispatched
kernels select it."""
import pytest
import torch

import split_cases as S


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e2, 3e4])
def test_split_format_bound(scale):
    """|split_load64(split_store(v)) - v| <= |v| 2^-22 + 2^-25 for |v| < 6e4, and the fp32 split_load of a stored pair is exact"""
    v = torch.randn(1 << 20, generator=torch.Generator().manual_seed(5)) * scale
    v = v[v.abs() < 6e4]
    hi, lo = S.split_store(v)
    v64 = S.split_load64(hi, lo)
    ratio = ((v64 - v.double()).abs() / S.fmt_bound(v.double())).max()
    print(f"scale {scale:g}: worst |error| / bound = {float(ratio):.4f}")
    assert ratio <= 1.0
    assert torch.equal(S.split_load(hi, lo).double(), v64)


def test_canary_helpers_on_host():
    """to_split_fm / from_split_fm / the canary check, on a CPU 'device': both layouts round-trip and a stray write is counted"""
    class Host:
        device = torch.device("cpu")
    x = S.split_pair(S.draw((2, 24, 3, 5), 1))
    for kw in ({}, {"c_total": 24 + S.SLICE_EXTRA, "c0": S.SLICE_C0}):
        fm = S.to_split_fm(Host, x, **kw)
        assert fm.lo == (48 if kw else 24) and fm.ld == 2 * fm.lo and fm.flat_ok()
        assert torch.equal(S.from_split_fm(fm), S.split_load64(*x))
        assert S.canary_damage(fm) == 0
        out = S.empty_split_fm(Host, 2, 3, 5, 20, **kw)
        assert out.cp == 24 and S.canary_damage(out) == 0
        if kw:
            base, c0 = S._base(out)
            assert c0 == S.SLICE_C0
            base[1, 2, 3, c0 + out.lo + out.cp] = 0.0          # first lo-plane element past the slice
            base[0, 0, 0, c0 - 1] = 1.0
            assert S.canary_damage(out) == 2
    plain = S.to_split_fm(Host, S.plain_pair(S.draw((1, 8, 2, 2), 2)), c_total=32, c0=8)
    assert plain.lo == 0 and plain.ld == 32 and S.canary_damage(plain) == 0


def test_case_table_is_complete():
    ops = {c.op for c in S.CASES}
    assert ops == {"convert", "maxpool", "maxpool_bwd", "axpby", "sum_act", "bn", "aap", "bilinear", "wpool"}
    assert len({c.id for c in S.CASES}) == len(S.CASES)


@pytest.mark.parametrize("case", [c for c in S.CASES if c.kind == "exact"], ids=lambda c: c.id)
def test_exact_emulations_meet_the_format_bound(case):
    """the bit-exact rows: what the emulation stores is within the format bound (+ its own E_op) of the fp64 reference"""
    h = S.host(case)
    err = (S.stored64(case, h.out32) - h.ref64).abs()
    if case.out == "split":
        assert (err <= h.bound).all()
    if case.op in ("maxpool", "maxpool_bwd"):
        assert h.e_op == 0.0            # max and the gridded gradient sums are exact in fp32


@pytest.mark.parametrize("case", [c for c in S.CASES if c.mutants], ids=lambda c: c.id)
def test_mutants_miss_the_bound(case):
    """a kernel that ignores lo on load, does not write lo, or takes the max-pool winner from hi alone misses the row's bound (the 4x margin
    on E_op included) by at least 16x on at least 10 % of the elements"""
    h = S.host(case)
    assert float((S.stored64(case, h.out32) - h.ref64).abs().max()) <= float((h.bound).max())
    for m in case.mutants:
        err = (S.mutant64(case, m) - h.ref64).abs()
        frac = float((err > 16 * h.bound).double().mean())
        print(f"{case.id} [{m}]: E_op {h.e_op:.3g}, {100 * frac:.1f} % of the elements beyond 16x the bound, median error / bound "
              f"{float((err / h.bound).median()):.1f}")
        assert frac >= 0.10, (case.id, m, frac)


# The two dispatching launchers, restated.  csrc/elementwise.hip, csbsr_adaptive_avgpool_fwd_split:
#     if ((long)(H / OH) * (W / OW) >= 64)  -> aap_fwd_block_kernel, else aap_fwd_kernel
def aap_takes_block(H, W, OH, OW):
    return (H // OH) * (W // OW) >= 64


# csrc/elementwise.hip, csbsr_bilinear_fwd_split (BIL_RS = 16; the strips <= 65535 clause holds for every shape here):
#     if (cols && OH >= BIL_RS && strips <= 65535 && (per_row + 255) / 256 * strips >= 64)  -> bilinear_fwd_cols_kernel, else bilinear_fwd_kernel
# with per_row = OW * (c / 8) and strips = N * ((OH + 15) / 16)
def bilinear_takes_cols(N, c, OH, OW):
    strips = N * ((OH + 15) // 16)
    return OH >= 16 and strips <= 65535 and (OW * (c // 8) + 255) // 256 * strips >= 64


def test_kernel_selection():
    aap = [c for c in S.CASES if c.op == "aap"]
    bil = [c for c in S.CASES if c.op == "bilinear"]
    for c in aap:
        assert aap_takes_block(*c.p["shape"][2:], *c.p["osize"]) == c.p["block"], c.id
    for c in bil:
        assert bilinear_takes_cols(c.p["shape"][0], c.p["shape"][1], *c.p["osize"]) == c.p["cols"], c.id
    block = {c.id for c in aap if c.p["block"]}
    assert {f"aap-{s}-c{c}" for s in ("20x20-2", "17x19-2", "24x24-3", "16x16-1") for c in (24, 136)} <= block
    assert {c.id for c in aap if not c.p["block"]} == {"aap-8x8-2-c24", "aap-8x8-3-c24", "aap-8x8-6-c24", "aap-11x14-3x5-c24"}
    assert {c.id.rsplit("-align", 1)[0] for c in bil if c.p["cols"]} == {"bilinear-23x31-50x70-drop", "bilinear-32x32-64x64"}
    assert {c.id.rsplit("-align", 1)[0] for c in bil if not c.p["cols"]} == {"bilinear-8x8-16x16", "bilinear-5x7-20x21-drop", "bilinear-6x6-1x1"}
    # the block kernel's passes: 100 pixels = 3 full passes of the 32 pixel lanes and a ragged one; 17x19 -> 2 has overlapping 9 x 10 bins
    assert S.aap_bins(20, 2) == [(0, 10), (10, 20)] and S.aap_bins(17, 2) == [(0, 9), (8, 17)] and S.aap_bins(19, 2) == [(0, 10), (9, 19)]
    # the composed chain's pooled map goes through the block kernel too
    N, C, H, W = S.CHAIN_SHAPE
    assert aap_takes_block((H - 1) // 2 + 1, (W - 1) // 2 + 1, 2, 2)


def test_chain_bound_excludes_a_hi_only_chain():
    """the composed chain: the emulation meets the propagated bound, the same chain with every lo plane forced to 0 misses it"""
    ins, r, em, e_op, e = S.chain_host()
    for name in e:
        err = float((em[name].double() - r[name]).abs().max())
        print(f"{name}: E_op {e_op[name]:.3g}, emulated chain error {err:.3g}, bound {e[name]:.3g}")
        assert err <= e[name], name
    hi_only = S.chain_host(hi_only=True)[2]
    err = float((hi_only["axpby"].double() - r["axpby"]).abs().max())
    print(f"hi-only chain error {err:.3g}, bound {e['axpby']:.3g}")
    assert err > 16 * e["axpby"]
