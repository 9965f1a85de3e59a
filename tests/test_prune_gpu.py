"""csrc/prune.hip and its drivers on the device: every result is an integer and is asked for exactly, against the NumPy restatement of
tests/prune_cases.py (whose own properties tests/test_prune_cpu.py holds).

Through the C ABI the skeleton sits inside an allocation filled with 1 -- a set pixel, so a read outside a plane would add a neighbour --,
and every output and the scratch inside a sentinel-filled allocation whose margins are checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import components_cases as CC
import prune_cases as PR
import skeleton_cases as SC
import topology_cases as TC
import width_cases as WC
from test_topology_gpu import _check_topology_keys, _files, _same
from test_width_gpu import _check_width_keys

pytestmark = pytest.mark.gpu

PAD = 64
ISENT = 0x5A5A5A5A
BSENT = 0x5A
DEV = torch.device("cuda", 0)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _out(n, dtype=torch.uint8):
    sent = ISENT if dtype == torch.int32 else BSENT
    buf = torch.full((n + 2 * PAD,), sent, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _margins_intact(*wholes):
    for w in wholes:
        sent = ISENT if w.dtype == torch.int32 else BSENT
        assert bool((w[:PAD] == sent).all()) and bool((w[-PAD:] == sent).all()), "a write outside an output"


def _lib():
    from csbsr_amd import _lib as L
    return L, L.load()


def steps_and_tile():
    _, lib = _lib()
    kp, kg, th, tw = (C.c_int32() for _ in range(4))
    assert lib.csbsr_prune_steps(C.byref(kp), C.byref(kg)) == 0 and lib.csbsr_prune_tile(C.byref(th), C.byref(tw)) == 0
    return kp.value, kg.value, th.value, tw.value


def device_prune(planes, spur_px):
    """(out uint8 [N, H, W], time uint8 [N, H, W], removed int32 [N]) of csbsr_skeleton_prune through the C ABI"""
    L, lib = _lib()
    planes = np.ascontiguousarray(planes, np.uint8)
    N, H, W = planes.shape
    pad = 2 * (W + 2)                                                                # set pixels before the first and behind the last plane
    buf = torch.full((planes.size + 2 * pad,), 1, dtype=torch.uint8, device=DEV)
    sk = buf[pad:pad + planes.size]
    sk.copy_(torch.from_numpy(planes.reshape(-1)))
    need = int(lib.csbsr_prune_work_bytes(N, H, W))
    assert need == 4 * N * H * ((W + 31) // 32) * 4
    (ww, work), (wo, out), (wt, time), (wr, removed) = _out(need), _out(N * H * W), _out(N * H * W), _out(N, torch.int32)
    L.call("csbsr_skeleton_prune", _ptr(sk), N, H, W, spur_px, _ptr(work), _ptr(time), _ptr(out), _ptr(removed), _stream())
    torch.cuda.synchronize()
    _margins_intact(ww, wo, wt, wr)
    assert np.array_equal(sk.cpu().numpy().reshape(planes.shape), planes), "the input was written"
    return out.cpu().numpy().reshape(N, H, W), time.cpu().numpy().reshape(N, H, W), removed.cpu().numpy()


def _equals_the_restatement(planes, L, want=None):
    out, time, removed = device_prune(planes, L)
    w_out, w_time, w_removed = PR.prune_of(planes, L) if want is None else want
    assert out.dtype == np.uint8 and np.array_equal(out, w_out), (L, np.argwhere(out != w_out)[:5])
    assert time.dtype == np.uint8 and np.array_equal(time, w_time), (L, np.argwhere(time != w_time)[:5])
    assert removed.dtype == np.int32 and np.array_equal(removed, w_removed), (L, removed, w_removed)
    return removed


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_constants_are_those_of_the_cases():
    _, lib = _lib()
    assert steps_and_tile() == (PR.KP, PR.KG, PR.TH, PR.TW) and lib.csbsr_prune_max_spur() == PR.MAX_SPUR == 64
    kp, kg = PR.KP, PR.KG
    assert set(PR.spur_lengths()) >= {1, 2, kp - 1, kp, kp + 1, 2 * kp + 1, kg + 1, 33, 64}


@pytest.mark.parametrize("name", list(PR.cases()))
def test_out_time_and_removed_equal_the_restatement(name):
    planes = PR.cases()[name]
    for L in PR.spur_lengths():
        _equals_the_restatement(planes, L, PR.expected(name, L))


@pytest.mark.parametrize("L", PR.spur_lengths())
def test_spurs_across_a_seam(L):
    """base in one tile, tip in the next: the spurs of L - 1 and L pixels go, the one of L + 1 stays"""
    removed = _equals_the_restatement(PR.seam_spurs(L), L)
    assert removed.tolist() == [2 * max(L - 1, 1), 2 * L, 0]


@pytest.mark.parametrize("name", list(PR.HAND))
def test_hand_shapes_lose_their_hand_derived_pixels_on_the_device(name):
    for L, want in PR.HAND[name][1].items():
        assert device_prune(PR.hand(name)[None], L)[2].tolist() == [want], L


@pytest.mark.parametrize("seed", PR.CRACK_SEEDS)
def test_the_fixture_counts_on_the_device(seed):
    for L, want in PR.FIXTURE_REMOVED[seed].items():
        out, _, removed = device_prune(PR.crack_skeleton(seed)[None], L)
        assert removed.tolist() == [want]
        if seed == 0:
            assert int(PR.tips_of(out[0])[0].sum()) == PR.FIXTURE_TIPS_0[L]


def test_the_planes_of_a_batch_are_independent():
    planes = PR.cases()["thin_between_full"]
    for L in (3, 20):
        out, time, removed = device_prune(planes, L)
        alone = device_prune(planes[1:2], L)
        assert np.array_equal(out[1], alone[0][0]) and np.array_equal(time[1], alone[1][0]) and removed[1] == alone[2][0] == 6      # the T's spur and the fork's short arm


def test_a_plane_of_many_tiles():
    """520 x 700: 9 x 6 tiles -- noise at three densities side by side, an empty band, and the skeleton of the noise below it"""
    rng = np.random.default_rng(12)
    plane = np.zeros((520, 700), np.uint8)
    for k, d in enumerate((0.1, 0.5, 0.9)):
        plane[:256, 200 * k:200 * k + 150] = rng.random((256, 150)) < d
    plane[128:192] = 0
    plane[260:] = SC.skeleton(rng.random((260, 700)) < 0.55)
    for L in (9, 40):
        _equals_the_restatement(plane[None], L)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_prune_spurs_surface():
    from csbsr_amd.utils.estimate_metrics import prune_spurs
    planes = PR.cases()["cracks"]
    N, H, W = planes.shape
    L = 16
    w_out, w_time, w_removed = PR.expected("cracks", L)
    s = torch.from_numpy(planes).to(DEV)
    res = prune_spurs(s, L)
    assert len(res) == 2
    out, removed = res
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (N, H, W) and np.array_equal(out.cpu().numpy(), w_out)
    assert removed.is_cuda and removed.dtype == torch.int32 and tuple(removed.shape) == (N,) and np.array_equal(removed.cpu().numpy(), w_removed)
    out_t, removed_t, time = prune_spurs(s, L, return_time=True)
    assert torch.equal(out_t, out) and torch.equal(removed_t, removed)
    assert time.is_cuda and time.dtype == torch.uint8 and tuple(time.shape) == (N, H, W) and np.array_equal(time.cpu().numpy(), w_time)
    for a in (s[:, None], torch.from_numpy(planes), s * 255, s[0], np.int64(L)):     # [N, 1, H, W]; a CPU tensor; any byte; one plane; a NumPy L
        ob, rb = prune_spurs(s, a) if not torch.is_tensor(a) else prune_spurs(a, L)
        n = 1 if torch.is_tensor(a) and a.dim() == 2 else N
        assert ob.is_cuda and tuple(ob.shape) == (n, H, W) and torch.equal(ob, out[:n]) and torch.equal(rb, removed[:n])
    wide = s.repeat(1, 1, 2)[:, :, 1:W + 1]                                         # a view that is not contiguous
    assert np.array_equal(prune_spurs(wide, L)[0].cpu().numpy(), PR.prune_of(wide.cpu().numpy(), L)[0])
    assert torch.equal(prune_spurs(out, L)[0], out) and int(prune_spurs(out, L)[1].sum()) == 0      # pruning again changes nothing
    for bad in (s.to(torch.int32), s.to(torch.float32), planes, s[0, 0]):
        with pytest.raises(ValueError):
            prune_spurs(bad, L)
    for bad in (0, 65, -1, True, 4.0, "4", None):
        with pytest.raises(ValueError):
            prune_spurs(s, bad)


def test_two_calls_return_equal_tensors():
    from csbsr_amd.utils.estimate_metrics import prune_spurs
    for name in ("noise_0.6", "cracks", "long_spur", "noise_130x260"):
        s = torch.from_numpy(PR.cases()[name]).to(DEV)
        for L in (9, 64):
            a, b = prune_spurs(s, L, return_time=True), prune_spurs(s, L, return_time=True)
            assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused():
    L, lib = _lib()
    sk = torch.ones(64, dtype=torch.uint8, device=DEV)
    out, time, work = (torch.full((n,), BSENT, dtype=torch.uint8, device=DEV) for n in (64, 64, 4096))
    removed = torch.full((4,), ISENT, dtype=torch.int32, device=DEV)
    st = _stream()
    good = dict(N=1, H=8, W=8, L=4)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(H=-8), dict(W=-8), dict(H=8193), dict(W=8193), dict(N=65536), dict(L=0), dict(L=-1),
                dict(L=65)):
        d = {**good, **bad}
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_skeleton_prune", _ptr(sk), d["N"], d["H"], d["W"], d["L"], _ptr(work), _ptr(time), _ptr(out), _ptr(removed), st)
        if "L" not in bad:
            assert lib.csbsr_prune_work_bytes(d["N"], d["H"], d["W"]) == 0
    for args in ((None, _ptr(work), _ptr(time), _ptr(out), _ptr(removed)), (_ptr(sk), None, _ptr(time), _ptr(out), _ptr(removed)),
                 (_ptr(sk), _ptr(work), None, _ptr(out), _ptr(removed)), (_ptr(sk), _ptr(work), _ptr(time), None, _ptr(removed)),
                 (_ptr(sk), _ptr(work), _ptr(time), _ptr(out), None),
                 (_ptr(out), _ptr(work), _ptr(time), _ptr(out), _ptr(removed)),      # in place
                 (_ptr(time), _ptr(work), _ptr(time), _ptr(out), _ptr(removed)), (_ptr(sk), _ptr(work), _ptr(out), _ptr(out), _ptr(removed))):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_skeleton_prune", args[0], 1, 8, 8, 4, *args[1:], st)
    with pytest.raises(L.CsbsrHipError):
        L.call("csbsr_prune_steps", None, None)
    with pytest.raises(L.CsbsrHipError):
        L.call("csbsr_prune_tile", None, None)
    torch.cuda.synchronize()
    for t in (out, time, work):                                                      # nothing ran: no output was written, no count cleared
        assert bool((t == BSENT).all())
    assert bool((removed == ISENT).all())


# ------------------------------------------------------------------------------------------------ the driver
def test_predict_dataset_with_prune_spur_px(tmp_path):
    """test_predict_dataset_with_min_crack_px's two images (stitched maps of 64 x 96 and 84 x 68), with the skeleton pruned"""
    import eval_io_cases as EC
    import predict_cases as PC
    from PIL import Image
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd import inference as I
    predict_dataset = I.predict_dataset
    images = PC.make_images(PC.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t, k, r, L = 0.4, 5, 64, 6
    measure_keys = {"name", "sr_u8", "map_u8", "map_f32", "kernels", "crack_px", "skeleton_px", "mean_width_px"}
    crack_keys = measure_keys | {"removed_px", "n_cracks", "labels", "cracks"}
    topo_keys = {"endpoints", "junctions", "junction_px", "isolated_px", "loops", "links", "length_geodesic_px", "orientation", "mean_width_geodesic_px",
                 "topology_map"}
    width_keys = {"max_width_px", "median_width_px", "p95_width_px", "centerline_width_px", "saturated_px", "widest", "width_hist", "width_d2"}
    total = 0
    for batch_patches in (16, 4):                                                   # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        want = PC.host_chain(ld, images, EC.stub_model, torch.from_numpy, EC.thresholds32()[EC.SAVE_IDX])
        save, save_w = tmp_path / f"{batch_patches}", tmp_path / f"{batch_patches}_w"
        got = list(predict_dataset(EC.stub_model, ld, save_dir=str(save), measure_threshold=t, min_crack_px=k, width_radius=r, topology=True,
                                   prune_spur_px=L))
        whole = list(predict_dataset(EC.stub_model, ld, save_dir=str(save_w), measure_threshold=t, width_radius=r, topology=True, prune_spur_px=L))
        bare = list(predict_dataset(EC.stub_model, ld, measure_threshold=t, prune_spur_px=L))
        cracks_only = list(predict_dataset(EC.stub_model, ld, measure_threshold=t, min_crack_px=k))
        measured = list(predict_dataset(EC.stub_model, ld, measure_threshold=t))
        spurs, inst = [], []
        for g, a, b, c, m, w in zip(got, whole, bare, cracks_only, measured, want):
            assert set(m) == measure_keys and set(c) == crack_keys                  # without the option: today's keys
            assert set(b) == measure_keys | {"spur_px"} and set(a) == measure_keys | topo_keys | width_keys | {"spur_px"}
            assert set(g) == crack_keys | topo_keys | width_keys | {"spur_px"}
            H, W = w["map_f32"].shape
            region = SC.binarise(w["map_f32"], t)
            lab = CC.canonical_labels(region, 8)[None]
            kept = CC.keep(lab, k)[0].astype(bool)
            skel_all = SC.skeleton(region)
            pruned_all = PR.prune(skel_all, L)[0].astype(bool)
            pruned = pruned_all & kept
            assert np.array_equal(pruned, PR.prune(skel_all & kept, L)[0].astype(bool))         # one pruning serves all components
            # the whole skeleton
            for x in (a, b):
                assert type(x["spur_px"]) is int and x["spur_px"] == int(skel_all.sum() - pruned_all.sum())
                assert (x["crack_px"], x["skeleton_px"] + x["spur_px"]) == (m["crack_px"], m["skeleton_px"]) and x["skeleton_px"] == pruned_all.sum()
                assert x["mean_width_px"] == (x["crack_px"] / x["skeleton_px"] if x["skeleton_px"] else 0.0)
            _check_topology_keys(a, pruned_all, int(region.sum()))
            _check_width_keys(a, np.where(pruned_all, WC.d2_of(region, r), 0).astype(np.int32), pruned_all, r)
            # the kept cracks
            assert type(g["spur_px"]) is int and g["spur_px"] == int((skel_all & kept).sum() - pruned.sum())
            assert (g["crack_px"], g["skeleton_px"] + g["spur_px"]) == (c["crack_px"], c["skeleton_px"]) and g["skeleton_px"] == pruned.sum() > 0
            _check_topology_keys(g, pruned, int(kept.sum()))
            d2 = np.where(pruned, WC.d2_of(region, r), 0).astype(np.int32)
            _check_width_keys(g, d2, pruned, r)
            trows, wrows = TC.topology_rows(lab, TC.topo_of(pruned)[None], k), WC.width_rows(lab, d2[None], k)
            assert len(trows) == len(wrows) == len(g["cracks"]) == len(c["cracks"]) >= 2
            for crack, plain, trow, (_, label, m2, y, x) in zip(g["cracks"], c["cracks"], trows.tolist(), wrows.tolist()):
                mine = lab[0] == label
                assert crack["y"] * W + crack["x"] + 1 == label == trow[1] and crack["area_px"] == plain["area_px"] and crack["bbox"] == plain["bbox"]
                assert type(crack["spur_px"]) is int and crack["spur_px"] == int((skel_all & mine).sum() - (pruned & mine).sum())
                assert crack["length_px"] == int((pruned & mine).sum()) == plain["length_px"] - crack["spur_px"]
                assert crack["mean_width_px"] == (crack["area_px"] / crack["length_px"] if crack["length_px"] else 0.0)
                assert {q: crack[q] for q in ("endpoints", "junctions", "loops", "links", "length_geodesic_px", "orientation")} == TC.crack_of(trow[2:], crack["length_px"])
                assert (crack["max_width_px"], crack["widest"]) == (WC.width(m2), (y, x) if m2 > 0 else None)
            assert sum(crack["spur_px"] for crack in g["cracks"]) == g["spur_px"]
            assert sum(crack["length_px"] for crack in g["cracks"]) == g["skeleton_px"]
            # nothing else changes with the option
            for key in ("map_f32", "sr_u8", "map_u8", "kernels"):
                assert torch.equal(g[key], m[key]) and torch.equal(a[key], m[key]) and torch.equal(b[key], m[key]), key
            assert torch.equal(g["labels"], c["labels"]) and (g["removed_px"], g["n_cracks"]) == (c["removed_px"], c["n_cracks"])
            for root, plane in ((save, pruned), (save_w, pruned_all)):
                assert np.array_equal(np.asarray(Image.open(root / "skeletons" / g["name"])), plane.astype(np.uint8) * 255)
            spurs.append((g["name"], g["skeleton_px"], g["spur_px"]))
            inst.append((g["name"], [dict(length_px=crack["length_px"], spur_px=crack["spur_px"]) for crack in g["cracks"]]))
            total += a["spur_px"]
        assert sorted(os.listdir(save)) == ["crack_instance_spurs.csv", "crack_instance_topology.csv", "crack_instance_widths.csv", "crack_instances.csv",
                                            "crack_spurs.csv", "crack_stats.csv", "crack_topology.csv", "crack_widths.csv", "images", "kernels",
                                            "kernels_origin", "masks", "skeletons"]
        assert sorted(os.listdir(save_w)) == ["crack_spurs.csv", "crack_stats.csv", "crack_topology.csv", "crack_widths.csv", "images", "kernels",
                                              "kernels_origin", "masks", "skeletons"]
        assert SC.read_csv(str(save / "crack_spurs.csv"))[0] == I.SPUR_COLUMNS and I.read_crack_spurs(str(save / "crack_spurs.csv")) == spurs
        assert SC.read_csv(str(save / "crack_instance_spurs.csv"))[0] == I.INSTANCE_SPUR_COLUMNS
        assert I.read_crack_instance_spurs(str(save / "crack_instance_spurs.csv")) == inst
        assert I.read_crack_spurs(str(save_w / "crack_spurs.csv")) == [(a["name"], a["skeleton_px"], a["spur_px"]) for a in whole]
        assert SC.read_csv(str(save / "crack_stats.csv"))[0] == ["name", "crack_px", "skeleton_px", "mean_width_px"]
        assert [(n, int(sk)) for n, _, sk, _ in SC.read_csv(str(save / "crack_stats.csv"))[1:]] == [(n, sk) for n, sk, _ in spurs]
        assert SC.read_csv(str(save / "crack_instances.csv"))[0] == I.INSTANCE_COLUMNS
        assert [[cr["length_px"] for cr in crs] for _, crs in I.read_crack_instances(str(save / "crack_instances.csv"))] == [[cr["length_px"] for cr in crs] for _, crs in inst]
    assert total > 0, "the maps have spurs of up to L pixels"
    # prune_spur_px=None is the call without the argument: the same keys, values and files
    for kwargs in (dict(), dict(measure_threshold=t), dict(measure_threshold=t, min_crack_px=k),
                   dict(measure_threshold=t, min_crack_px=k, width_radius=5, topology=True)):
        tag = "_".join(sorted(kwargs)) or "plain"
        off = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_off"), prune_spur_px=None, **kwargs))
        none = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_none"), **kwargs))
        assert len(off) == len(none) == 2
        for x, y in zip(off, none):
            cx, cy = x.pop("cracks", None), y.pop("cracks", None)
            hx, hy = x.pop("width_hist", None), y.pop("width_hist", None)
            _same(x, y)
            assert cx == cy and (hx is None) == (hy is None) and (hx is None or np.array_equal(hx, hy))
            assert "spur_px" not in x and not any("spur_px" in crack for crack in cx or [])
        fa, fb = _files(tmp_path / f"{tag}_off"), _files(tmp_path / f"{tag}_none")
        assert fa == fb and not any("spur" in n for n in fa)
    # an all-zero map
    zero = lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs))
    for kwargs in (dict(), dict(min_crack_px=k)):
        g = next(predict_dataset(zero, ld, measure_threshold=t, prune_spur_px=L, **kwargs))
        assert (g["skeleton_px"], g["spur_px"], g["mean_width_px"]) == (0, 0, 0.0)
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(prune_spur_px=4), dict(min_crack_px=k, prune_spur_px=4), dict(measure_threshold=t, prune_spur_px=0), dict(measure_threshold=t, prune_spur_px=65),
                   dict(measure_threshold=t, prune_spur_px=True), dict(measure_threshold=t, prune_spur_px=4.0), dict(measure_threshold=t, prune_spur_px="4")):
        with pytest.raises(ValueError):
            next(predict_dataset(model, ld, **kwargs))
