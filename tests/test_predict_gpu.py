"""Prediction of unlabeled images on the device (csrc/eval_io.hip: csbsr_stitch_tiles_u8, csbsr_amd/data/resident_predict.py,
csbsr_amd/inference.py: predict_dataset): the ragged stitch against its NumPy restatement bit for bit inside guard bands, the border
replication of csbsr_gather_crop_u8 the loader relies on, and predict_dataset against a host chain built from the loader's own tables, against
evaluate_dataset where both apply, and with the real model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import eval_io_cases as EC
import predict_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1 << 16        # more than any row of the hostile table below could overrun by: a broken clamp would still write into this buffer


def guarded(n, dtype):
    """(view, whole): ``n`` elements inside a larger 0xA5-filled byte buffer, GUARD bytes on either side."""
    nb = n * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((GUARD + nb + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return whole[GUARD:GUARD + nb].view(dtype), whole


def guards_intact(whole):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[-GUARD:] == 0xA5).all())


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stitch(p, Cc, PH, PW, tiles, dims, clip, f32, u8):
    from csbsr_amd import _lib as L
    off = torch.from_numpy(PC.pool_offsets(dims, Cc)).to(DEV)
    d = torch.tensor(dims, dtype=torch.int32, device=DEV)
    t = torch.tensor(tiles, dtype=torch.int32, device=DEV)
    L.call("csbsr_stitch_tiles_u8", _ptr(p), len(tiles), Cc, PH, PW, _ptr(t), _ptr(off), _ptr(d), clip, _ptr(f32), _ptr(u8),
           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", sorted(PC.KERNEL_CASES))
def test_stitch_tiles_equals_the_numpy_restatement(case):
    """(a) aligned, (b) misaligned C = 3 and C = 1, (c) values < 0, > 1, NaN, -0.0 with clip on and off, (d) fp32 only, uint8 only, both,
    (e) unowned pixels keep the sentinel -- every pool byte and both guard bands compared."""
    Cc, PH, PW, dims, tiles = PC.KERNEL_CASES[case]
    v = PC.tile_values((len(tiles), Cc, PH, PW), seed=len(case) + PH, special=True)
    assert np.isnan(v).any() and (v < 0).any() and (v > 1).any() and np.signbit(v[v == 0]).any()
    p = torch.from_numpy(v).to(DEV)
    total = sum(h * w for h, w in dims) * Cc
    for clip in (0, 1):
        want_f, want_u = PC.stitch_tiles_numpy(v, tiles, dims, clip)
        if case in ("unowned", "misaligned_c3", "misaligned_c1"):
            assert (want_f.view(np.uint32) == 0xA5A5A5A5).sum() >= total // 4            # (e): a good part of the pool has no owner
        for f_on, u_on in ((True, True), (True, False), (False, True)):
            f32, wf = guarded(total, torch.float32)
            u8, wu = guarded(total, torch.uint8)
            _stitch(p, Cc, PH, PW, tiles, dims, clip, f32 if f_on else None, u8 if u_on else None)
            assert guards_intact(wf) and guards_intact(wu)
            if f_on:
                assert np.array_equal(f32.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (case, clip)
            else:
                assert bool((wf == 0xA5).all())
            if u_on:
                assert np.array_equal(u8.cpu().numpy(), want_u), (case, clip)
            else:
                assert bool((wu == 0xA5).all())
    # clip off leaves the values; clip on leaves NaN and -0.0 what they are (the two masked assignments, not clamp)
    raw, _ = PC.stitch_tiles_numpy(v, tiles, dims, 0)
    clipped, _ = PC.stitch_tiles_numpy(v, tiles, dims, 1)
    assert np.isnan(clipped).sum() == np.isnan(raw).sum() and (raw > 1).any() and not (clipped > 1).any()


def test_stitch_tiles_rejects_bad_arguments_and_cuts_a_bad_table():
    from csbsr_amd import _lib as L
    Cc, PH, PW, dims, tiles = PC.KERNEL_CASES["aligned"]
    p = torch.from_numpy(PC.tile_values((len(tiles), Cc, PH, PW), seed=1)).to(DEV)
    total = sum(h * w for h, w in dims) * Cc
    f32, wf = guarded(total, torch.float32)
    u8, wu = guarded(total, torch.uint8)
    off = torch.from_numpy(PC.pool_offsets(dims, Cc)).to(DEV)
    d = torch.tensor(dims, dtype=torch.int32, device=DEV)
    t = torch.tensor(tiles, dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((_ptr(p), 0, Cc, PH, PW, _ptr(t), _ptr(off), _ptr(d), 1, _ptr(f32), _ptr(u8), st),           # N <= 0
                 (_ptr(p), 5, 2, PH, PW, _ptr(t), _ptr(off), _ptr(d), 1, _ptr(f32), _ptr(u8), st),            # C not 1 or 3
                 (_ptr(p), 5, Cc, PH, PW, _ptr(t), _ptr(off), _ptr(d), 1, None, None, st),                    # no output
                 (None, 5, Cc, PH, PW, _ptr(t), _ptr(off), _ptr(d), 1, _ptr(f32), _ptr(u8), st),
                 (_ptr(p), 5, Cc, PH, PW, None, _ptr(off), _ptr(d), 1, _ptr(f32), _ptr(u8), st)):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_stitch_tiles_u8", *args)
    # rows that ask for more than the patch holds or the image takes, all addressed to image 1 (16 x 24 of the 16 x 24 patches): whatever
    # they write stays inside image 1 -- image 0 and both guard bands keep the fill
    bad = [(1, 12, 20, 0, 0, 16, 24, 0), (1, -3, -5, 0, 0, 8, 8, 0), (1, 0, 0, 10, 20, 16, 24, 0), (1, 0, 0, -4, -4, 40, 40, 0),
           (1, 40, 40, 0, 0, 4, 4, 0)]
    _stitch(p, Cc, PH, PW, bad, dims, 1, f32, u8)
    n0 = dims[0][0] * dims[0][1] * Cc
    assert guards_intact(wf) and guards_intact(wu)
    assert bool((u8[:n0] == 0xA5).all()) and bool((f32[:n0].view(torch.int32) == 0xA5A5A5A5 - (1 << 32)).all())
    assert bool((u8[n0:] != 0xA5).any())


@pytest.mark.parametrize("case", range(len(PC.GATHER_CASES)))
def test_gather_replicates_the_border(case):
    """The loader is the first caller that relies on the per-pixel clamp of csbsr_gather_crop_u8: windows with a negative origin and windows
    past the far edge read the nearest pixel of the image (C = 3, window widths 12 -- the vector store -- and 10 -- the per-pixel one)."""
    from csbsr_amd.data.resident_test import _U8Pool
    (h, w), (wh, ww), origins = PC.GATHER_CASES[case]
    rng = np.random.default_rng(case)
    images = [rng.integers(0, 256, size=(3, 5, 3), dtype=np.uint8), rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8),
              rng.integers(0, 256, size=(4, 4, 3), dtype=np.uint8)]            # neighbours in the pool on either side
    pool = _U8Pool(images, 3, "image", DEV)
    sel = torch.tensor([(1, y0, x0, 0, 0) for y0, x0 in origins], dtype=torch.int32, device=DEV)
    got = pool.gather(sel, len(origins), wh, ww).cpu().numpy()
    want = np.stack([PC.gather_replicate_numpy(images[1], y0, x0, wh, ww) for y0, x0 in origins])
    assert got.dtype == want.dtype and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ predict_dataset
def _predict_loader(images, patch, halo, batch_patches, names=None):
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    names = names or [f"field_{i}.png" for i in range(len(images))]
    return DevicePredictLoader(ResidentImageSet(images, names, device=DEV), patch, 4, halo=halo, batch_patches=batch_patches)


def _same(got, want):
    assert [g["name"] for g in got] == [w["name"] for w in want]
    for g, w in zip(got, want):
        assert g["sr_u8"].dtype == torch.uint8 and g["map_u8"].dtype == torch.uint8 and g["map_f32"].dtype == torch.float32
        for k in ("sr_u8", "map_u8"):
            assert g[k].is_cuda and np.array_equal(g[k].cpu().numpy(), w[k]), (g["name"], k)
        assert np.array_equal(g["map_f32"].cpu().numpy().view(np.uint32), w["map_f32"].view(np.uint32)), g["name"]
        assert torch.equal(g["kernels"].cpu(), w["kernels"]), g["name"]


@pytest.mark.parametrize("halo,batch_patches", [(0, 16), (0, 4), (2, 16), (2, 4)])
def test_predict_dataset_with_the_stub(halo, batch_patches, tmp_path):
    """Three images 16 x 24, 21 x 17 and 5 x 9 LR, patch (8, 8), scale 4: with 16 patches per call images 0 and 1 share a unit, with 4 every
    image is a unit of its own and takes several calls.  Every returned buffer and every saved file equals the host chain."""
    from PIL import Image
    from csbsr_amd.inference import predict_dataset
    images = PC.make_images(PC.PREDICT_SIZES, seed=17)
    ld = _predict_loader(images, (8, 8), halo, batch_patches)
    assert [(u.i0, u.i1) for u in ld] == ([(0, 2), (2, 3)] if batch_patches == 16 else [(0, 1), (1, 2), (2, 3)])
    th = EC.thresholds32()[EC.SAVE_IDX]
    want = PC.host_chain(ld, images, EC.stub_model, torch.from_numpy, th)
    got = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path)))
    _same(got, want)
    _same(list(predict_dataset(EC.stub_model, ld)), want)                      # without saving: the same buffers
    assert [tuple(g["sr_u8"].shape) for g in got] == [(4 * h, 4 * w, 3) for h, w in PC.PREDICT_SIZES]
    assert [g["kernels"].shape[0] for g in got] == [6, 9, 2]
    assert want[0]["sr_u8"].min() == 0 and want[0]["sr_u8"].max() == 255
    th_dirs = [f"th_{EC.THRESHOLDS[i]:.2f}" for i in EC.SAVE_IDX]
    assert sorted(os.listdir(tmp_path)) == ["images", "kernels", "kernels_origin", "masks"]             # no iou_log.csv
    assert sorted(os.listdir(tmp_path / "masks")) == sorted(th_dirs + ["th_-1.00"])
    for w in want:
        name, stem = w["name"], w["name"].replace(".png", "")
        im = Image.open(tmp_path / "images" / name)
        assert im.mode == "RGB" and np.array_equal(np.array(im), w["sr_u8"])
        for j, t in enumerate(th_dirs):
            im = Image.open(tmp_path / "masks" / t / name)
            assert im.mode == "L" and np.array_equal(np.array(im), w["planes"][j]), (name, t)
        assert np.array_equal(np.array(Image.open(tmp_path / "masks" / "th_-1.00" / name)), w["map_u8"])
        for j, k in enumerate(w["kernels"]):
            assert np.array_equal(np.array(Image.open(tmp_path / "kernels" / f"{stem}_{j}.png")), (k / torch.max(k)).mul(255).byte().numpy()[0])
            assert np.array_equal(np.array(Image.open(tmp_path / "kernels_origin" / f"{stem}_{j}_origin.png")),
                                  (k / torch.sum(k)).mul(255).byte().numpy()[0])
    assert len(os.listdir(tmp_path / "images")) == 3 and len(os.listdir(tmp_path / "kernels")) == 17
    assert len(np.unique(want[1]["planes"])) == 2 and len({p.tobytes() for p in want[1]["planes"]}) >= 5


def test_predict_dataset_saves_what_evaluate_dataset_saves(tmp_path):
    """Halo 0, two images whose sizes are multiples of the patch (16 x 24 of the three above and a 24 x 16 one), one image per model call on
    both sides (batch size 1 there, 6 patches per call here): images/, masks/ and the kernel files are the same bytes."""
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet
    from csbsr_amd.inference import evaluate_dataset, predict_dataset
    lr = [PC.make_images(PC.PREDICT_SIZES, seed=17)[0], PC.make_images([(24, 16)], seed=18)[0]]
    rng = np.random.default_rng(0)
    hr = [rng.integers(0, 256, size=(4 * a.shape[0], 4 * a.shape[1], 3), dtype=np.uint8) for a in lr]
    masks = [(255 * (rng.random(a.shape[:2]) < 0.3)).astype(np.uint8) for a in hr]
    ts = ResidentTestSet(hr, masks, lr, EC.anisotropic_kernels(2), ["img_00.jpg", "img_01.jpg"], device=DEV)
    evaluate_dataset(EC.stub_model, DeviceTestLoader(ts, 32, 4, 1), save_dir=str(tmp_path / "eval"))
    ld = _predict_loader(lr, (8, 8), 0, 6, names=["img_00.png", "img_01.png"])
    assert [ld.chunks(u) for u in ld] == [[(0, 6)], [(6, 12)]]
    for _ in predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / "pred")):
        pass
    n = 0
    for root, _, files in os.walk(tmp_path / "eval"):
        for f in files:
            if f == "iou_log.csv":
                continue
            rel = os.path.relpath(os.path.join(root, f), tmp_path / "eval")
            assert open(os.path.join(root, f), "rb").read() == open(tmp_path / "pred" / rel, "rb").read(), rel
            n += 1
    assert n == 2 * (1 + 12) + 2 * 12 and sum(len(f) for _, _, f in os.walk(tmp_path / "pred")) == n


def test_predict_dataset_with_the_real_model():
    """Core LR 16, halo 8: windows of LR 32 -> HR 128.  Images 40 x 24 (3 x 2 tiles, the last row shifted inward by 8, two model calls) and
    16 x 16 (one tile, all halo replicated)."""
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.inference import predict_dataset
    from csbsr_amd.modeling.build_model import JointModel
    from csbsr_amd.utils.detfill import deterministic_fill
    m = JointModel(base_cfg.clone())
    deterministic_fill(m.state_dict())
    m.eval()
    images = PC.make_images([(40, 24), (16, 16)], seed=23)
    ld = _predict_loader(images, 16, 8, 4)
    assert [ld.chunks(u) for u in ld] == [[(0, 4), (4, 6)], [(6, 7)]] and (ld.wh, ld.ww) == (32, 32)
    host = lambda o: [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()} for d in o]
    a = host(predict_dataset(m, ld))
    b = host(predict_dataset(m, ld))
    for x, y in zip(a, b):
        for k in ("sr_u8", "map_u8", "map_f32", "kernels"):
            assert torch.equal(x[k], y[k]), k
        assert torch.isfinite(x["map_f32"]).all() and torch.isfinite(x["kernels"]).all()
        assert x["sr_u8"].float().std() > 1 and x["map_f32"].std() > 0
    want = PC.host_chain(ld, images, m, lambda w: torch.from_numpy(w).to(DEV), EC.thresholds32()[EC.SAVE_IDX])
    _same(list(predict_dataset(m, ld)), want)
