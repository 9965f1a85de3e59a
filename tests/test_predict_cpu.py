"""Host side of the prediction path (csbsr_amd/data/resident_predict.py, csrc/eval_io.hip: csbsr_stitch_tiles_u8): the tiling rule, the
binding, the work-unit grouping and the fixture recorded from the reference's TTICrackDataSetTest.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import predict_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PH, PW = 4, 6


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("halo", [0, 1, 3])
def test_plan_tiles_covers_every_pixel_exactly_once(halo, scale):
    from csbsr_amd.data.patch_sampler import SplitPatch
    from csbsr_amd.data.resident_predict import plan_tiles
    wh, ww = PH + 2 * halo, PW + 2 * halo
    for h in range(1, 3 * PH + 2):
        for w in range(1, 3 * PW + 2):
            g, s = plan_tiles(h, w, PH, PW, halo, scale, index=5)
            ny, nx = -(-h // PH), -(-w // PW)
            assert g.dtype == s.dtype == np.int32 and g.shape == (ny * nx, 5) and s.shape == (ny * nx, 8), (h, w)
            assert (g[:, 0] == 5).all() and (s[:, 0] == 5).all() and (g[:, 3:] == 0).all() and (s[:, 7] == 0).all()
            cover = np.zeros((scale * h, scale * w), np.int32)
            lr_owner = np.zeros((h, w), np.int32)
            for n, ((_, y0, x0, _, _), (_, dy, dx, sy, sx, th, tw, _)) in enumerate(zip(g, s)):
                iy, ix = divmod(n, nx)                                                      # row-major, the reference's patch order
                assert (dy, dx) == (scale * iy * PH, scale * ix * PW), (h, w, n)
                assert (th, tw) == (scale * (min((iy + 1) * PH, h) - iy * PH), scale * (min((ix + 1) * PW, w) - ix * PW))
                assert th > 0 and tw > 0 and sy >= 0 and sx >= 0 and sy + th <= scale * wh and sx + tw <= scale * ww, (h, w, n)
                assert dy + th <= scale * h and dx + tw <= scale * w
                # the window: the core origin shifted inward at the far edge, minus the halo; the source is the owned origin inside it
                assert (y0, x0) == (min(iy * PH, max(h - PH, 0)) - halo, min(ix * PW, max(w - PW, 0)) - halo), (h, w, n)
                assert (sy, sx) == (scale * (iy * PH - y0), scale * (ix * PW - x0))
                # a core never reads padding where the image has pixels: its rows lie inside the image unless the image is smaller than it
                assert y0 + halo >= 0 and (y0 + halo + PH <= h or h < PH) and x0 + halo >= 0 and (x0 + halo + PW <= w or w < PW)
                cover[dy:dy + th, dx:dx + tw] += 1
                lr_owner[dy // scale:(dy + th) // scale, dx // scale:(dx + tw) // scale] += 1
            assert (cover == 1).all() and (lr_owner == 1).all(), (h, w)
            if halo == 0 and h % PH == 0 and w % PW == 0:                                   # SplitPatch's own tiling
                img = torch.arange(3 * h * w, dtype=torch.float32).view(3, h, w)
                patches, shape = SplitPatch(1, 3, PH, PW)(img)
                assert list(shape[1:]) == [1, ny, nx, 3, PH, PW] and (s[:, 3:5] == 0).all()
                assert (s[:, 5] == scale * PH).all() and (s[:, 6] == scale * PW).all()
                for n, (_, y0, x0, _, _) in enumerate(g):
                    assert torch.equal(patches[n], img[:, y0:y0 + PH, x0:x0 + PW]), (h, w, n)


def test_plan_tiles_rejects_bad_arguments():
    from csbsr_amd.data.resident_predict import plan_tiles
    for bad in ((0, 5, 4, 6, 0, 4), (5, 5, 0, 6, 0, 4), (5, 5, 4, 6, -1, 4), (5, 5, 4, 6, 0, 0)):
        with pytest.raises(ValueError):
            plan_tiles(*bad)


def test_header_and_binding_declare_the_stitch():
    from csbsr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    m = re.search(r"\bint\s+csbsr_stitch_tiles_u8\s*\(([^)]*)\)\s*;", hdr)
    assert m, "csbsr_stitch_tiles_u8 is not declared in include/csbsr_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["csbsr_stitch_tiles_u8"]
    assert res is _lib.i32 and len(argtypes) == len(args) == 12
    for a, t in zip(args, argtypes):                                  # pointers and the stream are void*, int32_t / int64_t scalars as declared
        want = _lib.vp if ("*" in a or a.startswith("csbsr_stream_t")) else {"int32_t": _lib.i32, "int64_t": _lib.i64}[a.split()[0]]
        assert t is want, a
    src = open(os.path.join(ROOT, "csbsr_amd", "csrc", "eval_io.hip")).read()
    assert re.search(r'extern "C" int csbsr_stitch_tiles_u8\(', src)


def _loader(sizes, patch, scale, halo, batch_patches):
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    images = PC.make_images(sizes, seed=3)
    names = [f"im_{i}.png" for i in range(len(sizes))]
    return DevicePredictLoader(ResidentImageSet(images, names, device="cpu"), patch, scale, halo=halo, batch_patches=batch_patches), images


def test_work_units():
    # tiles per image at patch 8: 2, 1, 6, 12 (more than batch_patches), 3, 2, 4
    sizes = [(8, 16), (5, 7), (16, 24), (24, 32), (8, 24), (16, 8), (9, 9)]
    ld, _ = _loader(sizes, 8, 4, halo=2, batch_patches=9)
    tiles = [2, 1, 6, 12, 3, 2, 4]
    assert list(np.diff(ld.tile_start)) == tiles
    assert [(u.i0, u.i1) for u in ld] == [(0, 3), (3, 4), (4, 7)] and len(ld) == 3
    assert [ld.chunks(u) for u in ld] == [[(0, 9)], [(9, 18), (18, 21)], [(21, 30)]]
    for u in ld:
        n = u.t1 - u.t0
        assert n == sum(tiles[u.i0:u.i1]) and (n <= 9 or u.i1 - u.i0 == 1)
        assert all(b - a <= 9 for a, b in ld.chunks(u)) and [a for a, _ in ld.chunks(u)] + [u.t1] == [u.t0] + [b for _, b in ld.chunks(u)]
        hw = [4 * sizes[i][0] * 4 * sizes[i][1] for i in range(u.i0, u.i1)]
        assert u.npix == sum(hw) and list(ld.pix_offsets[u.i0:u.i1]) == list(np.cumsum([0] + hw[:-1]))
        assert set(ld.stitch[u.t0:u.t1, 0]) == set(range(u.i0, u.i1)) == set(ld.gather[u.t0:u.t1, 0])
    assert ld.off1_dev.dtype == ld.off3_dev.dtype == torch.int64 and torch.equal(ld.off3_dev, 3 * ld.off1_dev)
    assert ld.stitch_dev.dtype == ld.gather_dev.dtype == ld.out_dims_dev.dtype == torch.int32
    assert (ld.wh, ld.ww) == (12, 12) and np.array_equal(ld.out_dims, 4 * np.array(sizes))
    # a last short unit, and one unit per image when nothing fits together
    ld, _ = _loader(sizes[:3], 8, 4, halo=0, batch_patches=6)
    assert [(u.i0, u.i1, u.t1 - u.t0) for u in ld] == [(0, 2, 3), (2, 3, 6)]
    ld, _ = _loader(sizes, 8, 4, halo=0, batch_patches=1)
    assert [(u.i0, u.i1) for u in ld] == [(i, i + 1) for i in range(7)] and all(b - a == 1 for u in ld for a, b in ld.chunks(u))
    with pytest.raises(Exception, match="GPU"):
        next(ld.batches(ld.units[0]))                                  # no fallback: batches exist on a GPU only


def test_from_cfg_takes_image_size_as_the_lr_patch():
    from types import SimpleNamespace as NS
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    cfg = NS(INPUT=NS(IMAGE_SIZE=[8, 12]), MODEL=NS(SCALE_FACTOR=4, NUM_CLASSES=1))
    iset = ResidentImageSet(PC.make_images([(16, 24)], 1), ["a.png"], device="cpu")
    ld = DevicePredictLoader.from_cfg(cfg, iset, halo=1)
    assert (ld.ph, ld.pw, ld.scale, ld.wh, ld.ww) == (8, 12, 4, 10, 14) and len(ld.gather) == 4
    with pytest.raises(NotImplementedError):
        DevicePredictLoader(iset, 8, 1)


def test_from_dir_sorts_and_names_the_bad_file(tmp_path):
    from PIL import Image
    from csbsr_amd.data.resident_predict import ResidentImageSet
    imgs = PC.make_images([(5, 7), (6, 4)], 2)
    Image.fromarray(imgs[0]).save(tmp_path / "b.png")
    Image.fromarray(imgs[1]).save(tmp_path / "a.png")
    iset = ResidentImageSet.from_dir(str(tmp_path), device="cpu")
    assert iset.names == ["a.png", "b.png"] and iset.lr.dims.tolist() == [[6, 4], [5, 7]] and iset.lr.offsets.tolist() == [0, 72]
    assert np.array_equal(iset.lr.pool.numpy(), np.concatenate([imgs[1].reshape(-1), imgs[0].reshape(-1)])) and iset.nbytes == 72 + 105
    Image.fromarray(imgs[0][:, :, 0]).save(tmp_path / "c.png")
    with pytest.raises(ValueError, match="c.png"):
        ResidentImageSet.from_dir(str(tmp_path), device="cpu")
    with pytest.raises(FileNotFoundError):
        ResidentImageSet.from_dir(str(tmp_path), pattern="*.jpg", device="cpu")


def test_tables_select_the_windows_of_the_reference_fixture():
    """tests/golden/predict_tti.npz, recorded from the reference's TTICrackDataSetTest + TestTransforms under torch's DataLoader: with halo 0
    the loader's gather rows select the reference's patches in the reference's order, and its stitch rows put a batch of output patches
    where the reference's JointPatch puts them."""
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    g = PC.load_golden()
    assert g["names"] == sorted(g["names"]) and len(g["lr"]) == 3
    iset = ResidentImageSet(g["lr"], g["names"], device="cpu")
    ld = DevicePredictLoader(iset, g["patch"], g["scale"], halo=0, batch_patches=12)
    assert [(u.i0, u.i1) for u in ld] == [(0, 2), (2, 3)]                      # the reference's two batches
    ph, pw, s = *g["patch"], g["scale"]
    for unit, b in zip(ld, g["batches"]):
        assert ld.names[unit.i0:unit.i1] == b["fnames"]
        ref = b["imgs"].reshape(-1, 3, ph, pw)
        rows = ld.gather[unit.t0:unit.t1]
        assert len(rows) == len(ref) and (ld.wh, ld.ww) == (ph, pw)
        got = np.stack([PC.gather_replicate_numpy(g["lr"][r[0]], r[1], r[2], ph, pw) for r in rows])
        assert got.dtype == ref.dtype and np.array_equal(got, ref)
        H, W = (int(v) for v in ld.out_dims[unit.i0])
        assert list(b["img_unfold_shape"][2:]) == [H // (s * ph), W // (s * pw), 3, s * ph, s * pw]
        ramp = PC.ramp_patches(len(ref), 3, s * ph, s * pw)
        tiles = ld.stitch[unit.t0:unit.t1].copy()
        tiles[:, 0] -= unit.i0
        f32, _ = PC.stitch_tiles_numpy(ramp, tiles, ld.out_dims[unit.i0:unit.i1], clip=False)
        assert np.array_equal(f32.reshape(b["joint_ramp"].shape), b["joint_ramp"])


def test_stitch_tiles_numpy_is_stitch_numpy_on_a_uniform_grid():
    """The restatement the GPU tests compare against, checked against the existing one (eval_io_cases.stitch_numpy) where both apply."""
    import eval_io_cases as EC
    B, C, nH, nW, ph, pw = 2, 3, 2, 3, 8, 12
    v = EC.stitch_values((B, C, nH, nW, ph, pw), seed=4)
    v.reshape(-1)[[5, 999]] = np.nan
    tiles = [(b, iy * ph, ix * pw, 0, 0, ph, pw, 0) for b in range(B) for iy in range(nH) for ix in range(nW)]
    for clip in (0, 1):
        wf, wu = EC.stitch_numpy(v, B, C, nH, nW, ph, pw, clip)
        f32, u8 = PC.stitch_tiles_numpy(v, tiles, [(nH * ph, nW * pw)] * B, clip)
        assert np.array_equal(f32.view(np.int32), wf.reshape(-1).view(np.int32)) and np.array_equal(u8, wu.reshape(-1))
