"""csbsr_gather_resize_u8 and the loader's resized_crop mode on the device (csrc/resident.hip, csbsr_amd/data/resident.py): windows of the
output size against csbsr_gather_crop_u8 bit for bit; resampled windows against the fp64 restatement under a bound taken from torch's own
CPU error; the fixture recorded from the reference's transforms; the border clamp; the loader; and one resumed training run.

The tolerance rule, per case: E_ref = max|torch CPU fp32 - fp64 restatement|, E_k = max|kernel - fp64 restatement|, and
E_k <= 2 * E_ref + 2^-24 (the kernel may add taps in another order, contract to FMA or round a weight differently: each one more error of
the class torch itself makes; 2^-24 for the cases where torch happens to be exact)."""
import functools

import numpy as np
import pytest
import torch

import resident_cases as RC
import resized_crop_cases as RZ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gather_resized(ds, sel7, h, w, antialias):
    sel_dev = torch.from_numpy(np.ascontiguousarray(sel7, dtype=np.int32)).to(DEV)
    hr, mask = ds.gather_resized(sel_dev, len(sel7), h, w, antialias)
    torch.cuda.synchronize()
    return hr.cpu().numpy(), mask.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return RZ.wide_inputs() if name == "wide" else RZ.parity_inputs()


@functools.lru_cache(maxsize=None)
def _reference(name, out, antialias):
    """((fp64 restatement, E_ref, bound) for the images, the same for the masks), computed once per case"""
    images, masks = _inputs(name)
    rows = RZ.wide_rows() if name == "wide" else RZ.parity_rows_for(*out)
    return rows, RZ.tolerance(images, rows, *out, antialias), RZ.tolerance(masks, rows, *out, antialias)


def _check(got, ref, what):
    r64, e_ref, bound = ref
    e_k = float(np.abs(got.astype(np.float64) - r64).max())
    per = np.abs(got.astype(np.float64) - r64).reshape(len(got), -1).max(axis=1)
    print(f"{what}: E_k {e_k:.3e}  E_ref {e_ref:.3e}  bound {bound:.3e}  (worst sample {int(per.argmax())})")
    assert got.dtype == np.float32 and e_k <= bound, (what, e_k, bound, per.tolist())


# ------------------------------------------------------------------------------------------------------------------- identity
def test_window_of_the_output_size_is_the_plain_gather():
    """All four flip combinations at offsets 0 / maximal / interior: weights are exactly {1, 0}, so the bits are csbsr_gather_crop_u8's."""
    from csbsr_amd.data.resident import ResidentDataset
    images, masks = RZ.parity_inputs()
    ds = ResidentDataset(images, masks, device=DEV)
    for h, w in (RZ.CROP, (10, 18)):
        rows = []
        for img in (0, 4, 8, 1):
            H, W = RZ.PARITY_SIZES[img]
            for y0, x0 in ((0, 0), (H - h, W - w), ((H - h) // 2, (W - w) // 3), (0, W - w), (H - h, 0)):
                for flips in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    rows.append((img, y0, x0) + flips + (h, w))
        sel7 = np.array(rows, dtype=np.int32)
        ds.check_windows(sel7, h, w)
        sel_dev = torch.from_numpy(sel7[:, :5].copy()).to(DEV)
        want_i, want_m = ds.gather(sel_dev, len(sel7), h, w)
        assert torch.equal(want_i.cpu(), torch.from_numpy(RC.gather_numpy(images, sel7[:, :5], h, w)))
        for antialias in (1, 0):
            got_i, got_m = gather_resized(ds, sel7, h, w, antialias)
            assert torch.equal(torch.from_numpy(got_i), want_i.cpu()), (h, w, antialias)
            assert torch.equal(torch.from_numpy(got_m), want_m.cpu()), (h, w, antialias)


# ------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("antialias", [1, 0])
@pytest.mark.parametrize("name,out", [("parity", RZ.CROP), ("odd", RZ.ODD_OUT), ("wide", RZ.WIDE_OUT)])
def test_kernel_against_the_fp64_restatement(name, out, antialias):
    """One launch per pool (C = 3 and C = 1) with a different window per sample: see resized_crop_cases.parity_rows / wide_rows."""
    from csbsr_amd.data.resident import ResidentDataset
    images, masks = _inputs(name)
    rows, ref_i, ref_m = _reference(name, out, antialias)
    ds = ResidentDataset(images, masks, device=DEV)
    ds.check_windows(rows, *out)
    got_i, got_m = gather_resized(ds, rows, *out, antialias)
    assert got_i.shape == (len(rows), 3) + out and got_m.shape == (len(rows), 1) + out
    _check(got_i, ref_i, f"{name} {out} antialias {antialias} C 3")
    _check(got_m, ref_m, f"{name} {out} antialias {antialias} C 1")
    again_i, again_m = gather_resized(ds, rows, *out, antialias)          # run-to-run bit-reproducible
    assert np.array_equal(again_i, got_i) and np.array_equal(again_m, got_m)


def test_kernel_reproduces_the_reference_fixture():
    from csbsr_amd.data.resident import ResidentDataset
    g = RZ.load_golden()
    h, w = g["crop"]
    ds = ResidentDataset(g["images"], g["masks"], device=DEV)
    ds.check_windows(g["sel"], h, w)
    got_i, got_m = gather_resized(ds, g["sel"], h, w, 1)
    for arrays, got, want, what in ((g["images"], got_i, g["out_image"], "image"), (g["masks"], got_m, g["out_mask"], "mask")):
        r64, e_ref, bound = RZ.tolerance(arrays, g["sel"], h, w, 1)
        _check(got, (r64, e_ref, bound), f"fixture {what}")
        # the fixture itself is a torch CPU fp32 result: it sits E_ref from the fp64 value, the kernel at most `bound`
        assert float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) <= bound + e_ref


# ------------------------------------------------------------------------------------------------------------------- clamp
def test_overhanging_window_replicates_the_border():
    """The host rejects such rows; the kernel is handed them directly.  A small image between two neighbours filled with a sentinel byte,
    windows that hang over it by 1 .. 3 pixels per side (less than the neighbours are large, so no read can leave the allocation): the
    result is the restatement with border replication, and does not change with the sentinel."""
    from csbsr_amd.data.resident import ResidentDataset
    rng = np.random.default_rng(77)
    H, W = RZ.CLAMP_SIZE
    image, mask = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    h, w = RZ.CROP
    results = []
    for sentinel in (255, 0):
        images = [np.full((H, W, 3), sentinel, np.uint8), image, np.full((H, W, 3), sentinel, np.uint8)]
        masks = [np.full((H, W), sentinel, np.uint8), mask, np.full((H, W), sentinel, np.uint8)]
        ds = ResidentDataset(images, masks, device=DEV)
        with pytest.raises(ValueError):
            ds.check_windows(RZ.CLAMP_ROWS, h, w)
        results.append(gather_resized(ds, RZ.CLAMP_ROWS, h, w, 1))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    _check(results[0][0], RZ.tolerance([None, image], RZ.CLAMP_ROWS, h, w, 1), "clamp C 3")
    _check(results[0][1], RZ.tolerance([None, mask], RZ.CLAMP_ROWS, h, w, 1), "clamp C 1")
    # the last row is a window of the output size that hangs over the top: plain replication, exact
    last = RZ.gather_resize_numpy([None, image], RZ.CLAMP_ROWS[-1:], h, w, 1, np.float32)
    assert np.array_equal(results[0][0][-1:], last)


# ------------------------------------------------------------------------------------------------------------------- loader
def make_loader(seed=3, hr=(32, 48), n=12, **kw):
    from csbsr_amd.data.resident import ResidentDataset, DeviceTrainLoader
    rng = np.random.default_rng(5)
    sizes = [(int(rng.integers(hr[0] - 8, hr[0] + 40)), int(rng.integers(hr[1] - 8, hr[1] + 40))) for _ in range(n)]      # some smaller than the crop
    images, masks = RC.random_pairs(rng, sizes)
    for m in masks:                                                       # a crack-like band every window meets, and a blob
        m[:] = 0
        m[m.shape[0] // 2 - 2:m.shape[0] // 2 + 2, :] = 255
        y, x = int(rng.integers(2, m.shape[0] - 12)), int(rng.integers(2, m.shape[1] - 12))
        m[y:y + 10, x:x + 10] = 255
    ds = ResidentDataset(images, masks, device=DEV)
    args = dict(batch_size=4, seed=seed, vflip_p=0.5, resized_crop={"scale": (0.4, 1.0), "ratio": (0.75, 4 / 3)})
    args.update(kw)
    return ds, images, masks, DeviceTrainLoader(ds, hr, 4, **args)


def test_batch_equals_gather_resized_and_device_degradation():
    from csbsr_amd.data.degrade import DeviceDegradation
    ds, images, masks, ld = make_loader()
    sel, params = ld.draw(4)
    assert sel.shape == (4, 7) and len({tuple(r[5:]) for r in sel.tolist()}) > 1
    x, hr, mask, k, sdf = ld.batch(sel, params)
    want_hr, want_mask = ds.gather_resized(sel.to(DEV), 4, ld.h, ld.w, True)
    assert torch.equal(hr, want_hr) and torch.equal(mask, want_mask)
    _check(hr.cpu().numpy(), RZ.tolerance(images, sel.numpy(), ld.h, ld.w, 1), "loader hr")
    soft = mask[(mask > 0) & (mask < 1)]
    assert soft.numel() > 0                                               # the mask went through the same bilinear resample
    x2, hr2, mask2, k2, sdf2 = DeviceDegradation(4, ksize=21, device=DEV)(hr.clone(), mask.clone(), params=params)
    assert x.shape == (4, 3, ld.h // 4, ld.w // 4) and k.shape == (4, 1, 21, 21) and sdf.shape == mask.shape
    assert torch.equal(x, x2) and torch.equal(k, k2) and torch.equal(sdf, sdf2)
    assert all(t.device == torch.device(DEV) and t.dtype == torch.float32 for t in (x, hr, mask, k, sdf))
    again = ld.batch(sel, params)                                         # two runs: bit-identical
    assert all(torch.equal(a, b) for a, b in zip(again, (x, hr, mask, k, sdf)))
    with pytest.raises(ValueError):                                       # a [B,5] table is not this mode's
        ld.batch(sel[:, :5], params)


def test_two_loaders_with_one_seed_yield_identical_batches():
    a, b = make_loader(seed=21, num_iterations=5)[3], make_loader(seed=21, num_iterations=5)[3]
    n = 0
    for ba, bb in zip(a, b):
        assert all(torch.equal(ta, tb) for ta, tb in zip(ba, bb))
        n += 1
    assert n == 5
    c = make_loader(seed=22, num_iterations=1)[3]
    assert not torch.equal(next(iter(c))[1], next(iter(make_loader(seed=21, num_iterations=1)[3]))[1])
    # shuffle=False (the validation loader) jitters too
    v = make_loader(seed=4, shuffle=False)[3]
    sel = v.draw()[0]
    assert sel[:, 0].tolist() == [0, 1, 2, 3] and sel.shape[1] == 7


# ------------------------------------------------------------------------------------------------------------------- trainer
def test_resumed_run_with_resized_crop_is_the_uninterrupted_run(tmp_path):
    """test_trainer_gpu.test_resumed_run_is_the_uninterrupted_run with the option on (Adam, the same sizes): 2 + 2 iterations through
    ``resume`` against 4 in one go; parameters and logged losses are bit-identical."""
    from test_trainer_gpu import _pool, _small_cfg, _small_model
    from csbsr_amd import trainer as T
    from csbsr_amd.data.resident import DeviceTrainLoader
    cfg = _small_cfg("Adam")
    ds = _pool()
    loader = lambda n, seed: DeviceTrainLoader(ds, 64, 4, batch_size=2, num_iterations=n, seed=seed, drop_last=True,
                                               resized_crop={"scale": (0.5, 1.0), "ratio": (0.75, 4 / 3)})
    it0 = 40000

    def run(model, opt, ld, resume_iter, out=None):
        logs = []
        T.do_train(cfg, model, opt, T.build_scheduler(cfg, opt, resume_iter), ld, resume_iter=resume_iter, log_step=1, save_step=2,
                   output_dir=out, log=logs.append)
        return [(r["iteration"], r["segment_loss"], r["sr_loss"], r["boundary_alpha"]) for r in logs if "segment_loss" in r]
    torch.manual_seed(5)
    full = _small_model(cfg, it0)
    logs_full = run(full, T.build_optimizer(cfg, full), loader(4, 31), it0)
    assert [r[0] for r in logs_full] == [40001, 40002, 40003, 40004]
    torch.manual_seed(5)
    first = _small_model(cfg, it0)
    logs_a = run(first, T.build_optimizer(cfg, first), loader(2, 31), it0, str(tmp_path))
    del first
    torch.manual_seed(777)
    torch.rand(3, device=DEV)
    second = _small_model(cfg, 0)
    opt_second = T.build_optimizer(cfg, second)
    ld = loader(4, 999)
    it = T.resume(cfg, str(tmp_path), 40002, second, opt_second, ld)
    assert it == 40002
    logs_b = run(second, opt_second, ld, it)
    assert logs_a + logs_b == logs_full
    sd, sd_full = second.state_dict(), full.state_dict()
    for name, t in sd.items():
        assert torch.equal(t, sd_full[name]), name
    # and the option changed the run: the same seed without it sees other pixels
    plain = DeviceTrainLoader(ds, 64, 4, batch_size=2, num_iterations=1, seed=31, drop_last=True)
    assert next(iter(plain.iter_decisions()))[0].shape[1] == 5
