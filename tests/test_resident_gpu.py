"""The HBM-resident training loader on the device (csbsr_amd/data/resident.py, csrc/resident.hip): the gather kernel against the fixture
recorded from the reference's transforms and against its NumPy restatement, bit for bit; the loader against DeviceDegradation on the
gathered tensors; and one training step fed by the loader against the same step fed host copies."""
import ctypes as C

import numpy as np
import pytest
import torch

import resident_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gather(ds, sel, h, w):
    sel_dev = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).to(DEV)
    hr, mask = ds.gather(sel_dev, len(sel), h, w)
    torch.cuda.synchronize()
    return hr.cpu(), mask.cpu()


def test_kernel_reproduces_the_reference_fixture():
    from csbsr_amd.data.resident import ResidentDataset
    g = RC.load_golden()
    h, w = g["crop"]
    ds = ResidentDataset(g["images"], g["masks"], device=DEV)
    hr, mask = gather(ds, g["sel"], h, w)
    for s in range(len(g["sel"])):
        assert torch.equal(hr[s], torch.from_numpy(g["out_image"][s])), f"image of sample {s} {g['sel'][s].tolist()}"
        assert torch.equal(mask[s], torch.from_numpy(g["out_mask"][s])), f"mask of sample {s} {g['sel'][s].tolist()}"


@pytest.mark.parametrize("crop", [(32, 48), (30, 45), (17, 3)])          # 16-byte rows, row tails, windows narrower than a lane's run
def test_kernel_equals_numpy_on_random_draws(crop):
    from csbsr_amd.data.resident import ResidentDataset
    h, w = crop
    rng = np.random.default_rng(100 + h)
    sizes = [(int(rng.integers(h, h + 40)), int(rng.integers(w, w + 60))) for _ in range(50)]
    sizes[7], sizes[31] = (h, w), (h + 5, w)
    images, masks = RC.random_pairs(rng, sizes, binary_masks=False)
    ds = ResidentDataset(images, masks, device=DEV)
    sel = RC.random_selection(rng, ds.dims, 64, h, w)
    sel[:4, 0] = (7, 31, 7, 31)
    sel[:4, 1:3] = 0
    ds.check_selection(sel, h, w)
    hr, mask = gather(ds, sel, h, w)                                      # channels 3 and channels 1
    assert torch.equal(hr, torch.from_numpy(RC.gather_numpy(images, sel, h, w)))
    assert torch.equal(mask, torch.from_numpy(RC.gather_numpy(masks, sel, h, w)))


def test_kernel_never_leaves_the_image_on_a_bad_window():
    """The host rejects such rows; the kernel is handed them directly here and must clamp every coordinate into the image: the output is
    the edge-replicated image, and the bytes of the neighbouring images never appear."""
    from csbsr_amd.data.resident import ResidentDataset
    h, w = 16, 24
    images = [np.full((20, 30, 3), 0, np.uint8), np.full((18, 26, 3), 200, np.uint8), np.full((20, 30, 3), 0, np.uint8)]
    masks = [np.zeros((20, 30), np.uint8), np.full((18, 26), 200, np.uint8), np.zeros((20, 30), np.uint8)]
    ds = ResidentDataset(images, masks, device=DEV)
    sel = np.array([(1, -5, -7, 0, 0), (1, 9, 11, 1, 0), (1, 40, 2, 0, 1), (1, 2, 100, 1, 1), (1, -3, 8, 1, 0)], np.int32)
    with pytest.raises(ValueError):
        ds.check_selection(sel, h, w)
    hr, mask = gather(ds, sel, h, w)
    want = np.float32(200) / np.float32(255)
    assert (hr == want).all() and (mask == want).all()


def make_loader(seed=3, hr=(32, 48), n=12, **kw):
    from csbsr_amd.data.resident import ResidentDataset, DeviceTrainLoader
    rng = np.random.default_rng(5)
    sizes = [(int(rng.integers(hr[0], hr[0] + 30)), int(rng.integers(hr[1], hr[1] + 30))) for _ in range(n)]
    images, masks = RC.random_pairs(rng, sizes)
    for m in masks:                                                       # a crack-like band every window meets, and a blob
        m[:] = 0
        m[m.shape[0] // 2 - 2:m.shape[0] // 2 + 2, :] = 255
        y, x = int(rng.integers(2, m.shape[0] - 12)), int(rng.integers(2, m.shape[1] - 12))
        m[y:y + 10, x:x + 10] = 255
    ds = ResidentDataset(images, masks, device=DEV)
    args = dict(batch_size=4, seed=seed, vflip_p=0.5)
    args.update(kw)
    return ds, images, masks, DeviceTrainLoader(ds, hr, 4, **args)


def test_batch_equals_device_degradation_on_the_gathered_tensors():
    from csbsr_amd.data.degrade import DeviceDegradation
    ds, images, masks, ld = make_loader()
    sel, params = ld.draw(4)
    x, hr, mask, k, sdf = ld.batch(sel, params)
    assert torch.equal(hr.cpu(), torch.from_numpy(RC.gather_numpy(images, sel.numpy(), ld.h, ld.w)))
    assert torch.equal(mask.cpu(), torch.from_numpy(RC.gather_numpy(masks, sel.numpy(), ld.h, ld.w)))
    x2, hr2, mask2, k2, sdf2 = DeviceDegradation(4, ksize=21, device=DEV)(hr.clone(), mask.clone(), params=params)
    assert x.shape == (4, 3, ld.h // 4, ld.w // 4) and k.shape == (4, 1, 21, 21) and sdf.shape == mask.shape
    assert torch.equal(x, x2) and torch.equal(k, k2) and torch.equal(sdf, sdf2)
    assert all(t.device == torch.device(DEV) and t.dtype == torch.float32 for t in (x, hr, mask, k, sdf))


def test_staging_ring_reuse_and_growth():
    """Six forced tables of 2, 2, 5, 2, 2, 2 rows through a loader of batch_size 2: more calls than the staging ring has slots, the third
    outgrows its slot, and nothing waits for the device in between.  Every batch is the NumPy restatement on its own rows, bit for bit."""
    from csbsr_amd.data.resident import ResidentDataset, DeviceTrainLoader, _SLOTS
    h, w = 16, 24
    rng = np.random.default_rng(21)
    images, masks = RC.random_pairs(rng, [(20, 30)] * 12)
    ld = DeviceTrainLoader(ResidentDataset(images, masks, device=DEV), (h, w), 4, batch_size=2, blur=False, seed=0)
    tables = [RC.random_selection(rng, ld.dataset.dims, B, h, w) for B in (2, 2, 5, 2, 2, 2)]
    assert len(tables) > _SLOTS
    got = [ld.batch(torch.from_numpy(sel))[1:3] for sel in tables]
    for i, (sel, (hr, mask)) in enumerate(zip(tables, got)):
        assert torch.equal(hr.cpu(), torch.from_numpy(RC.gather_numpy(images, sel, h, w))), f"hr of call {i}"
        assert torch.equal(mask.cpu(), torch.from_numpy(RC.gather_numpy(masks, sel, h, w))), f"mask of call {i}"


def test_blur_false_gives_a_delta_kernel_and_the_unblurred_lr():
    from csbsr_amd import _lib as L
    from csbsr_amd.data.degrade import DeviceDegradation
    from csbsr_amd.engine import _ptr
    ds, images, masks, ld = make_loader(blur=False)
    sel, params = ld.draw(4)
    x, hr, mask, k, sdf = ld.batch(sel, None)
    want_k = torch.zeros(4, 1, 21, 21)
    want_k[:, 0, 10, 10] = 1                                              # crack_dataset.py:56-58
    assert torch.equal(k.cpu(), want_k)
    assert torch.equal(hr.cpu(), torch.from_numpy(RC.gather_numpy(images, sel.numpy(), ld.h, ld.w)))
    want_x = torch.empty_like(x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.call("csbsr_aa_bicubic_down_fwd", _ptr(hr), _ptr(want_x), 4 * 3, ld.h, ld.w, 4, 1, st)
    assert torch.equal(x, want_x)
    # the same LR image by the other route: a blur with the delta kernel is the identity (0 * v + 1 * hr, exact for hr >= 0), so the
    # blur=True pipeline handed the delta kernel must give these bits
    same = torch.empty_like(hr)
    L.call("csbsr_blur_fwd", _ptr(hr), _ptr(k), 4, 3, ld.h, ld.w, 21, 1, None, _ptr(same), None, 0, st)
    assert torch.equal(same, hr)
    # and it is the antialiased bicubic of the crop: torch's own resize on the host, to fp32 rounding of a 64-tap weighted mean of
    # values in [0, 1] (|error| <= 64 taps x 2^-24 x sum|w| with sum|w| < 2 for the bicubic kernel: 8e-6; 2e-5 asserted)
    ref_x = torch.nn.functional.interpolate(hr.cpu(), size=(ld.h // 4, ld.w // 4), mode="bicubic", align_corners=False, antialias=True)
    err = float((x.cpu() - ref_x).abs().max())
    print(f"blur=False LR vs torch antialiased bicubic: max abs {err:.3e}")
    assert err <= 2e-5
    assert torch.equal(sdf, DeviceDegradation(4, device=DEV).sdf(mask))
    blurred = make_loader(blur=True)[3]
    xb = blurred.batch(sel, params)[0]
    assert not torch.equal(xb, x)


def test_two_loaders_with_one_seed_yield_identical_batches():
    a, b = make_loader(seed=21, num_iterations=5)[3], make_loader(seed=21, num_iterations=5)[3]
    n = 0
    for ba, bb in zip(a, b):
        assert all(torch.equal(ta, tb) for ta, tb in zip(ba, bb))
        n += 1
    assert n == 5
    c = make_loader(seed=22, num_iterations=1)[3]
    assert not torch.equal(next(iter(c))[1], next(iter(make_loader(seed=21, num_iterations=1)[3]))[1])


def test_iteration_crosses_epochs_with_short_batches():
    ld = make_loader(seed=2, n=10, num_iterations=4)[3]
    assert [b[0].shape[0] for b in ld] == [4, 4, 2, 4]


def test_training_step_fed_by_the_loader_equals_the_step_fed_host_copies():
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    ld = make_loader(seed=8, hr=(64, 64), batch_size=2)[3]
    batch = next(iter(ld))
    m = JointModelWithLoss(base_cfg.clone(), 1000, 0, None)
    deterministic_fill(m.state_dict(), "contractive")
    m.train()
    m.dropout_enabled = False

    def step(x, hr, mask, k, sdf):
        for p in m.parameters():
            p.grad = None
        seg_l, sr_l, _, _, _ = m(40000, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, segment_sdf=sdf)
        (0.7 * sr_l.mean() + 0.3 * seg_l.mean()).backward()
        torch.cuda.synchronize()
        return seg_l.detach().cpu(), sr_l.detach().cpu()

    seg_a, sr_a = step(*batch)
    seg_b, sr_b = step(*(t.cpu() for t in batch))
    assert seg_a.shape == (2,) and torch.isfinite(seg_a).all() and torch.isfinite(sr_a).all()
    assert torch.equal(seg_a, seg_b) and torch.equal(sr_a, sr_b)
