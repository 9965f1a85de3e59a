"""The pieces the resident loaders and the multi-tensor launches share, no GPU: ResidentDataset's pools against U8Pool built directly
(csbsr_amd/data/pool.py), the messages of U8Pool.check_rows through ResidentDataset.check_selection / check_windows, and the chunk map of
csbsr_amd/multi_tensor.py."""
import numpy as np
import pytest
import torch

SIZES = [(40, 52), (31, 45), (24, 32), (50, 33), (37, 64), (29, 41), (44, 36)]          # of test_resident_cpu.py / test_resized_crop_cpu.py


def _pairs(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return ([rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for H, W in sizes],
            [rng.integers(0, 256, size=(H, W), dtype=np.uint8) for H, W in sizes])


@pytest.fixture(scope="module")
def ds():
    from csbsr_amd.data.resident import ResidentDataset
    return ResidentDataset(*_pairs(SIZES), device="cpu")


def test_resident_dataset_is_two_u8_pools():
    from csbsr_amd.data.pool import U8Pool
    from csbsr_amd.data.resident import ResidentDataset
    images, masks = _pairs([(24, 40), (7, 5), (13, 40), (24, 1), (1, 9), (16, 17)], seed=3)
    ds = ResidentDataset(images, masks, device="cpu")
    for pool, data, offsets, offsets_dev in ((U8Pool(images, 3, "image", "cpu"), ds.image_pool, ds.image_offsets, ds.image_offsets_dev),
                                             (U8Pool(masks, 1, "mask", "cpu"), ds.mask_pool, ds.mask_offsets, ds.mask_offsets_dev)):
        assert data.dtype == torch.uint8 and np.array_equal(data.numpy(), pool.pool.numpy())
        assert offsets.dtype == np.int64 and np.array_equal(offsets, pool.offsets) and np.array_equal(offsets_dev.numpy(), pool.offsets)
        assert ds.dims.dtype == np.int32 and np.array_equal(ds.dims, pool.dims) and np.array_equal(ds.dims_dev.numpy(), pool.dims)
    assert np.array_equal(ds.image_offsets, 3 * ds.mask_offsets)
    for i in range(len(images)):
        a, m = ds.sample(i)
        assert np.array_equal(a, images[i]) and np.array_equal(m[:, :, 0], masks[i])


# the messages below were recorded from the commit before check_selection and check_windows became one function
SELECTION = [
    ((7, 0, 0, 0, 0), 'selection row 1: image index 7 outside the pool of 7'),
    ((-1, 0, 0, 0, 0), 'selection row 1: image index -1 outside the pool of 7'),
    ((0, -1, 0, 0, 0), 'selection row 1: window y0 -1 x0 0 of 24 x 32 leaves image 0 (40 x 52)'),
    ((0, 0, -1, 0, 0), 'selection row 1: window y0 0 x0 -1 of 24 x 32 leaves image 0 (40 x 52)'),
    ((0, 17, 0, 0, 0), 'selection row 1: window y0 17 x0 0 of 24 x 32 leaves image 0 (40 x 52)'),
    ((0, 0, 21, 0, 0), 'selection row 1: window y0 0 x0 21 of 24 x 32 leaves image 0 (40 x 52)'),
    ((2, 1, 0, 0, 0), 'selection row 1: window y0 1 x0 0 of 24 x 32 leaves image 2 (24 x 32)'),
    ((2, 0, 1, 1, 1), 'selection row 1: window y0 0 x0 1 of 24 x 32 leaves image 2 (24 x 32)'),
    ((0, 0, 0, 2, 0), 'selection row 1: mirror / vflip must be 0 or 1'),
    ((0, 0, 0, 0, -1), 'selection row 1: mirror / vflip must be 0 or 1'),
]
GOOD = [(0, 0, 0, 0, 0, 40, 52), (1, 30, 44, 1, 1, 1, 1), (6, 4, 6, 1, 0, 40, 30)]
WINDOWS = [
    ((1, 30, 44, 0, 0, 2, 1), 24, 32, 'window row 1: window y0 30 x0 44 of 2 x 1 leaves image 1 (31 x 45)'),
    ((1, 0, 40, 0, 0, 5, 6), 24, 32, 'window row 1: window y0 0 x0 40 of 5 x 6 leaves image 1 (31 x 45)'),
    ((1, -1, 0, 0, 0, 5, 6), 24, 32, 'window row 1: window y0 -1 x0 0 of 5 x 6 leaves image 1 (31 x 45)'),
    ((1, 0, 0, 0, 0, 0, 6), 24, 32, 'window row 1: window size 0 x 6 must be at least 1 x 1'),
    ((1, 0, 0, 0, 0, 6, -3), 24, 32, 'window row 1: window size 6 x -3 must be at least 1 x 1'),
    ((1, 0, 0, 2, 0, 6, 6), 24, 32, 'window row 1: mirror / vflip must be 0 or 1'),
    ((1, 0, 0, 0, -1, 6, 6), 24, 32, 'window row 1: mirror / vflip must be 0 or 1'),
    ((7, 0, 0, 0, 0, 6, 6), 24, 32, 'window row 1: image index 7 outside the pool of 7'),
    (None, 4, 32, 'window row 0: window 40 x 52 is more than 8 times the output 4 x 32'),
    (None, 24, 6, 'window row 0: window 40 x 52 is more than 8 times the output 24 x 6'),
]


def _message(check, table, h, w):
    with pytest.raises(ValueError) as e:
        check(table, h, w)
    return str(e.value)


@pytest.mark.parametrize("row,expected", SELECTION)
def test_check_selection_message(ds, row, expected):
    assert _message(ds.check_selection, np.array([(0, 16, 20, 1, 1), row], np.int32), 24, 32) == expected


@pytest.mark.parametrize("row,h,w,expected", WINDOWS)
def test_check_windows_message(ds, row, h, w, expected):
    table = np.array(GOOD, np.int32)
    if row is not None:
        table[1] = row
    assert _message(ds.check_windows, table, h, w) == expected


def test_table_shape_and_type_messages(ds):
    good = np.array(GOOD, np.int32)
    ds.check_windows(good, 24, 32)
    ds.check_selection(good[:, :5], 1, 1)
    assert _message(ds.check_selection, np.zeros((2, 4), np.int32), 24, 32) == 'selection table must be integer [B][5], got int32 (2, 4)'
    assert _message(ds.check_selection, np.zeros((2, 5), np.float32), 24, 32) == 'selection table must be integer [B][5], got float32 (2, 5)'
    assert _message(ds.check_selection, good, 24, 32) == 'selection table must be integer [B][5], got int32 (3, 7)'
    assert _message(ds.check_windows, good[:, :5].copy(), 24, 32) == 'window table must be integer [B][7], got int32 (3, 5)'
    assert _message(ds.check_windows, good.astype(np.float32), 24, 32) == 'window table must be integer [B][7], got float32 (3, 7)'


def test_chunk_maps():
    from csbsr_amd import multi_tensor as MT
    assert MT.CHUNK == 8192
    bt, bc = MT.chunk_maps([0, 1, 8192, 8193, 20000], "cpu")
    assert bt.dtype == bc.dtype == torch.int32
    assert bt.tolist() == [1, 2, 3, 3, 4, 4, 4] and bc.tolist() == [0, 0, 0, 1, 0, 1, 2]          # the empty tensor gets no block
    again = MT.chunk_maps([0, 1, 8192, 8193, 20000], "cpu")
    assert again[0] is bt and again[1] is bc
