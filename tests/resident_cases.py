"""Shared by the resident-dataset tests and tests/golden/make_resident_golden.py: the NumPy restatement of csbsr_gather_crop_u8 and
small input makers.  No GPU, no reference code."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resident_batch.npz")


def gather_numpy(arrays, sel, h, w):
    """arrays: list of uint8 H x W x C; sel [B][5] = (index, y0, x0, mirror, vflip) -> fp32 [B][C][h][w].
    The flips act on the whole image, the window is taken afterwards, then HWC -> CHW and the IEEE fp32 division by 255."""
    out = []
    for idx, y0, x0, mirror, vflip in np.asarray(sel).tolist():
        a = arrays[idx]
        if a.ndim == 2:
            a = a[:, :, None]
        if mirror:
            a = a[:, ::-1]
        if vflip:
            a = a[::-1]
        win = a[y0:y0 + h, x0:x0 + w]
        assert win.shape[:2] == (h, w), "window leaves the image"
        out.append(win.astype(np.float32).transpose(2, 0, 1) / np.float32(255))
    return np.stack(out)


def random_pairs(rng, sizes, binary_masks=True):
    """uint8 images (every byte value equally likely) and masks for the (H, W) in ``sizes``."""
    images = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for H, W in sizes]
    if binary_masks:
        masks = [(255 * (rng.random((H, W)) < 0.3)).astype(np.uint8) for H, W in sizes]
    else:
        masks = [rng.integers(0, 256, size=(H, W), dtype=np.uint8) for H, W in sizes]
    return images, masks


def random_selection(rng, dims, B, h, w, indices=None):
    """B valid rows over images of sizes ``dims`` [n][2], every image at least h x w."""
    dims = np.asarray(dims)
    idx = rng.integers(0, len(dims), size=B) if indices is None else np.asarray(indices)
    sel = np.empty((B, 5), dtype=np.int32)
    sel[:, 0] = idx
    sel[:, 1] = rng.integers(0, dims[idx, 0] - h + 1)
    sel[:, 2] = rng.integers(0, dims[idx, 1] - w + 1)
    sel[:, 3] = rng.integers(0, 2, size=B)
    sel[:, 4] = rng.integers(0, 2, size=B)
    return sel


def load_golden():
    z = np.load(GOLDEN)
    n = int(z["n_images"])
    return {"images": [z[f"image_{i}"] for i in range(n)], "masks": [z[f"mask_{i}"] for i in range(n)], "sel": z["sel"],
            "crop": tuple(int(v) for v in z["crop"]), "out_image": z["out_image"], "out_mask": z["out_mask"], "path": z["path"]}
