"""numpy restatement of Pillow's two-pass 8-bit bilinear resize over the host tap tables (a plain helper module, imported by the
tests): tests/test_v1_input_cpu.py holds it to Pillow and to the reference's fixture, tests/test_v1_input_gpu.py holds the kernel to it
where the fixture stores no bytes (crops at the origin and the far corner)."""
import numpy as np

from tvts_amd.data_loader import transforms as TR


def resample_u8(frames, new_h: int, new_w: int):
    """numpy restatement of Pillow's two-pass 8-bit bilinear resize over the tables above: uint8 [..., H, W, C] -> [..., new_h,
    new_w, C].  What tvts_resize_crop_u8 computes on the device (there for the crop window only)."""
    a = np.asarray(frames)
    assert a.dtype == np.uint8 and a.ndim >= 3
    half = 1 << (TR.PIL_PRECISION_BITS - 1)

    def one_pass(src, axis, n_out):
        tab = TR.pil_bilinear_coeffs(src.shape[axis], n_out)
        src = np.moveaxis(src, axis, 0).astype(np.int64)
        out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
        for i, (first, k) in enumerate(tab):
            acc = np.full(src.shape[1:], half, dtype=np.int64)
            for j, kj in enumerate(k):
                acc += src[first + j] * kj
            out[i] = np.clip(acc >> TR.PIL_PRECISION_BITS, 0, 255)
        return np.moveaxis(out, 0, axis)

    h_axis, w_axis = a.ndim - 3, a.ndim - 2
    return one_pass(one_pass(a, w_axis, new_w), h_axis, new_h)
