"""The resampling arithmetic of llicti_decode_images_tensor_resized (include/llicti_hip.h, "RESIZED CROPS"), restated in numpy float32 from the
header's text: one numpy operation per rounded operation, vectorised over output indices / pixels, sequential over taps.  No code of the
library is used; tests/test_resize_cpu.py holds it against torch's F.interpolate and the library's weight rule against it, tests/test_hip_resize.py
the kernel against it bit for bit."""
import numpy as np

F = np.float32
TAP_MAX = 9                 # taps per axis the kernel is compiled for (scale <= 4 with the filter on)


def axis_taps(n, m, antialias, idx=None):
    """Box extent n -> output extent m, for the output indices idx (default: all) -> (lo [k] int, count [k] int, weights [k, T] float32 with zeros
    behind each index's last tap, total [k] float32); T = the largest count."""
    i = np.arange(m, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    scale = F(n) / F(m)
    support = scale if (antialias and scale > F(1)) else F(1)
    inv = F(1) / support
    center = scale * (i.astype(F) + F(0.5))
    lo = np.maximum(0, np.trunc((center - support) + F(0.5)).astype(np.int64))
    hi = np.minimum(n, np.trunc((center + support) + F(0.5)).astype(np.int64))
    cnt = hi - lo
    T = int(cnt.max())
    t = np.zeros((len(i), T), dtype=F)
    total = np.zeros(len(i), dtype=F)
    for k in range(T):
        d = ((lo + k).astype(F) - center) + F(0.5)
        tk = np.maximum(F(0), F(1) - np.abs(d * inv)).astype(F)
        tk = np.where(k < cnt, tk, F(0)).astype(F)
        t[:, k] = tk
        total = np.where(k < cnt, total + tk, total).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (t / total[:, None]).astype(F)
    w = np.where(np.arange(T)[None, :] < cnt[:, None], w, F(0)).astype(F)
    return lo, cnt, w, total


def resample(box, Ho, Wo, antialias):
    """uint8 [3, hs, ws] -> float32 [3, Ho, Wo] in 0 .. 255: per row tap the sum over the column taps of w * p (left to right from +0, product
    then sum), then the sum over the row taps the same way."""
    box = np.asarray(box)
    assert box.dtype == np.uint8 and box.ndim == 3
    _, hs, ws = box.shape
    ylo, ycnt, wy, _ = axis_taps(hs, Ho, antialias)
    xlo, xcnt, wx, _ = axis_taps(ws, Wo, antialias)
    p = box.astype(F)
    v = np.zeros((3, Ho, Wo), dtype=F)
    for a in range(wy.shape[1]):
        rows = np.minimum(ylo + a, hs - 1)                        # (beyond an index's last tap the weight is zero: x + 0 * p == x)
        h = np.zeros((3, Ho, Wo), dtype=F)
        for b in range(wx.shape[1]):
            cols = np.minimum(xlo + b, ws - 1)
            prod = (wx[:, b][None, None, :] * p[:, rows][:, :, cols]).astype(F)
            h = (h + prod).astype(F)
        v = (v + (wy[:, a][None, :, None] * h).astype(F)).astype(F)
    return v


def bf16_round(x):
    """float32 -> the float32 value of its bfloat16 rounding (to nearest even; NaN as torch writes it)"""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint32) << np.uint32(16)
    r = np.where((u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0x7FC00000), r).astype(np.uint32)
    return r.view(F)


def finish(v, mean=None, std=None, dtype="float32"):
    """v in 0 .. 255 -> v / 255, (x - mean[c]) / std[c], the rounding to dtype ("float32" | "float16" | "bfloat16"); returned as float32 values
    (exactly representable in dtype)."""
    x = (v / F(255.0)).astype(F)
    if mean is not None:
        m, s = np.asarray(mean, dtype=F), np.asarray(std, dtype=F)
        x = ((x - m[:, None, None]).astype(F) / s[:, None, None]).astype(F)
    if dtype == "float16":
        return x.astype(np.float16).astype(F)
    if dtype == "bfloat16":
        return bf16_round(x)
    assert dtype == "float32"
    return x


def resized_crop(img, box, size, antialias, flip=False, mean=None, std=None, dtype="float32"):
    """The whole call for one image: uint8 [3, H, W] (the DECODED image: for reduce = r pass img[:, ::2 ** r, ::2 ** r]), box = (y0, x0, hs, ws)
    -> float32 values [3, Ho, Wo] of the output tensor."""
    y0, x0, hs, ws = box
    src = np.asarray(img)[:, y0:y0 + hs, x0:x0 + ws]
    assert src.shape == (3, hs, ws), "the box leaves the image"
    out = finish(resample(src, size[0], size[1], antialias), mean, std, dtype)
    return out[:, :, ::-1].copy() if flip else out
