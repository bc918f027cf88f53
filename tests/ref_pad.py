"""The padded window of llicti_decode_images_tensor_o (include/llicti_hip.h, "TENSOR OPTIONS"), restated in plain Python from the header's text:
a second reading of it.  No code of the library is used; tests/test_tensor_layout_cpu.py holds the library's index map and np.pad's against it,
tests/test_hip_tensor_layout.py the kernel bit for bit."""
import numpy as np

NONE, CONSTANT, EDGE, REFLECT, SYMMETRIC = 0, 1, 2, 3, 4
FILL, REFUSED = -1, -2
NAMES = {"constant": CONSTANT, "edge": EDGE, "reflect": REFLECT, "symmetric": SYMMETRIC}


def pad_index(n, t, mode):
    """Coordinate t on an axis of n pixels -> the source index in 0 .. n - 1, FILL, or REFUSED."""
    mode = NAMES.get(mode, mode)
    if n < 1 or mode not in (NONE, CONSTANT, EDGE, REFLECT, SYMMETRIC):
        return REFUSED
    if 0 <= t < n:
        return t
    if mode == NONE:
        return REFUSED                              # the window leaves its image
    if mode == CONSTANT:
        return FILL
    if mode == EDGE:
        return 0 if t < 0 else n - 1
    over = -t if t < 0 else t - (n - 1)             # pixels past the side
    if mode == REFLECT:                             # period 2 n - 2, the edge pixel not repeated: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...
        if over > n - 1:
            return REFUSED
        return -t if t < 0 else (n - 1) - over
    if over > n:                                    # SYMMETRIC, period 2 n, the edge pixel repeated: ... 1 0 | 0 1 ... n-1 | n-1 n-2 ...
        return REFUSED
    return over - 1 if t < 0 else n - over


def window_ok(Hr, Wr, y0, x0, Ho, Wo, mode):
    """Whether the call takes the Ho x Wo window at (y0, x0) of an Hr x Wr decoded grid: every coordinate of either axis maps somewhere."""
    mode = NAMES.get(mode, mode)
    if not (1 <= Ho <= 8160 and 1 <= Wo <= 8160) or (mode != NONE and not (-8160 <= y0 <= 8160 and -8160 <= x0 <= 8160)):
        return False
    return all(pad_index(Hr, y0 + i, mode) != REFUSED for i in range(Ho)) and all(pad_index(Wr, x0 + j, mode) != REFUSED for j in range(Wo))


def padded_window(img_u8, y0, x0, Ho, Wo, mode, fill=(0, 0, 0)):
    """uint8 [3, Hr, Wr] (the DECODED image: for reduce = r pass img[:, ::2 ** r, ::2 ** r]) -> (float32 [3, Ho, Wo] of pixel values on the
    0 .. 255 scale, with fill[c] where the window's row or column maps to "fill"; bool [Ho, Wo], True where it does).  Not flipped."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] == 3
    _, Hr, Wr = img.shape
    rows = [pad_index(Hr, y0 + i, mode) for i in range(Ho)]
    cols = [pad_index(Wr, x0 + j, mode) for j in range(Wo)]
    assert REFUSED not in rows and REFUSED not in cols, "the call refuses this window"
    rows, cols = np.asarray(rows), np.asarray(cols)
    filled = (rows == FILL)[:, None] | (cols == FILL)[None, :]
    out = img[:, np.maximum(rows, 0)][:, :, np.maximum(cols, 0)].astype(np.float32)      # (a "fill" index reads pixel 0: overwritten below)
    for c in range(3):
        out[c][filled] = np.float32(fill[c])
    return out, filled
