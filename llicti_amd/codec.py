"""Host side of the HIP codec: device memory, streams and container plumbing on torch-ROCm tensors.

`HipCodec` owns one C-ABI context (one per GPU / process) and exposes
  - the kernel-level entry points on torch tensors (used by the parity tests), and
  - `encode(rgb_u8[B,3,H,W]) -> (containers, seg_len)` / `decode(...)`, which keep the containers in HBM,
  - helpers turning a device container into the reference's `bytestream_list` and back.
PyTorch is plumbing here (allocation, streams, host copies); every computation happens in the HIP
library.  Nothing in this module imports the CPU oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .weights import pack_state_dict

NSEG = 49                        # segment lengths per image in the C-ABI: config A's 4 + 45 (config B uses the first 4 + 18, the rest are 0)
MODE_AC = 0                      # the reference's container: 45 torchac-algorithm streams per image (config B: 18)
MODELS = {88: 5, 60: 2}          # head width -> wavelet levels: config A, config B (configs/llicti_{A,B}.json)
B_MAX_STREAMS = 18               # config B: xwide streams per image (one per container segment; 9 x 2 levels)
B_MAX_AUTO = 13                  # ... and the largest size-rule count of its "auto" mode (auto_counts(13)[-1] = 18)
NLEVELS_MAX = 5                  # LLICTI_NLEVELS: the level axis of the C-ABI's per-level tables (config B uses the first 2)
PROG_MAX_STREAMS = 128           # rows of llicti_level_cuts' table: the streams of an image


# ---- container "auto": a PURE FUNCTION OF THE IMAGE'S SIZE (round 6).  Round 5's rule also looked at the batch size, the compute-unit count and -- through a
# running mean the model kept -- at what had been coded before, so an image's bytes depended on eval_batch, on the coding order and on the rank count
# (ADVICE r5): a sharded run's log differed from the one-rank run's on exactly the content the reference exists for.  Now an image
# of H x W always gets the same container whatever it is coded with, next to or after.
STREAM_BYTES_BUDGETED = 4.7      # what an xwide v4 stream is budgeted at: measured with the oracle on natural-like and model-drawn images of 321x481 ... 768x512, a container
                                 # of M streams is -16 ... -24 + (4.0 ... 4.9) M bytes larger than the reference-format one (2.3-2.8 per stream on noise, 5.1 on a 1.5-bit
                                 # source; tests/sim_v4.py; 1.8 of them are the 256 lanes' 0.057 bit each)
AC_TERMINATION_BYTES = 22.5      # ... the offset: what the reference format spends on its 45 range-coder terminations, less the 1.5 bytes the tables differ by
XWIDE_MIN_SHARE = 6144           # last-stage symbols per stream: the tail fills the 7,936-bit payload the initial states carry from 1.3 bits per symbol up (the reference's
                                 # trained model on natural images: 1.68, exp_debug.log.1:2682; a source cheaper than that leaves payload unused: ~1 byte per missing 8 bits)
NARROW_MIN_TAIL = 512            # ... and a 64-lane stream its 1,984 bits
LENGTH_TABLE_BYTES = 4.0         # a stream of a 64- / 128-stream container pays a u32 in its segment's length table


def last_stage_bits(seg_len, H, W):
    """Bits per symbol the LAST stage's Cg stream (segment 48: level 0, band x10) of an image in the REFERENCE-FORMAT container took
    (bench.py reports it for its content classes).  seg_len: the image's 49 segment lengths."""
    return 8.0 * float(seg_len[NSEG - 1]) / max(1, (H // 2) * (W // 2))


def image_streams(H, W, nlevels=5):
    """xwide v4 streams of an H x W image in container "auto" -- a function of the size alone.  Two limits.  BYTES: M streams cost about
    STREAM_BYTES_BUDGETED M over the ideal code length, the reference format's terminations AC_TERMINATION_BYTES, and the north star's 0.001 bpp
    are H W / 8000 bytes (tests/test_oracle_golden.py::test_auto_container_budget_by_size holds the oracle's sizes against it).  PAYLOAD: a
    stream's 256 initial states carry 992 bytes that only its own share of the LAST stage's symbols can fill.  768x512: 15; 0: no xwide stream
    fits (auto_container falls back to one 64-lane stream or the reference format).  More than 32 streams come as 64 or 128 (two / four per
    container segment behind a table of their lengths)."""
    nc_last = (H // 2) * (W // 2)                 # coded positions of level 0, band x10
    if nlevels != 5:
        # config B: AC_TERMINATION_BYTES is 24 bytes of range-coder terminations for config A's 45 streams less 1.5 bytes by which the two
        # formats' tables differ (its comment above); config B's reference format has 9 L = 18 streams, so 24 * 18 / 45 = 9.6 bytes of
        # terminations, less the same 1.5.  The count stays within B_MAX_AUTO.
        budget = H * W / 8000.0 + (AC_TERMINATION_BYTES + 1.5) * 9 * nlevels / 45 - 1.5
        return max(0, min(int(budget / STREAM_BYTES_BUDGETED), nc_last // XWIDE_MIN_SHARE, B_MAX_AUTO))
    budget = H * W / 8000.0 + AC_TERMINATION_BYTES
    m = min(int(budget / STREAM_BYTES_BUDGETED), nc_last // XWIDE_MIN_SHARE)
    if m > 32:
        for big in (128, 64):
            if big * (STREAM_BYTES_BUDGETED + LENGTH_TABLE_BYTES) <= budget and nc_last // XWIDE_MIN_SHARE >= big:
                return big
        m = 32
    return max(0, m)


def image_mode(H, W, mixed=False, nlevels=5):
    """ENCODER mode of ONE image in container "auto": MODE_RANS_AUTO(image_streams(H, W)) -- xwide v4 streams, their count picked by the encoder from
    the image itself: what its size gives, a third more where the last stage's symbols are expensive (an xwide stream costs ~2.5 bytes there instead
    of ~4.5), half where the last stage is too cheap to fill the streams' payloads; an image too small for one xwide stream gets a 64-lane stream
    (from ~45x45 pixels) or -- only where the call holds images of one size (`mixed` False) -- the reference format."""
    m = image_streams(H, W, nlevels)
    if nlevels != 5:            # config B: xwide streams or the reference format only
        return MODE_RANS_AUTO(m) if m >= 1 else (MODE_RANS(1, wide=2) if mixed else MODE_AC)
    if m > 32:
        return MODE_RANS(m, wide=2)             # (64 / 128 streams: very large images; the count is the size rule's)
    if m >= 1:
        return MODE_RANS_AUTO(m)
    if (H // 2) * (W // 2) >= NARROW_MIN_TAIL or mixed:
        return MODE_RANS(1)
    return MODE_AC


def auto_container(H, W):
    """Name of the "auto" ENCODER mode of an H x W image (image_mode): "xauto15" for 768x512 -- the container that comes out is xrans8, xrans15 or
    xrans20, by the image's content."""
    return name_of_mode(image_mode(H, W))


def auto_modes(sizes, nlevels=5):
    """Container modes of the images of ONE call ([(H, W), ...]) in container "auto": each image's own (image_mode) -- xwide streams, their number per image
    a function of its size -- unless one of them is too small for an xwide stream: the images of a call share a lane kind, so then every image of the
    call gets one 64-lane stream (the reference format, where all are that small and of one size).  What an image of a call of EQUAL sizes gets depends
    on its size alone; in a call of mixed sizes a tiny neighbour (below ~90x90 pixels) can push an image to the 64-lane kind -- the reference's test set
    has no such image (tests/golden/eval_shapes.json: 321x481 is its smallest)."""
    mixed = len(set(sizes)) > 1
    modes = [image_mode(h, w, mixed, nlevels) for h, w in sizes]
    if all(_mode_wide(m) == 2 for m in modes if m != MODE_AC) and MODE_AC not in modes:
        return modes
    if all(m == MODE_AC for m in modes):
        return modes
    return [MODE_RANS(1, wide=2 if nlevels != 5 else 0)] * len(sizes)


def MODE_RANS(M=8, wide=False):
    """rANS container: M independent interleaved rANS streams per image.  wide = 0 / False: 64 lanes per stream, M in 1 .. 32, 64, 128 (v3);
    wide = 1 / True: 128 lanes (two 64-symbol chunks per coder step), M in 1 .. 14 (v3); wide = 2 ("xwide"): 256 lanes, one decoder lane per
    symbol, the v4 stream layout, M in 1 .. 32, 64, 128 (include/llicti_hip.h)."""
    return (0x100 + 0x200 * int(wide)) | int(M)


def MODE_RANS_AUTO(M):
    """ENCODE ONLY: xwide v4 streams whose count the encoder picks per image, on the device, from the image itself (include/llicti_hip.h,
    LLICTI_MODE_RANS_X_AUTO): M = the count the image's size gives (image_streams); expensive last-stage symbols -> M + ceil(M / 3), a last stage
    too cheap to fill M payloads -> ceil(M / 2).  The container is an ordinary MODE_RANS(count, wide=2) one: its header says which (mode_of_header)."""
    return 0x10500 | int(M)


def _mode_auto(mode: int) -> bool:
    return bool(mode & 0x10000)


def auto_counts(M):
    """The stream counts an "auto" encode of size-rule count M may pick (llicti_amd/csrc/host_types.hpp: rans_auto_pick): (a last stage that cannot
    fill the payloads, cheap symbols, default, expensive symbols) = (ceil(M / 2), ceil(2 M / 3), M, min(32, M + ceil(M / 3)))."""
    return (M + 1) // 2, (2 * M + 2) // 3, M, min(32, M + (M + 2) // 3)


def _mode_wide(mode: int) -> int:
    return ((mode & 0xF00) - 0x100) // 0x200


def rans_tag(M, wide=False):
    """Header byte 0 of a rANS container with M streams per image (xwide v4: 0xE8 whatever M -- the count is in the pad field, rans_pad_hi)."""
    wide = int(wide)
    ext = 1 if (M > 32 or wide) else 0
    if wide == 2:
        v = 16
    elif wide == 1:
        v = M + 1
    else:
        v = {64: 0, 128: 1}[M] if ext else M - 1
    return 0x88 | (ext << 6) | (((v >> 3) & 3) << 4) | (v & 7)


def rans_pad_hi(M, wide=False):
    """Bits 10 .. 15 of the header's int16 pad field: the stream count of an xwide v4 container (1 .. 32 as they are, 33 / 34 = 64 / 128 streams),
    zero in every other container."""
    return (M if M <= 32 else {64: 33, 128: 34}[M]) if int(wide) == 2 else 0


def mode_of_header(hdr, pad=None) -> int:
    """Container mode of a header: `hdr` = its 17 bytes (bytes 0 .. 2, the 12 min / max bytes, the int16 pad field), or a bytestream_list, or
    byte 0 alone with the pad field in `pad` (only an xwide v4 container needs it: its stream count lives in the field's bits 10 .. 15)."""
    if isinstance(hdr, (list, tuple)):
        hdr = bytes(hdr[0][0]) + bytes(hdr[0][1]) + bytes(hdr[0][2])
    if isinstance(hdr, (bytes, bytearray, np.ndarray)):
        byte0 = int(hdr[0])
        if len(hdr) >= 17:
            pad = int(hdr[15]) | (int(hdr[16]) << 8)
    else:
        byte0 = int(hdr)
    u = 0 if pad is None else (int(pad) >> 10) & 0x3F
    if byte0 == 5:
        return MODE_AC
    if byte0 == 2:              # config B's reference format (2 scales): its pad field has 4 bits
        if pad is not None and int(pad) >> 4:
            raise ValueError(f"pad field 0x{int(pad):04x} of a 2-level container has bits above its 4 pad flags")
        return MODE_AC
    if byte0 == 0xE9:           # config B's xwide v4 streams (llicti_amd/csrc/host_plan.hpp: rans_byte0): the count as in 0xE8, pad bits 4 .. 9 zero
        if pad is None or not (1 <= u <= 34) or (int(pad) & 0x3F0):
            raise ValueError(f"container tag 0xe9 (config B, xwide v4) needs its stream count in the pad field and pad bits 4 .. 9 clear")
        return MODE_RANS(u if u <= 32 else {33: 64, 34: 128}[u], wide=2)
    if (byte0 & 0x88) == 0x88:          # rANS: bits 5,4,2,1,0 = v; bit 6 clear: M = v + 1; set: v = 0, 1 -> 64, 128 streams, 2 .. 15 -> v - 1 wide streams,
        v = (((byte0 >> 4) & 3) << 3) | (byte0 & 7)       # 16 -> xwide streams in the v4 layout, their count in the pad field's high bits
        if (byte0 >> 6) & 1:
            if v >= 16:
                if v != 16 or not (1 <= u <= 34):
                    raise ValueError(f"container tag 0x{byte0:02x} with pad field high bits {u}: an xwide container of the retired v3 layout (rounds 4-5), "
                                     "or an xwide v4 tag without its pad field -- this build reads and writes xwide v4")
                return MODE_RANS(u if u <= 32 else {33: 64, 34: 128}[u], wide=2)
            if u:
                raise ValueError("pad field high bits set in a container that is not xwide v4")
            if v <= 1:
                return MODE_RANS(64 << v)
            return MODE_RANS(v - 1, wide=1)
        if u:
            raise ValueError("pad field high bits set in a container that is not xwide v4")
        return MODE_RANS(v + 1)
    if (byte0 & 0x88) == 0x80:
        raise ValueError(f"container tag 0x{byte0:02x} is the retired LLICTI-rANS v2 format; this build reads and writes v3 / v4 only")
    raise ValueError(f"unknown container tag 0x{byte0:02x}")


def mode_of_name(name: str) -> int:
    """"ac" | "rans<M>" | "wrans<M>" (wide streams: 128 lanes) | "xrans<M>" (xwide streams: 256 lanes) -> mode."""
    name = str(name).lower()
    if name == "ac":
        return MODE_AC
    if name.startswith("xauto"):
        return MODE_RANS_AUTO(int(name[5:]))
    if name.startswith("xrans"):
        return MODE_RANS(int(name[5:]), wide=2)
    if name.startswith("wrans"):
        return MODE_RANS(int(name[5:]), wide=1)
    if name.startswith("rans"):
        return MODE_RANS(int(name[4:] or 8))
    raise ValueError(f"unknown container {name!r}: ac, rans<M>, wrans<M>, xrans<M>, xauto<M> (or \"auto\" where the image sizes are known)")


def name_of_mode(mode: int) -> str:
    if _mode_auto(mode):
        return "xauto%d" % (mode & 0xFF)
    return "ac" if mode == MODE_AC else ("rans%d", "wrans%d", "xrans%d")[_mode_wide(mode)] % (mode & 0xFF)


def reduced_dims(H, W, reduce):
    """Size of an H x W image decoded at `reduce` (HipCodec.decode(..., reduce=r)): (ceil(H / 2^r), ceil(W / 2^r)) -- the shape of
    img[::2**r, ::2**r].  The decode is a DECIMATION of the lossless image (the lazy wavelet has no smoothing filter: fine texture aliases)."""
    H, W, r = int(H), int(W), int(reduce)
    if H < 1 or W < 1 or not 0 <= r <= 5:
        raise ValueError(f"reduced_dims: H={H} W={W} reduce={r} (need H, W >= 1 and 0 <= reduce <= 5)")
    return (H + (1 << r) - 1) >> r, (W + (1 << r) - 1) >> r


# Interleaved pixel formats of encode_px / decode_px (LLICTI_PIX_*): three colour bytes in the named order; the 4-byte formats carry a fourth byte
# that the encoder ignores and the decoder writes as 255 (alpha is not coded).
PIX_RGB8, PIX_BGR8, PIX_RGBA8, PIX_BGRA8 = 0, 1, 2, 3
PIX_FORMATS = {"rgb": PIX_RGB8, "bgr": PIX_BGR8, "rgba": PIX_RGBA8, "bgra": PIX_BGRA8}


def pixel_format(fmt) -> int:
    """"rgb" | "bgr" | "rgba" | "bgra" (or a PIX_* constant) -> the PIX_* constant."""
    if isinstance(fmt, str):
        if fmt.lower() not in PIX_FORMATS:
            raise ValueError(f"unknown pixel format {fmt!r} (one of {', '.join(PIX_FORMATS)})")
        return PIX_FORMATS[fmt.lower()]
    return int(fmt)


def pixel_bytes(fmt) -> int:
    """Bytes per pixel of a format (llicti_pixel_bytes; works without a device)."""
    n = int(_lib.lib().llicti_pixel_bytes(pixel_format(fmt)))
    if n == 0:
        raise ValueError(f"unknown pixel format {fmt!r}")
    return n


def pixel_span(fmt, H, W, pitch=0) -> int:
    """Bytes from the first pixel of an H x W window to the end of its last one, (H - 1) * pitch + W * bpp (llicti_pixel_span; pitch 0: tight rows)."""
    n = int(_lib.lib().llicti_pixel_span(pixel_format(fmt), int(H), int(W), int(pitch)))
    if n == 0:
        raise ValueError(f"pixel_span: format {fmt!r}, H={H}, W={W}, pitch={pitch} (need a known format, H, W >= 1 and pitch >= W * bpp)")
    return n


# Element types of decode_tensor's output (LLICTI_T_*)
T_F32, T_F16, T_BF16 = 0, 1, 2
TENSOR_DTYPES = {torch.float32: T_F32, torch.float16: T_F16, torch.bfloat16: T_BF16}


def tensor_elem_bytes(dtype) -> int:
    """Bytes per element of a decode_tensor dtype (a torch dtype or LLICTI_T_*; llicti_tensor_elem_bytes, works without a device)."""
    n = int(_lib.lib().llicti_tensor_elem_bytes(int(TENSOR_DTYPES.get(dtype, dtype))))
    if n == 0:
        raise ValueError(f"unknown tensor dtype {dtype!r} (torch.float32, torch.float16, torch.bfloat16)")
    return n


def crc32_combine(crc_a, crc_b, len_b) -> int:
    """zlib's crc32_combine: crc32(A + B) from crc32(A), crc32(B) and len(B) (llicti_crc32_combine, works without a device)."""
    return int(_lib.lib().llicti_crc32_combine(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b)))


def crc32_geometry():
    """(pixels a lane of the digest kernel owns, pixels a workgroup owns) -- llicti_crc32_geometry, works without a device: an image of n pixels
    has the kernel's seams at n - k * lane and n - k * group."""
    lane, group = C.c_int(), C.c_int()
    _lib.check(_lib.lib().llicti_crc32_geometry(C.byref(lane), C.byref(group)))
    return lane.value, group.value


def tensor_window_ok(H, W, reduce, y0, x0, Ho, Wo) -> bool:
    """Whether an Ho x Wo window at (y0, x0) lies inside an H x W image decoded at `reduce` (llicti_tensor_window_ok, works without a device)."""
    return bool(_lib.lib().llicti_tensor_window_ok(int(H), int(W), int(reduce), int(y0), int(x0), int(Ho), int(Wo)))


# Tensor options (llicti_tensor_opts): layouts, pad modes and fill spaces by the names the Python calls take
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1
PAD_NONE, PAD_CONSTANT, PAD_EDGE, PAD_REFLECT, PAD_SYMMETRIC = 0, 1, 2, 3, 4
FILL_PIXEL, FILL_OUTPUT = 0, 1
PAD_MODES = {"constant": PAD_CONSTANT, "edge": PAD_EDGE, "reflect": PAD_REFLECT, "symmetric": PAD_SYMMETRIC}
FILL_SPACES = {"pixel": FILL_PIXEL, "output": FILL_OUTPUT}


def pad_index(n, t, mode) -> int:
    """Where coordinate t of a padded window lands on an axis of n pixels under `mode` (a name of PAD_MODES or LLICTI_PAD_*): the source index in
    0 .. n - 1, -1 for "fill", -2 for refused (llicti_pad_index: the function the kernel calls, compiled for the host; works without a device)."""
    return int(_lib.lib().llicti_pad_index(int(n), int(t), int(PAD_MODES.get(mode, mode))))


def tensor_window_pad_ok(H, W, reduce, y0, x0, Ho, Wo, mode) -> bool:
    """Whether decode_tensor(pad=dict(mode=...)) takes the Ho x Wo window at (y0, x0) -- either may be negative -- of an H x W image decoded at
    `reduce` (llicti_tensor_window_pad_ok, works without a device)."""
    return bool(_lib.lib().llicti_tensor_window_pad_ok(int(H), int(W), int(reduce), int(y0), int(x0), int(Ho), int(Wo), int(PAD_MODES.get(mode, mode))))


def center_crop_origins(sizes, size, reduce=0):
    """torchvision's CenterCrop(size) as the windows of decode_tensor: sizes = (H, W) per image at FULL size, size = (Ho, Wo), reduce one int or
    one per image -> (y0s, x0s) on every image's decoded grid (reduced_dims at its reduce), for origin=.  An image smaller than the crop on an
    axis is padded first, as CenterCrop pads it -- (c - n) // 2 in front, (c - n + 1) // 2 behind --, and the window then starts at
    int(round((n' - c) / 2.0)) of the padded extent n': on the image's own grid that origin is NEGATIVE, so such a batch goes with
    pad=dict(mode="constant").  Pure Python, no device."""
    Ho, Wo = int(size[0]), int(size[1])
    sizes = list(sizes)
    rs = [int(reduce)] * len(sizes) if isinstance(reduce, (int, np.integer)) else [int(r) for r in reduce]
    assert len(rs) == len(sizes) and Ho >= 1 and Wo >= 1

    def origin(n, c):
        front = (c - n) // 2 if n < c else 0
        behind = (c - n + 1) // 2 if n < c else 0
        return int(round((n + front + behind - c) / 2.0)) - front
    dims = [reduced_dims(h, w, r) for (h, w), r in zip(sizes, rs)]
    return [origin(h, Ho) for h, _ in dims], [origin(w, Wo) for _, w in dims]


def _tensor_opts(channels_last, pad):
    """channels_last= and pad= of the tensor decodes -> None (nothing new is asked for: the call is its sibling) or a _lib.TensorOpts"""
    if not channels_last and pad is None:
        return None
    o = _lib.TensorOpts(LAYOUT_NHWC if channels_last else LAYOUT_NCHW, PAD_NONE, FILL_PIXEL, (0.0, 0.0, 0.0))
    if pad is not None:
        pad = dict(pad)
        mode, fill, space = pad.pop("mode"), pad.pop("fill", 0), pad.pop("space", "pixel")
        if pad:
            raise TypeError(f"pad: unknown keys {sorted(pad)}")
        if isinstance(mode, str) and mode not in PAD_MODES:
            raise ValueError(f"pad mode {mode!r} (one of {sorted(PAD_MODES)})")
        if isinstance(space, str) and space not in FILL_SPACES:
            raise ValueError(f"fill space {space!r} (one of {sorted(FILL_SPACES)})")
        fill = [float(fill)] * 3 if isinstance(fill, (int, float, np.integer, np.floating)) else [float(v) for v in fill]
        assert len(fill) == 3
        o.pad_mode, o.fill_space = int(PAD_MODES.get(mode, mode)), int(FILL_SPACES.get(space, space))      # (an int goes through: the library says what it does not know)
        o.fill[0], o.fill[1], o.fill[2] = fill
    return o


RESIZE_BOX_SLICE = 128         # images per launch of the resized decode's last kernel (kResizeBoxMax: a larger batch takes several launches)
RESIZE_TAP_MAX = 9             # taps per axis that kernel is compiled for (kResizeTapMax)


def resize_window_ok(H, W, reduce, y0, x0, hs, ws, Ho, Wo, antialias=True) -> bool:
    """Whether decode_tensor_resized takes the hs x ws box at (y0, x0) of an H x W image decoded at `reduce` for an Ho x Wo output
    (llicti_resize_window_ok, works without a device): inside the decoded image, Ho, Wo in 1 .. 8160, and with the filter on a scale of at
    most 4 per axis."""
    return bool(_lib.lib().llicti_resize_window_ok(int(H), int(W), int(reduce), int(y0), int(x0), int(hs), int(ws), int(Ho), int(Wo), int(antialias)))


def resize_axis(n, m, antialias, i, cap=RESIZE_TAP_MAX):
    """The taps of output index i when n source pixels are resampled to m (llicti_resize_axis: the function the kernel calls, compiled for the
    host) -> (count, first source index, float32 weights [cap], zeros behind the last tap)."""
    lo = C.c_int(0)
    w = np.zeros(int(cap), dtype=np.float32)
    cnt = int(_lib.lib().llicti_resize_axis(int(n), int(m), int(bool(antialias)), int(i), C.byref(lo), w.ctypes.data_as(C.POINTER(C.c_float)), int(cap)))
    return cnt, int(lo.value), w


def _box_on_grid(box, r):
    """A full-resolution box (y0, x0, h, w) as the pixels of the grid decimated by 2^r that lie inside it (resized_crop_plan states the rule)"""
    y0, x0, h, w = (int(v) for v in box)
    s = 1 << r
    y0r, x0r = -(-y0 // s), -(-x0 // s)
    return y0r, x0r, (y0 + h - 1) // s + 1 - y0r, (x0 + w - 1) // s + 1 - x0r


def _box_must_fit(H, W, box):
    y0, x0, h, w = box
    if not (0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W):
        raise ValueError(f"box (y0 {y0}, x0 {x0}, {h} x {w}) leaves its {H} x {W} image")


def resized_crop_plan(sizes, boxes_full, size, nlevels=5, per_image=False):
    """The `reduce` a batch of resized crops can be decoded at, and its boxes on that grid.  sizes: (H, W) per image; boxes_full: (y0, x0, h, w)
    per image in FULL-resolution pixels (torchvision's RandomResizedCrop.get_params order); size = (Ho, Wo) -> (reduce, boxes_reduced) for
    decode_tensor_resized.  reduce is ONE value for the call: the largest r in 0 .. nlevels at which EVERY image's box
    still has at least Ho rows and Wo columns of decoded pixels (0 if none has: the boxes are then magnified) -- one tight crop sends the whole
    batch through level 0.  per_image=True -> ([r_b], boxes_reduced) for decode_tensor_resized(reduce=[...]): r_b is the largest r at which
    image b's OWN box keeps Ho x Wo decoded pixels (0 if none does), and box b is mapped to its image's grid.  A box maps to the pixels of the
    decimated grid that lie inside it: y0r = ceil(y0 / 2^r), y1r = floor((y0 + h - 1) / 2^r) + 1, and the same for the columns.
    A REDUCED DECODE IS A DECIMATION -- every 2^r-th pixel of the image, taken without a low-pass filter -- so it ALIASES: fine detail of the
    source folds into the crop, where a full decode followed by an antialiased resize would have averaged it out.  What is gained is that the r
    finest levels are never decoded (level 0 alone is three quarters of the CNN work).  Pure Python, no device."""
    Ho, Wo = int(size[0]), int(size[1])
    sizes, boxes_full = list(sizes), list(boxes_full)
    assert len(sizes) == len(boxes_full) and Ho >= 1 and Wo >= 1
    for (H, W), box in zip(sizes, boxes_full):
        _box_must_fit(H, W, box)
    if per_image:
        rs = [max([0] + [r for r in range(1, int(nlevels) + 1) if _box_on_grid(b, r)[2] >= Ho and _box_on_grid(b, r)[3] >= Wo]) for b in boxes_full]
        return rs, [_box_on_grid(b, r) for b, r in zip(boxes_full, rs)]
    reduce = 0
    for r in range(1, int(nlevels) + 1):
        if all(m[2] >= Ho and m[3] >= Wo for m in (_box_on_grid(b, r) for b in boxes_full)):
            reduce = r
    return reduce, [_box_on_grid(b, reduce) for b in boxes_full]


VIEW_SLICE = 128               # views per launch of the views call's last kernel (kViewMax: a longer group takes several launches)


def multi_crop_plan(sizes, groups_full, nlevels=5, per_image=False):
    """resized_crop_plan for views (decode_tensor_views): several crops per image, of several output sizes, from ONE decode.  sizes: (H, W) per
    image; groups_full: a list of (size, image_indices, boxes_full) -- size = (Ho, Wo) of the group, image_indices[v] the image view v is cut
    from (None: view v is image v), boxes_full[v] = (y0, x0, h, w) in FULL-resolution pixels of that image -> (reduce, [boxes_reduced per
    group]).  reduce is ONE value for the call: the largest r in 0 .. nlevels at which EVERY view of EVERY group still has at least Ho x Wo decoded
    pixels of its group's size in its box (0 if none has) -- the small crops of a multi-crop set decide it.  per_image=True -> ([r_b], the
    same) for decode_tensor_views(reduce=[...]): r_b is the smallest such r over the views that name image b, nlevels for an image no view
    names (its DC band only), and every view's box is mapped to its image's grid.  The box mapping is
    resized_crop_plan's, and so is what it says about a reduced decode: a DECIMATION, which aliases.  For one group with image_indices None it
    returns what resized_crop_plan returns.  Pure Python, no device."""
    sizes = list(sizes)
    groups = []
    for size, image, boxes in groups_full:
        Ho, Wo = int(size[0]), int(size[1])
        boxes = list(boxes)
        image = list(range(len(sizes))) if image is None else [int(b) for b in image]
        assert len(image) == len(boxes) and Ho >= 1 and Wo >= 1
        for b, box in zip(image, boxes):
            if not 0 <= b < len(sizes):
                raise ValueError(f"a view names image {b}: the batch has images 0 .. {len(sizes) - 1}")
            _box_must_fit(sizes[b][0], sizes[b][1], box)
        groups.append((Ho, Wo, boxes, image))
    if per_image:
        rs = [int(nlevels)] * len(sizes)
        for Ho, Wo, boxes, image in groups:
            for b, box in zip(image, boxes):
                rs[b] = min(rs[b], max([0] + [r for r in range(1, int(nlevels) + 1) if _box_on_grid(box, r)[2] >= Ho and _box_on_grid(box, r)[3] >= Wo]))
        return rs, [[_box_on_grid(box, rs[b]) for b, box in zip(image, boxes)] for _, _, boxes, image in groups]
    groups = [g[:3] for g in groups]
    reduce = 0
    for r in range(1, int(nlevels) + 1):
        if all(m[2] >= Ho and m[3] >= Wo for Ho, Wo, boxes in groups for m in (_box_on_grid(b, r) for b in boxes)):
            reduce = r
    return reduce, [[_box_on_grid(b, reduce) for b in boxes] for _, _, boxes in groups]


def _reduce_arg(reduce, B):
    """`reduce=` of the decode calls: one int for the call -> (r, None); a sequence of B ints, image b stopping at its own level
    (the llicti_decode_images_*_rv calls) -> (None, int32 array)."""
    if isinstance(reduce, (int, np.integer)):
        return int(reduce), None
    rv = np.ascontiguousarray(list(reduce), dtype=np.int32)
    if rv.shape != (B,):
        raise ValueError(f"reduce: {rv.size} values for a batch of {B} images (one int, or one per image)")
    return None, rv


def _reduced_sizes(Hs, Ws, r, rv):
    """every image's decoded size at the call's reduce r, or at its own rv[b] (a value the library will refuse counts as 0 here: the call says so)"""
    rs = [r] * len(Hs) if rv is None else [int(v) for v in rv]
    return [reduced_dims(h, w, k) if 0 <= k <= 5 else (int(h), int(w)) for h, w, k in zip(Hs, Ws, rs)]


def _flip_arg(flip, n):
    fl = None if flip is None else np.ascontiguousarray(np.asarray(flip) != 0, dtype=np.uint8)
    assert fl is None or fl.shape == (n,)
    return fl


def _norm_args(mean, std):
    mn = None if mean is None else np.ascontiguousarray(mean, dtype=np.float32)
    sd = None if std is None else np.ascontiguousarray(std, dtype=np.float32)
    assert (mn is None or mn.shape == (3,)) and (sd is None or sd.shape == (3,))
    return mn, sd


def _box_columns(boxes, n):
    """n boxes (y0, x0, hs, ws), or None -> the four int32 columns the library takes (None each)"""
    if boxes is None:
        return [None] * 4
    bx = np.ascontiguousarray(boxes, dtype=np.int32)
    assert bx.shape == (n, 4)
    return [np.ascontiguousarray(bx[:, k]) for k in range(4)]


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous()
        return C.c_void_p(t.data_ptr())
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return C.c_void_p(t.ctypes.data)
    raise TypeError(type(t))


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class HipCodec:
    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise _lib.LlictiError(_lib.ENODEVICE, "no GPU visible to PyTorch-ROCm: the LLICTI hot path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.L = _lib.lib()
        ctx = C.c_void_p()
        _lib.check(self.L.llicti_create(C.byref(ctx), self.device.index))
        self.ctx = ctx
        self._ws = None
        self._ws_need = {}
        self._ws_grown = False
        self._mc = {}
        self.have_weights = False
        self.head, self.nlevels = 88, 5             # config A until set_model()

    def set_model(self, head, nlevels):
        """Model shape of the context (llicti_set_model): (88, 5) = config A, (60, 2) = config B.  A change drops the weights."""
        if (int(head), int(nlevels)) == (self.head, self.nlevels):
            return
        _lib.check(self.L.llicti_set_model(self.ctx, int(head), int(nlevels)))
        self.head, self.nlevels = int(head), int(nlevels)
        self.have_weights = False
        self._ws_need.clear()
        self._mc.clear()

    def close(self):
        if getattr(self, "ctx", None):
            self.L.llicti_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd):
        """Reference-keyed state_dict (or the canonical packed dict) -> device."""
        packed = sd if (isinstance(sd, dict) and 0 in sd) else pack_state_dict(sd)
        head = int(packed[0].get("head", 88))
        if head != self.head:
            raise ValueError(f"weights with {head}-wide heads for a context of {self.head}-wide ones: set_model({head}, {MODELS.get(head)}) first")
        for b in range(3):
            d = packed[b]
            _lib.check(self.L.llicti_set_band_weights(self.ctx, b, int(d["K0"]), _ptr(d["w0"]), _ptr(d["b0"]),
                                                      _ptr(d["w1"]), _ptr(d["b1"]), _ptr(d["w2"]), _ptr(d["b2"])))
        self.have_weights = True

    # ------------------------------------------------------------------ kernel-level wrappers
    def lift(self, rgb):
        B, _, H, W = rgb.shape
        planes = torch.empty((B, 3, H, W), dtype=torch.int16, device=self.device)
        fplanes = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        mm = torch.empty((B, 4), dtype=torch.int32, device=self.device)
        _lib.check(self.L.llicti_lift_u8(self.ctx, _ptr(rgb), B, H, W, _ptr(planes), _ptr(fplanes), _ptr(mm), _stream_ptr(self.device)))
        return planes, fplanes, mm

    def unlift(self, planes):
        B, _, H, W = planes.shape
        rgb = torch.empty((B, 3, H, W), dtype=torch.uint8, device=self.device)
        _lib.check(self.L.llicti_unlift_u8(self.ctx, _ptr(planes), B, H, W, _ptr(rgb), _stream_ptr(self.device)))
        return rgb

    def band_params(self, fplanes, lvl, band):
        B, _, H, W = fplanes.shape
        _, _, h, w, _, _, _, _ = _lib.level_geom(H, W, lvl, band)
        out = torch.empty((B, 64, h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.L.llicti_band_params_f32(self.ctx, _ptr(fplanes), B, H, W, lvl, band, _ptr(out), _stream_ptr(self.device)))
        return out                             # channel-planar: 4 heads x 16 planes (15 used; the 16th is never written); params60() gives the reference's 60 channels

    def lift_train(self, rgb):
        """uint8 [B,3,H,W] -> float32 [B,3,H,W] planes of the training path's float lift (Y - 127/255, Co, Cg)."""
        B, _, H, W = rgb.shape
        fplanes = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        _lib.check(self.L.llicti_lift_train_f32(self.ctx, _ptr(rgb), B, H, W, _ptr(fplanes), _stream_ptr(self.device)))
        return fplanes

    def selfinfo(self, fplanes, params, lvl, band):
        """-> float32 [B, 3, h, w]: -log2 pmf (bits) of the band's Y, Co, Cg targets."""
        B, _, H, W = fplanes.shape
        _, _, h, w, _, _, _, _ = _lib.level_geom(H, W, lvl, band)
        out = torch.empty((B, 3, h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.L.llicti_selfinfo_f32(self.ctx, _ptr(fplanes), _ptr(params), B, H, W, lvl, band, _ptr(out),
                                              _stream_ptr(self.device)))
        return out

    def forward_selfinfo(self, rgb):
        """LLICTI.forward: list of L tensors [B, 9, h, w] (L = 5 / 2 levels for config A / B; scale 0 first; channel 3*band + colour)."""
        fplanes = self.lift_train(rgb)
        res = []
        for lvl in range(self.nlevels):
            bands = [self.selfinfo(fplanes, self.band_params(fplanes, lvl, b), lvl, b) for b in range(3)]
            res.append(torch.cat(bands, dim=1))
        return res

    @staticmethod
    def params60(p64):
        """[B, 64, h, w] device layout (channel planes) -> [B, h, w, 60] in the reference's channel order (LLICTI_nets.py:381-387)."""
        B, _, h, w = p64.shape
        return p64.reshape(B, 4, 16, h, w)[:, :, :15].reshape(B, 60, h, w).permute(0, 2, 3, 1)

    def cdf_tables(self, planes, params, mm, lvl, band, clr, row_stride=512):
        B, _, H, W = planes.shape
        *_, hc, wc = _lib.level_geom(H, W, lvl, band)
        out = torch.empty((B, hc * wc, row_stride), dtype=torch.int16, device=self.device)
        _lib.check(self.L.llicti_cdf_u16(self.ctx, _ptr(planes), _ptr(params), _ptr(mm), B, H, W, lvl, band, clr,
                                         _ptr(out), row_stride, _stream_ptr(self.device)))
        return out

    def cdf_pairs(self, planes, params, mm, lvl, band):
        B, _, H, W = planes.shape
        *_, hc, wc = _lib.level_geom(H, W, lvl, band)
        out = torch.empty((3, B, hc * wc), dtype=torch.int32, device=self.device)
        _lib.check(self.L.llicti_cdf_pairs_u32(self.ctx, _ptr(planes), _ptr(params), _ptr(mm), B, H, W, lvl, band,
                                               _ptr(out), _stream_ptr(self.device)))
        return out

    def ac_encode(self, cdf, sym, Lp=None):
        """torchac seam: cdf int16/uint16 [S, N, stride] with Lp valid entries per row (default: stride), sym int16 [S, N]
        -> (streams uint8 [S, out_stride], lengths int32 [S])."""
        S, N, stride = cdf.shape
        Lp = stride if Lp is None else int(Lp)
        out_stride = (2 * N + 32 + 3) // 4 * 4      # slots are written 32 bits at a time
        out = torch.zeros((S, out_stride), dtype=torch.uint8, device=self.device)
        ln = torch.zeros((S,), dtype=torch.int32, device=self.device)
        _lib.check(self.L.llicti_ac_encode_u16cdf(self.ctx, _ptr(cdf), Lp, stride, _ptr(sym), S, N, _ptr(out), out_stride,
                                                  _ptr(ln), _stream_ptr(self.device)))
        _lib.check(self.L.llicti_check_status(self.ctx, _stream_ptr(self.device)))
        return out, ln

    def poison_workspace(self, value=0xA5):
        """Overwrite the cached workspace (tests / bench: a decode must not depend on what an earlier call left there)."""
        if self._ws is not None:
            self._ws.fill_(value)

    def ac_decode(self, cdf, Lp, streams, lens, N):
        S, _, stride = cdf.shape
        in_stride = streams.shape[1]
        sym = torch.empty((S, N), dtype=torch.int16, device=self.device)
        _lib.check(self.L.llicti_ac_decode_u16cdf(self.ctx, _ptr(cdf), int(Lp), stride, _ptr(streams), in_stride, _ptr(lens),
                                                  S, N, _ptr(sym), _stream_ptr(self.device)))
        return sym

    # ------------------------------------------------------------------ whole batch
    def _workspace_of(self, n):
        """The cached workspace, grown to the RUNNING MAXIMUM of what the calls needed (a data set of many image sizes must not
        re-allocate per call; the library validates the size it is given against what the call needs)."""
        if n == 0:
            _lib.check(_lib.EINVAL)
        if self._ws is None or self._ws.numel() < n:
            self._ws = None
            self._ws = torch.empty((int(n * 1.25) if self._ws_grown else n,), dtype=torch.uint8, device=self.device)
            self._ws_grown = True
        return self._ws

    def _ws_bytes(self, key, ask):
        """The workspace bytes of the call `key` names: remembered (the table is cleared at 256 entries), else ask()ed of the library."""
        n = self._ws_need.get(key)
        if n is None:
            if len(self._ws_need) > 256:
                self._ws_need.clear()
            n = self._ws_need[key] = int(ask())
        return n

    def workspace(self, B, H, W, mode=MODE_AC):
        def ask():
            Hs, Ws, m = (C.c_int * B)(*([H] * B)), (C.c_int * B)(*([W] * B)), (C.c_int * 1)(mode)
            return self.L.llicti_workspace_bytes_ctx(self.ctx, B, Hs, Ws, m, 1)      # (the context's model)
        return self._workspace_of(self._ws_bytes((B, H, W, mode), ask))

    @staticmethod
    def _modes_arg(mode, B):
        """mode: one int, or one per image -> (int or None, int32 array or None)"""
        if isinstance(mode, (int, np.integer)):
            return int(mode), None
        m = np.ascontiguousarray(mode, dtype=np.int32)
        assert m.shape == (B,)
        return (int(m[0]), None) if (m == m[0]).all() else (None, m)

    def workspace_v(self, Hs, Ws, mode):
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        one, per = self._modes_arg(mode, len(Hs))
        modes = np.array([one], dtype=np.int32) if per is None else per
        return self._workspace_of(self._ws_bytes((Hs.tobytes(), Ws.tobytes(), one if per is None else per.tobytes()), lambda: self.L.llicti_workspace_bytes_ctx(
            self.ctx, len(Hs), _ptr(Hs), _ptr(Ws), _ptr(modes), len(modes))))

    def max_container_bytes(self, H, W):
        n = self._mc.get((H, W))
        if n is None:
            n = int(self.L.llicti_max_container_bytes_ctx(self.ctx, H, W))
            if n == 0:
                _lib.check(_lib.EINVAL)
            if len(self._mc) > 1024:
                self._mc.clear()
            self._mc[(H, W)] = n
        return n

    def encode(self, rgb, mode=MODE_AC, out=None, seg_len=None):
        """rgb uint8 [B,3,H,W] on this device -> (containers uint8 [B, stride], seg_len int32 [B,49]), async."""
        assert rgb.dtype == torch.uint8 and rgb.is_cuda and rgb.dim() == 4 and rgb.shape[1] == 3
        rgb = rgb.contiguous()
        B, _, H, W = rgb.shape
        ws = self.workspace(B, H, W, mode)
        stride = self.max_container_bytes(H, W)
        if out is None:
            out = torch.empty((B, stride), dtype=torch.uint8, device=self.device)
        if seg_len is None:
            seg_len = torch.zeros((B, NSEG), dtype=torch.int32, device=self.device)
        _lib.check(self.L.llicti_encode_images(self.ctx, _ptr(rgb), B, H, W, mode, _ptr(ws), ws.numel(), _ptr(out), out.shape[1],
                                               _ptr(seg_len), _stream_ptr(self.device)))
        return out, seg_len

    def decode(self, containers, seg_len, H, W, mode=MODE_AC, out=None, reduce=0):
        """device containers -> uint8 [B,3,H,W], async.  reduce = r (0 .. the model's levels): uint8 [B,3,Hr,Wr] of reduced_dims(H, W, r) --
        exactly full[..., ::2**r, ::2**r], from the levels >= r alone (decode_reduced)."""
        B = containers.shape[0]
        if reduce:
            flat = self.decode_reduced(containers, seg_len, [H] * B, [W] * B, mode, reduce, out=None if out is None else out.view(-1))
            return out if out is not None else flat.view(B, 3, *reduced_dims(H, W, reduce))
        ws = self.workspace(B, H, W, mode)
        if out is None:
            out = torch.empty((B, 3, H, W), dtype=torch.uint8, device=self.device)
        _lib.check(self.L.llicti_decode_images(self.ctx, _ptr(containers), containers.shape[1], _ptr(seg_len), B, H, W, mode,
                                               _ptr(ws), ws.numel(), _ptr(out), _stream_ptr(self.device)))
        return out

    # ---- batches of mixed sizes (llicti_encode_images_v / llicti_decode_images_v): images tightly packed in one flat uint8 buffer
    @staticmethod
    def flat_offsets(Hs, Ws):
        """Byte offsets of the images' [3][H][W] blocks in the flat RGB buffer of a mixed-size batch (tightly packed), and its size."""
        sizes = 3 * np.asarray(Hs, dtype=np.int64) * np.asarray(Ws, dtype=np.int64)
        offs = np.concatenate(([0], np.cumsum(sizes)))
        return offs[:-1], int(offs[-1])

    def _containers_out(self, Hs, Ws, out, seg_len):
        """The output side of a call that writes containers for images of sizes Hs[b] x Ws[b]: the caller's tensors, or new ones of the widest
        container stride among the sizes -> (out uint8 [B, stride], seg_len int32 [B, 49], that stride)"""
        stride = max(self.max_container_bytes(int(h), int(w)) for h, w in set(zip(Hs.tolist(), Ws.tolist())))
        if out is None:
            out = torch.empty((len(Hs), stride), dtype=torch.uint8, device=self.device)
        if seg_len is None:
            seg_len = torch.zeros((len(Hs), NSEG), dtype=torch.int32, device=self.device)
        return out, seg_len, stride

    def _encode_front(self, Hs, Ws, mode, out, seg_len):
        """The front of the encode calls on mixed sizes: sizes as int32 arrays, the workspace, the outputs and the mode as one int (per None)
        or one per image (one None: stream counts may differ) -> (Hs, Ws, B, ws, out, seg_len, one, per)"""
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        ws = self.workspace_v(Hs, Ws, mode)
        out, seg_len, stride = self._containers_out(Hs, Ws, out, seg_len)
        assert out.shape[1] >= stride
        return (Hs, Ws, len(Hs), ws, out, seg_len) + self._modes_arg(mode, len(Hs))

    def encode_v(self, rgb_flat, Hs, Ws, mode, out=None, seg_len=None):
        """rgb_flat: uint8 device tensor holding B images of sizes Hs[b] x Ws[b] back to back ([3][H][W] each) -> (containers uint8
        [B, stride], seg_len int32 [B, 49]), async.  Image b's bytes are those of encode() on that image alone."""
        assert rgb_flat.dtype == torch.uint8 and rgb_flat.is_cuda and rgb_flat.dim() == 1 and rgb_flat.is_contiguous()
        assert rgb_flat.numel() >= self.flat_offsets(Hs, Ws)[1]
        Hs, Ws, B, ws, out, seg_len, one, per = self._encode_front(Hs, Ws, mode, out, seg_len)
        if per is None:                             # (one mode for the call; else llicti_encode_images_vm)
            _lib.check(self.L.llicti_encode_images_v(self.ctx, _ptr(rgb_flat), None, B, _ptr(Hs), _ptr(Ws), one, _ptr(ws), ws.numel(),
                                                     _ptr(out), out.shape[1], _ptr(seg_len), _stream_ptr(self.device)))
        else:
            _lib.check(self.L.llicti_encode_images_vm(self.ctx, _ptr(rgb_flat), None, B, _ptr(Hs), _ptr(Ws), _ptr(per), _ptr(ws), ws.numel(),
                                                      _ptr(out), out.shape[1], _ptr(seg_len), _stream_ptr(self.device)))
        return out, seg_len

    def _decode_prologue(self, name, containers, seg_len, Hs, Ws, mode, reduce, opts=None):
        """The front of the decode calls that take `reduce`: sizes as int32 arrays, the workspace, the modes array and the reduce argument
        -> (B, every image's decoded size, call), where call(*tail) runs llicti_<name> (reduce an int) or llicti_<name>_rv (one per image) on
        the leading arguments, `tail` and this device's stream.  opts (a _lib.TensorOpts): llicti_<name>_o instead -- B reduce values whatever
        `reduce` is, and `opts` behind the stream."""
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        B = len(Hs)
        assert containers.shape[0] == B
        ws = self.workspace_v(Hs, Ws, mode)          # (the full decode's: a reduced call uses the same layout)
        one, per = self._modes_arg(mode, B)
        modes = np.array([one], dtype=np.int32) if per is None else per
        r, rv = _reduce_arg(reduce, B)
        dims = _reduced_sizes(Hs, Ws, r, rv)
        end = ()
        if opts is not None:
            rv, end = (np.full(B, r, dtype=np.int32) if rv is None else rv), (C.byref(opts),)
        fn = getattr(self.L, "llicti_" + name + ("_o" if opts is not None else "" if rv is None else "_rv"))

        def call(*tail):
            _lib.check(fn(self.ctx, _ptr(containers), containers.shape[1], _ptr(seg_len), B, _ptr(Hs), _ptr(Ws), _ptr(modes), len(modes),
                          r if rv is None else _ptr(rv), _ptr(ws), ws.numel(), *tail, _stream_ptr(self.device), *end))
        return B, dims, call      # (a bad r: the library says so)

    def _tensor_out(self, out, n, size, dtype, channels_last=False):
        """the [n, 3, Ho, Wo] output of a tensor decode, the caller's (checked) or a new one -> (out, the library's dtype code, Ho, Wo).
        channels_last: the tensor is [n, 3, Ho, Wo] in torch.channels_last -- strides (3 Ho Wo, 1, 3 Wo, 3), held as strides (is_contiguous
        cannot tell the layouts apart when a dimension has size 1)."""
        Ho, Wo = int(size[0]), int(size[1])
        dt = TENSOR_DTYPES.get(dtype, dtype)          # (an int goes through as it is: the library says what it does not know)
        tdt = next((k for k, v in TENSOR_DTYPES.items() if v == dt), torch.float32)
        if not channels_last:
            if out is None:
                out = torch.empty((n, 3, max(Ho, 0), max(Wo, 0)), dtype=tdt, device=self.device)
            assert out.is_cuda and out.is_contiguous() and out.dtype == tdt and out.numel() >= n * 3 * Ho * Wo
            return out, int(dt), Ho, Wo
        if out is None:
            out = torch.empty((n, 3, max(Ho, 0), max(Wo, 0)), dtype=tdt, device=self.device, memory_format=torch.channels_last)
        assert out.is_cuda and out.dtype == tdt and tuple(out.shape) == (n, 3, max(Ho, 0), max(Wo, 0)), "out: a [n, 3, Ho, Wo] device tensor of the call's dtype"
        if Ho >= 1 and Wo >= 1:                       # (a size the library will refuse: it says so)
            assert tuple(out.stride()) == (3 * Ho * Wo, 1, 3 * Wo, 3), f"out: strides {tuple(out.stride())}, channels_last needs {(3 * Ho * Wo, 1, 3 * Wo, 3)}"
        return out, int(dt), Ho, Wo

    def decode_reduced(self, containers, seg_len, Hs, Ws, mode, reduce, out=None, rgb_off=None):
        """llicti_decode_images_reduced: device containers of B images of FULL sizes Hs[b] x Ws[b] (mode: one, or one per image) -> flat uint8
        device tensor holding image b's [3][Hr][Wr] block (reduced_dims) at byte rgb_off[b], or back to back (rgb_off None), async.  Only the
        stages of levels >= reduce are launched; a rANS container's end-of-stream check (the last stage's tail coder) is therefore not run for
        reduce >= 1: check() / image_status() report what the launched kernels flag.  reduce = 0 is decode_v.
        reduce may be a sequence of B ints (llicti_decode_images_reduced_rv): image b stops at its own level reduce[b] and is exactly what the
        call at that one value gives for it -- size, bytes, status word; level l runs for the images with reduce[b] <= l alone."""
        B, dims, call = self._decode_prologue("decode_images_reduced", containers, seg_len, Hs, Ws, mode, reduce)
        sizes = [3 * h * w for h, w in dims]
        if rgb_off is None:
            offs, total = None, sum(sizes)
        else:
            offs = np.ascontiguousarray(rgb_off, dtype=np.uint64)
            assert offs.shape == (B,)
            total = max(int(o) + n for o, n in zip(offs, sizes))
        if out is None:
            out = torch.empty((total,), dtype=torch.uint8, device=self.device)
        assert out.numel() >= total
        call(_ptr(out), _ptr(offs))
        return out

    # ---- interleaved, pitched pixels (llicti_encode_images_px / llicti_decode_images_px): the layout image sources deliver
    def _px_layout(self, fmt, dims, px_off, pitch):
        """-> (format, offsets or None, pitches or None, bytes the windows reach into the buffer)"""
        fmt = pixel_format(fmt)
        bpp = pixel_bytes(fmt)
        B = len(dims)
        pt = None if pitch is None else np.ascontiguousarray(pitch, dtype=np.uint64)
        offs = None if px_off is None else np.ascontiguousarray(px_off, dtype=np.uint64)
        assert (pt is None or pt.shape == (B,)) and (offs is None or offs.shape == (B,))
        # (a pitch the library will refuse counts as tight here: the call below reports it)
        spans = [(h - 1) * max(int(pt[b]) if pt is not None else 0, w * bpp) + w * bpp for b, (h, w) in enumerate(dims)]
        total = sum(spans) if offs is None else max(int(o) + n for o, n in zip(offs, spans))
        return fmt, offs, pt, total

    def encode_px(self, pix, Hs, Ws, mode, fmt=PIX_RGB8, px_off=None, pitch=None, out=None, seg_len=None):
        """pix: flat uint8 device tensor of INTERLEAVED pixels (fmt: "rgb" | "bgr" | "rgba" | "bgra" or PIX_*); image b's Hs[b] x Ws[b] window
        starts at byte px_off[b] with rows pitch[b] bytes apart (None: tight rows / the windows back to back), so a window may be a crop of a
        larger frame -> (containers, seg_len) as encode_v: the bytes of the planar call on the same pixel values.  Alpha is ignored.  Async."""
        assert pix.dtype == torch.uint8 and pix.is_cuda and pix.dim() == 1 and pix.is_contiguous()
        Hs, Ws, B, ws, out, seg_len, one, per = self._encode_front(Hs, Ws, mode, out, seg_len)
        fmt, offs, pt, total = self._px_layout(fmt, list(zip(Hs.tolist(), Ws.tolist())), px_off, pitch)
        assert pix.numel() >= total
        modes = np.full(B, one, dtype=np.int32) if per is None else per
        _lib.check(self.L.llicti_encode_images_px(self.ctx, _ptr(pix), fmt, _ptr(offs), _ptr(pt), B, _ptr(Hs), _ptr(Ws), _ptr(modes),
                                                  _ptr(ws), ws.numel(), _ptr(out), out.shape[1], _ptr(seg_len), _stream_ptr(self.device)))
        return out, seg_len

    def decode_px(self, containers, seg_len, Hs, Ws, mode, fmt=PIX_RGB8, reduce=0, out=None, px_off=None, pitch=None):
        """device containers of B images of FULL sizes Hs[b] x Ws[b] -> flat uint8 device tensor of interleaved pixels: image b's window (of
        reduced_dims(Hs[b], Ws[b], reduce)) at byte px_off[b] with rows pitch[b] bytes apart (None: back to back / tight).  Only the bytes of
        the windows' rows are written -- `out` may be a canvas whose other bytes must stay; alpha is written as 255.  reduce as decode_reduced
        (an int, or one per image: image b's window then has reduced_dims(Hs[b], Ws[b], reduce[b])).  Async."""
        B, dims, call = self._decode_prologue("decode_images_px", containers, seg_len, Hs, Ws, mode, reduce)
        fmt, offs, pt, total = self._px_layout(fmt, dims, px_off, pitch)
        if out is None:
            out = torch.empty((total,), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.dim() == 1 and out.numel() >= total
        call(_ptr(out), fmt, _ptr(offs), _ptr(pt))
        return out

    def decode_v(self, containers, seg_len, Hs, Ws, mode, out=None, reduce=0):
        """device containers of B images of sizes Hs[b] x Ws[b] -> flat uint8 device tensor (the images back to back), async.
        reduce = r: the images at reduced_dims(Hs[b], Ws[b], r), back to back (decode_reduced); one r per image: each at its own size."""
        if not isinstance(reduce, (int, np.integer)) or reduce:
            return self.decode_reduced(containers, seg_len, Hs, Ws, mode, reduce, out=out)
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        B = len(Hs)
        assert containers.shape[0] == B
        ws = self.workspace_v(Hs, Ws, mode)
        total = self.flat_offsets(Hs, Ws)[1]
        if out is None:
            out = torch.empty((total,), dtype=torch.uint8, device=self.device)
        assert out.numel() >= total
        one, per = self._modes_arg(mode, B)
        if per is None:
            _lib.check(self.L.llicti_decode_images_v(self.ctx, _ptr(containers), containers.shape[1], _ptr(seg_len), B, _ptr(Hs), _ptr(Ws), one,
                                                     _ptr(ws), ws.numel(), _ptr(out), None, _stream_ptr(self.device)))
        else:
            _lib.check(self.L.llicti_decode_images_vm(self.ctx, _ptr(containers), containers.shape[1], _ptr(seg_len), B, _ptr(Hs), _ptr(Ws), _ptr(per),
                                                      _ptr(ws), ws.numel(), _ptr(out), None, _stream_ptr(self.device)))
        return out

    # ---- float tensors (llicti_decode_images_tensor / llicti_encode_images_f32): the batch tensor a network is fed with, planar float32 in
    def decode_tensor(self, containers, seg_len, Hs, Ws, mode, size, dtype=torch.float32, origin=None, flip=None, mean=None, std=None, reduce=0, out=None,
                      channels_last=False, pad=None):
        """device containers of B images of FULL sizes Hs[b] x Ws[b] (they may differ) -> ONE device tensor [B, 3, Ho, Wo] of `dtype` (float32,
        float16, bfloat16), written by the decode's last kernel, async.  size = (Ho, Wo); origin = (y0s, x0s): every image's window origin in the
        decoded image (the reduced one for reduce >= 1; None: 0) -- the window must lie inside the image, nothing is padded or resampled;
        flip: B flags, a set one mirrors that window left to right; mean, std: 3 floats each (both or neither).  The values are those of
        torchvision's ToTensor + Normalize on the CPU, bit for bit: v / 255 (one fp32 division), then (x - mean[c]) / std[c], then dtype's
        round-to-nearest-even.  Origins and flips are per-call data: calls that differ only in them share one cached plan.  `out`: a contiguous
        [B, 3, Ho, Wo] tensor of that dtype to write into (nothing outside it is touched).  reduce as decode_reduced (an int, or one per image:
        image b's origin is then in the coordinates of its own decimated grid).
        channels_last=True: the same values as a [B, 3, Ho, Wo] tensor in torch.channels_last (strides (3 Ho Wo, 1, 3 Wo, 3); a caller's `out`
        must have exactly those), interleaved by the same kernel -- no transpose pass.  pad=dict(mode="constant" | "edge" | "reflect" |
        "symmetric", fill=0 or 3 values, space="pixel" | "output"): a window may leave its image, origins may be negative (-8160 .. 8160) --
        numpy's pad modes of those names (torch's "replicate" is "edge"); "reflect" mirrors at most n - 1 pixels past a side of n, "symmetric"
        n.  fill in space "pixel" is a value on the 0 .. 255 scale that is normalised like a pixel (torchvision's Pad(fill) in front of ToTensor +
        Normalize), in space "output" the element itself (0: the padded zeros of a collate).  center_crop_origins gives CenterCrop's windows.
        With neither, the call is the one it always was; with either, the plan, its key and the counters are still decode_reduced's."""
        opts = _tensor_opts(channels_last, pad)
        B, _, call = self._decode_prologue("decode_images_tensor", containers, seg_len, Hs, Ws, mode, reduce, opts)
        out, dt, Ho, Wo = self._tensor_out(out, B, size, dtype, channels_last)
        y0 = x0 = None
        if origin is not None:
            y0, x0 = (np.ascontiguousarray(v, dtype=np.int32) for v in origin)
            assert y0.shape == (B,) and x0.shape == (B,)
        fl = _flip_arg(flip, B)
        mn, sd = _norm_args(mean, std)
        call(C.c_void_p(out.data_ptr()), dt, Ho, Wo, _ptr(y0), _ptr(x0), _ptr(fl), _ptr(mn), _ptr(sd))
        return out

    def decode_tensor_resized(self, containers, seg_len, Hs, Ws, mode, size, boxes, dtype=torch.float32, flip=None, mean=None, std=None, antialias=True,
                              reduce=0, out=None, channels_last=False):
        """decode_tensor with a resampling step (llicti_decode_images_tensor_resized): image b's source box boxes[b] = (y0, x0, hs, ws) -- in the
        coordinates of the decoded image, the reduced one for reduce >= 1; boxes None: every whole image -- is resampled to size = (Ho, Wo) by
        the decode's last kernel, flipped, normalised and written into ONE device tensor [B, 3, Ho, Wo] of `dtype`, async: torchvision's
        RandomResizedCrop + flip + ToTensor + Normalize on a batch of mixed sizes.  The filter is F.interpolate's bilinear one
        (align_corners=False); antialias=True widens it by the scale when a box shrinks, up to a scale of 4 per axis -- beyond that raise
        `reduce` (resized_crop_plan picks it).  A box of Ho x Wo gives decode_tensor's bytes.  Boxes, flips, size and flag are per-call data:
        calls that differ only in them share decode_reduced's cached plan and neither allocate nor synchronise.  reduce: an int, or one per image
        (resized_crop_plan(..., per_image=True)): box b is then in the coordinates of image b's own decimated grid, and a tight crop no longer
        sends its neighbours through the finest levels.  channels_last as decode_tensor's (a box that leaves its image stays refused)."""
        B, _, call = self._decode_prologue("decode_images_tensor_resized", containers, seg_len, Hs, Ws, mode, reduce, _tensor_opts(channels_last, None))
        out, dt, Ho, Wo = self._tensor_out(out, B, size, dtype, channels_last)
        cols = _box_columns(boxes, B)
        fl = _flip_arg(flip, B)
        mn, sd = _norm_args(mean, std)
        aa = int(antialias) if isinstance(antialias, (bool, int, np.integer)) else -1
        call(C.c_void_p(out.data_ptr()), dt, Ho, Wo, *(_ptr(c) for c in cols), _ptr(fl), _ptr(mn), _ptr(sd), aa)
        return out

    def decode_tensor_views(self, containers, seg_len, Hs, Ws, mode, groups, mean=None, std=None, reduce=0, channels_last=False):
        """Several resized crops per image from ONE decode (llicti_decode_images_tensor_views).  groups: a list of dict(size=(Ho, Wo),
        image=[...] | None, boxes=[(y0, x0, hs, ws), ...] | None, flip=None, dtype=torch.float32, antialias=True, out=None): view v of a
        group is what decode_tensor_resized writes for image image[v] (any order, repeats allowed, images may be absent; None: view v is
        image v) with box boxes[v] (decoded coordinates, the reduced ones for reduce >= 1; None: the whole image), to the bit.  -> a list
        of one device tensor [n, 3, Ho, Wo] per group, async.  Outputs of different groups must not overlap.  The batch is decoded once;
        every view costs one more pass of the last kernel.  Image indices, boxes and flips are per-call data: calls that differ only in
        them share decode_reduced's cached plan and neither allocate nor synchronise.  multi_crop_plan picks reduce: an int, or one per image
        (per_image=True) -- a view's box is then in the coordinates of ITS image's decimated grid, and an image no view names may be passed at
        the model's level count.  channels_last as decode_tensor's: it holds for EVERY group of the call."""
        B, _, call = self._decode_prologue("decode_images_tensor_views", containers, seg_len, Hs, Ws, mode, reduce, _tensor_opts(channels_last, None))
        groups = list(groups)
        arr = (_lib.ViewGroup * max(len(groups), 1))()
        outs, keep = [], []
        for g, spec in enumerate(groups):
            spec = dict(spec)
            Ho, Wo = (int(v) for v in spec.pop("size"))
            image, boxes, flip, out = spec.pop("image", None), spec.pop("boxes", None), spec.pop("flip", None), spec.pop("out", None)
            dtype, antialias = spec.pop("dtype", torch.float32), spec.pop("antialias", True)
            if spec:
                raise TypeError(f"group {g}: unknown keys {sorted(spec)}")
            img = None if image is None else np.ascontiguousarray(image, dtype=np.int32)
            assert img is None or img.ndim == 1
            n = B if img is None else len(img)
            out, dt, Ho, Wo = self._tensor_out(out, n, (Ho, Wo), dtype, channels_last)
            cols = _box_columns(boxes, n)
            fl = _flip_arg(flip, n)
            aa = int(antialias) if isinstance(antialias, (bool, int, np.integer)) else -1
            keep.append((img, cols, fl))                  # (the host arrays live until the call returns)
            vg = arr[g]
            vg.d_out, vg.dtype, vg.Ho, vg.Wo, vg.antialias, vg.n = out.data_ptr(), dt, Ho, Wo, aa, n
            vg.image, vg.flip = _ptr(img), _ptr(fl)
            vg.y0, vg.x0, vg.hs, vg.ws = (_ptr(c) for c in cols)
            outs.append(out)
        mn, sd = _norm_args(mean, std)
        call(arr, len(groups), _ptr(mn), _ptr(sd))
        return outs

    def encode_f32(self, x_flat, Hs, Ws, mode, x_off=None, out=None, seg_len=None):
        """encode_v on planar float32: x_flat is a flat float32 device tensor holding image b's [3][Hs[b]][Ws[b]] block at ELEMENT x_off[b] (None:
        back to back) -> (containers, seg_len), async.  A sample x is the pixel round(x * 255) (half to even, as torch.round), clamped to
        0 .. 255, NaN -> 0; the bytes are those of encode_v on these pixel values."""
        assert x_flat.dtype == torch.float32 and x_flat.is_cuda and x_flat.dim() == 1 and x_flat.is_contiguous()
        Hs, Ws, B, ws, out, seg_len, one, per = self._encode_front(Hs, Ws, mode, out, seg_len)
        sizes = 3 * Hs.astype(np.int64) * Ws.astype(np.int64)
        offs = None if x_off is None else np.ascontiguousarray(x_off, dtype=np.uint64)
        assert offs is None or offs.shape == (B,)
        assert x_flat.numel() >= (int(sizes.sum()) if offs is None else max(int(o) + int(n) for o, n in zip(offs, sizes)))
        modes = np.full(B, one, dtype=np.int32) if per is None else per
        _lib.check(self.L.llicti_encode_images_f32(self.ctx, _ptr(x_flat), _ptr(offs), B, _ptr(Hs), _ptr(Ws), _ptr(modes), _ptr(ws), ws.numel(),
                                                   _ptr(out), out.shape[1], _ptr(seg_len), _stream_ptr(self.device)))
        return out, seg_len

    # ---- transcode (llicti_transcode_images): containers of one kind into containers of another at the cost of one decode
    def transcode_workspace(self, Hs, Ws, src_mode, dst_mode):
        """(the cached workspace, grown to the running maximum like the other workspaces, for a transcode of these sizes and modes --
        llicti_transcode_workspace_bytes: the source call's layout followed by the target's --, [source modes, target modes] as the int32
        arrays the C-ABI takes: one entry, or one per image)"""
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        B = len(Hs)
        sides = []
        for mode in (src_mode, dst_mode):
            one, per = self._modes_arg(mode, B)
            sides.append(np.array([one], dtype=np.int32) if per is None else per)
        n = self._ws_bytes(("transcode", Hs.tobytes(), Ws.tobytes(), sides[0].tobytes(), sides[1].tobytes()), lambda: self.L.llicti_transcode_workspace_bytes(
            self.ctx, B, _ptr(Hs), _ptr(Ws), _ptr(sides[0]), len(sides[0]), _ptr(sides[1]), len(sides[1])))
        if n == 0:
            raise _lib.LlictiError(_lib.EINVAL, "transcode: a combination of sizes and container modes the call refuses (an \"auto\" source, mixed lane kinds, "
                                                "the reference format with images of different sizes, a mode the model does not take)")
        return self._workspace_of(n), sides

    def transcode(self, containers, seg_len, Hs, Ws, src_mode, dst_mode, out=None, seg_len_out=None):
        """device containers of B images of sizes Hs[b] x Ws[b] in src_mode (one mode or one per image: what container_modes() / mode_of_header say)
        -> (containers uint8 [B, stride], seg_len int32 [B, 49]) in dst_mode (one or one per image, MODE_RANS_AUTO included), async: image b's
        bytes are those of encode() of its pixels in dst_mode[b], made from ONE pass of the band CNN and without the pixels.  Status as after a
        decode: check() / image_status(); a flagged image's seg_len row is zeros."""
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        B = len(Hs)
        assert containers.dtype == torch.uint8 and containers.is_cuda and containers.dim() == 2 and containers.shape[0] == B and containers.is_contiguous()
        ws, (src, dst) = self.transcode_workspace(Hs, Ws, src_mode, dst_mode)
        out, seg_len_out, _ = self._containers_out(Hs, Ws, out, seg_len_out)
        _lib.check(self.L.llicti_transcode_images(self.ctx, _ptr(containers), containers.shape[1], _ptr(seg_len), B, _ptr(Hs), _ptr(Ws),
                                                  _ptr(src), len(src), _ptr(dst), len(dst), _ptr(ws), ws.numel(),
                                                  _ptr(out), out.shape[1], _ptr(seg_len_out), _stream_ptr(self.device)))
        return out, seg_len_out

    # ---- records (llicti_pack_records / llicti_unpack_records): the strided containers of a batch <-> one dense blob of .llic records
    @property
    def nseg(self):
        """Segments per container of the context's model: 4 + 9 x levels (49 config A, 22 config B) -- the `n` of a .llic record."""
        return 4 + 9 * self.nlevels

    def record_bytes(self, seg_len):
        """Bytes of the .llic record of one image from its segment lengths (host array; llicti_record_bytes, works without a device call):
        6 + 4n + sum, 0 for a negative length."""
        sl = np.ascontiguousarray(seg_len, dtype=np.int32)
        assert sl.ndim == 1 and sl.size >= self.nseg
        return int(self.L.llicti_record_bytes(self.ctx, _ptr(sl)))

    def _record_containers(self, containers, seg_len):
        """The container side of a record call, checked: device containers uint8 [B, .] whose rows may be strided (one row: its length is the
        stride) and their seg_len int32 [B, 49] -> (B, the row stride in bytes)"""
        assert containers.dtype == torch.uint8 and containers.is_cuda and containers.dim() == 2 and containers.stride(1) == 1
        B = int(containers.shape[0])
        stride = int(containers.stride(0)) if B > 1 else int(containers.shape[1])
        assert seg_len.dtype == torch.int32 and seg_len.is_cuda and tuple(seg_len.shape) == (B, NSEG) and seg_len.is_contiguous()
        return B, stride

    def _pack_out(self, B, worst, out, rec_off):
        """The blob side of a pack: the caller's blob and offsets, checked, or new ones (the blob of `worst` bytes) -> (out, rec_off)"""
        if out is None:
            out = torch.empty((worst,), dtype=torch.uint8, device=self.device)
        if rec_off is None:
            rec_off = torch.empty((B + 1,), dtype=torch.int64, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.dim() == 1 and out.stride(0) == 1
        assert rec_off.dtype == torch.int64 and rec_off.is_cuda and rec_off.numel() == B + 1 and rec_off.is_contiguous()
        return out, rec_off

    def _unpack_front(self, blob, rec_off, stride, out, seg_len):
        """The blob side of an unpack: the blob checked, rec_off (a host array / tensor, or a device tensor) on the device, and the containers
        to write -- the caller's, or new ones of `stride` bytes a row (None: the tight stride of HOST offsets) -- with their seg_len ->
        (ro_d, B, out, its row stride, seg_len)"""
        assert blob.dtype == torch.uint8 and blob.is_cuda and blob.dim() == 1 and blob.stride(0) == 1
        if isinstance(rec_off, torch.Tensor) and rec_off.is_cuda:
            ro_h, ro_d = None, rec_off
        else:
            ro_h = np.ascontiguousarray(rec_off.numpy() if isinstance(rec_off, torch.Tensor) else rec_off, dtype=np.int64)
            ro_d = torch.from_numpy(ro_h).to(self.device, non_blocking=True)
        assert ro_d.dtype == torch.int64 and ro_d.dim() == 1 and ro_d.numel() >= 2 and ro_d.is_contiguous()
        B = ro_d.numel() - 1
        if out is None:
            out = torch.empty((B, int(self.tight_stride(ro_h, self.nseg) if stride is None else stride)), dtype=torch.uint8, device=self.device)
        if seg_len is None:
            seg_len = torch.empty((B, NSEG), dtype=torch.int32, device=self.device)
        assert out.shape[0] == B
        return (ro_d, B, out, self._record_containers(out, seg_len)[1], seg_len)

    def pack_records(self, containers, seg_len, out=None, rec_off=None):
        """device containers uint8 [B, stride] + seg_len int32 [B, 49] -> (blob, rec_off): the images' .llic records back to back from blob[0]
        (flat uint8 device tensor) and their offsets, int64 device tensor [B + 1] -- rec_off[b] the first byte of record b, rec_off[B] the
        total, from a scan on the device.  Async: neither the sizes nor the total come to the host here (rec_off.cpu() when they are needed).
        blob[:rec_off[B]] equals b"".join(dumps_llic(...)) of the same containers; nothing at or past rec_off[B] is written.  out: the blob to
        write into (its numel is the capacity; None: the worst case, B x (header + stride)); a total above the capacity makes check() raise
        ENOSPACE with rec_off[B] = the capacity needed.  An image whose seg_len row is unusable (a negative entry, a sum above stride) gets a
        zero-length record and EFORMAT in image_status()."""
        B, stride = self._record_containers(containers, seg_len)
        assert stride >= containers.shape[1]
        out, rec_off = self._pack_out(B, B * (6 + 4 * self.nseg + int(containers.shape[1])), out, rec_off)
        _lib.check(self.L.llicti_pack_records(self.ctx, C.c_void_p(containers.data_ptr()), stride, _ptr(seg_len), B,
                                              C.c_void_p(out.data_ptr()), out.numel(), _ptr(rec_off), _stream_ptr(self.device)))
        return out, rec_off

    @staticmethod
    def tight_stride(rec_off, nseg):
        """The default stride of unpack_records from HOST offsets: the largest payload, rounded up to 16 (at least 16)."""
        ro = np.asarray(rec_off, dtype=np.int64)
        pay = int((np.diff(ro) - (6 + 4 * int(nseg))).max()) if ro.size > 1 else 0
        return max(16, (pay + 15) // 16 * 16)

    def unpack_records(self, blob, rec_off, stride=None, out=None, seg_len=None):
        """blob (flat uint8 device tensor) + rec_off ([B + 1] int64 offsets of B records in it: a host array / tensor, or a device tensor) ->
        (containers uint8 [B, stride], seg_len int32 [B, 49]) on the device, async: what the decode calls take.  Every record is validated on
        the device before a payload byte is read; one that fails gives an all-zero seg_len row, EFORMAT in image_status() (and check()), and
        leaves its container untouched -- a decode behind it refuses that image the same way.  stride=None: the largest payload rounded up to
        16, from rec_off when that is on the host; with device offsets the caller gives it (the decoders need no more than the payloads)."""
        if stride is None and out is None and isinstance(rec_off, torch.Tensor) and rec_off.is_cuda:
            raise ValueError("unpack_records: with rec_off on the device the caller gives stride (or out)")
        ro_d, B, out, cstride, seg_len = self._unpack_front(blob, rec_off, stride, out, seg_len)
        _lib.check(self.L.llicti_unpack_records(self.ctx, C.c_void_p(blob.data_ptr()), blob.numel(), _ptr(ro_d), B,
                                                C.c_void_p(out.data_ptr()), cstride, _ptr(seg_len), _stream_ptr(self.device)))
        return out, seg_len

    # ---- progressive records (llicti_level_cuts / llicti_pack_progressive / llicti_unpack_progressive): the same bytes level-major, so that a
    # decode at reduce = r needs a prefix of the record alone (llicti_amd/progressive.py states the format)
    def level_cuts(self, containers, seg_len, Hs, Ws, mode, out=None):
        """device xwide v4 containers of B images (mode: one, or one per image -- what container_modes gives) -> int32 device tensor
        [B, 128, 5]: entry [b, m, l] the byte of stream m at which the main coder's cursor stands behind level l (l >= 1; row m >= the image's
        stream count and l = 0: zero).  A full decode without pixels, async; check() / image_status() are a full decode's."""
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        B = len(Hs)
        assert containers.shape[0] == B and containers.dtype == torch.uint8 and containers.is_cuda
        ws = self.workspace_v(Hs, Ws, mode)
        modes = np.ascontiguousarray(np.broadcast_to(np.asarray(mode, dtype=np.int32), (B,)))
        if out is None:
            out = torch.empty((B, PROG_MAX_STREAMS, NLEVELS_MAX), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_cuda and tuple(out.shape) == (B, PROG_MAX_STREAMS, NLEVELS_MAX) and out.is_contiguous()
        cstride = int(containers.stride(0)) if B > 1 else int(containers.shape[1])
        _lib.check(self.L.llicti_level_cuts(self.ctx, C.c_void_p(containers.data_ptr()), cstride, _ptr(seg_len), B, _ptr(Hs), _ptr(Ws), _ptr(modes),
                                            _ptr(ws), ws.numel(), _ptr(out), _stream_ptr(self.device)))
        return out

    def pack_progressive(self, containers, seg_len, cuts, out=None, rec_off=None, prefix=None):
        """device containers + seg_len + level_cuts' table -> (blob, rec_off, prefix): the images' progressive records back to back from
        blob[0], their offsets (int64 [B + 1]) and every image's prefix lengths P_0 .. P_L (int64 [B, 6]; entries above the model's L: 0), all
        on the device, async.  pack_records' contract: out's numel is the capacity (None: the worst case), ENOSPACE / EFORMAT as there; an
        image whose header, lengths, length tables or cuts do not hold together gets a zero-length record."""
        B, stride = self._record_containers(containers, seg_len)
        assert cuts.dtype == torch.int32 and cuts.is_cuda and tuple(cuts.shape) == (B, PROG_MAX_STREAMS, NLEVELS_MAX) and cuts.is_contiguous()
        out, rec_off = self._pack_out(B, B * (12 + 4 * self.nseg + 4 * PROG_MAX_STREAMS * (self.nlevels + 1) + int(containers.shape[1])), out, rec_off)
        if prefix is None:
            prefix = torch.empty((B, NLEVELS_MAX + 1), dtype=torch.int64, device=self.device)
        assert prefix.dtype == torch.int64 and prefix.is_cuda and tuple(prefix.shape) == (B, NLEVELS_MAX + 1) and prefix.is_contiguous()
        _lib.check(self.L.llicti_pack_progressive(self.ctx, C.c_void_p(containers.data_ptr()), stride, _ptr(seg_len), B, _ptr(cuts),
                                                  C.c_void_p(out.data_ptr()), out.numel(), _ptr(rec_off), _ptr(prefix), _stream_ptr(self.device)))
        return out, rec_off, prefix

    def unpack_progressive(self, blob, rec_off, reduce=0, stride=None, out=None, seg_len=None):
        """blob (flat uint8 device tensor) + rec_off ([B + 1] int64 offsets: record b is blob[rec_off[b]:rec_off[b + 1]], the prefix P_{r_b} of a
        progressive record or anything longer) + reduce (one int, or one per image) -> (containers uint8 [B, stride], seg_len int32 [B, 49]),
        async: the frame bytes and the pieces of the levels >= r_b at their places, every other byte of `out` as it was.  Everything is
        validated on the device first; a refused record gives EFORMAT, a zero seg_len row and an untouched container.  out=None: a new,
        uninitialised tensor as unpack_records makes -- but for the images with r_b = L, whose rows are filled with 0x80: the decoders parse the
        top of every stream whatever the reduce, a zero there is an EFORMAT, and at r_b < L that top is among the delivered bytes; stride as
        unpack_records -- with no `out` the caller gives it: a prefix does not say how long the payload is."""
        fresh = out is None
        if fresh and stride is None:
            raise ValueError("unpack_progressive: the caller gives stride (or out)")
        ro_d, B, out, cstride, seg_len = self._unpack_front(blob, rec_off, stride, out, seg_len)
        if fresh:
            for b, r in enumerate(np.broadcast_to(np.asarray(reduce), (B,))):
                if int(r) >= self.nlevels:           # (no stream byte is delivered: the one case in which old bytes meet the decoders' parser)
                    out[b].fill_(0x80)
        red = np.ascontiguousarray(np.broadcast_to(np.asarray(reduce, dtype=np.int32), (B,)))
        _lib.check(self.L.llicti_unpack_progressive(self.ctx, C.c_void_p(blob.data_ptr()), blob.numel(), _ptr(ro_d), B, _ptr(red),
                                                    C.c_void_p(out.data_ptr()), cstride, _ptr(seg_len), _stream_ptr(self.device)))
        return out, seg_len

    def container_modes(self, containers):
        """The modes the headers of device containers [B, stride] name (a small download: 17 bytes per image; synchronises the current stream) --
        what decode() / decode_v() take for containers that came out of an "auto" encode (MODE_RANS_AUTO: the encoder picked the stream counts)."""
        hdr = containers[:, :17].contiguous().cpu().numpy()
        return [mode_of_header(hdr[b]) for b in range(hdr.shape[0])]

    def check(self):
        _lib.check(self.L.llicti_check_status(self.ctx, _stream_ptr(self.device)))

    def image_status(self, B):
        """Per-image status of the last decode: numpy int32 [B], 0 = ok, EFORMAT = that image's container was malformed."""
        out = np.zeros(B, dtype=np.int32)
        _lib.check(self.L.llicti_image_status(self.ctx, _ptr(out), B, _stream_ptr(self.device)))
        return out

    def set_tuning(self, key, value):
        _lib.check(self.L.llicti_set_tuning(self.ctx, key.encode(), int(value)))

    def encoded_fplanes(self, B, H, W, mode):
        """float32 [B,3,H,W] = (YCoCg-R - [127,0,0]) / 255 of the batch the LAST encode() / decode() of this shape and mode worked on, copied out of
        the workspace (llicti_workspace_planes): the `x_ycocg` of the reference's compress() without a second lift.  Enqueued on the
        current stream, behind that call."""
        o16, o32 = C.c_size_t(), C.c_size_t()
        _lib.check(self.L.llicti_workspace_planes(self.ctx, B, H, W, mode, C.byref(o16), C.byref(o32)))
        n = B * 3 * H * W * 4
        return self._ws[o32.value:o32.value + n].view(torch.float32).view(B, 3, H, W).clone()

    def last_params_v(self, Hs, Ws, mode, image):
        """float32 [64, h*w] CNN outputs of level 0, band x10 -- the LAST band-CNN launch -- of image `image` of the last encode_v() / decode_v() on
        images of these sizes in `mode` (one, or one per image), copied out of the workspace (llicti_workspace_params_v); params60() of its [1, 64, h, w]
        view gives the reference's 60 channels."""
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        one, per = self._modes_arg(mode, len(Hs))
        modes = np.full(len(Hs), one, dtype=np.int32) if per is None else per
        off, npos = C.c_size_t(), C.c_long()
        _lib.check(self.L.llicti_workspace_params_v(self.ctx, len(Hs), _ptr(Hs), _ptr(Ws), _ptr(modes), int(image), C.byref(off), C.byref(npos)))
        n = 64 * npos.value * 4
        return self._ws[off.value:off.value + n].view(torch.float32).view(64, npos.value).clone()

    # ---- pixel digests (llicti_crc32_planes / llicti_digest_images): zlib's CRC-32 of every image's planar uint8 [3][H][W] bytes, on the device
    @staticmethod
    def _crc_i64(crc32):
        """the kernels' uint32 words (held in an int32 tensor) as int64 values 0 .. 2^32 - 1"""
        return crc32.to(torch.int64) & 0xFFFFFFFF

    def crc32_planes(self, planes):
        """int16 device planes [B, 3, H, W] (lift's) -> int64 device tensor [B]: zlib.crc32 of each image's RGB bytes as uint8 [3][H][W], async."""
        assert planes.dtype == torch.int16 and planes.is_cuda and planes.dim() == 4 and planes.shape[1] == 3 and planes.is_contiguous()
        B, _, H, W = planes.shape
        crc = torch.empty((B,), dtype=torch.int32, device=self.device)
        _lib.check(self.L.llicti_crc32_planes(self.ctx, _ptr(planes), B, H, W, _ptr(crc), _stream_ptr(self.device)))
        return self._crc_i64(crc)

    def digests(self, Hs, Ws, mode, reduce=None):
        """The digests of the images of the PRECEDING whole-batch encode or decode of this batch (sizes Hs[b] x Ws[b], mode as that call took it:
        one, or one per image), out of the cached workspace that call ran in -> (crc, have): int64 device tensor [B] holding 0 .. 2^32 - 1 --
        zlib.crc32 of image b's pixels as planar uint8 [3][H][W] bytes -- and int32 [B], 1 where image b was coded in full.  reduce: what the
        decode was given (None or 0: a full decode, or an encode; an int; one per image) -- an image with reduce >= 1 has have = 0, crc = 0 and
        is not read.  Enqueued on the current stream, behind that call; no plan is built, nothing is allocated by the library, nothing
        synchronises.  Whatever form the decode delivered -- planar, interleaved, a float crop, a resized box, views -- the digest is that of
        the whole decoded image."""
        Hs, Ws = np.ascontiguousarray(Hs, dtype=np.int32), np.ascontiguousarray(Ws, dtype=np.int32)
        B = len(Hs)
        if self._ws is None:
            raise _lib.LlictiError(_lib.EINVAL, "digests: no whole-batch call has run on this codec yet")
        one, per = self._modes_arg(mode, B)
        modes = np.array([one], dtype=np.int32) if per is None else per
        red = None if reduce is None else np.ascontiguousarray(np.broadcast_to(np.asarray(reduce, dtype=np.int32), (B,)))
        crc = torch.empty((B,), dtype=torch.int32, device=self.device)
        have = torch.empty((B,), dtype=torch.int32, device=self.device)
        _lib.check(self.L.llicti_digest_images(self.ctx, B, _ptr(Hs), _ptr(Ws), _ptr(modes), len(modes), _ptr(red), _ptr(self._ws), self._ws.numel(),
                                               _ptr(crc), _ptr(have), _stream_ptr(self.device)))
        return self._crc_i64(crc), have

    def counter(self, name):
        """llicti_get_counter: "device_syncs", "device_allocs", "plan_builds", "plan_hits", "block_waits", "plans_cached", "blocks_pooled"."""
        v = C.c_long()
        _lib.check(self.L.llicti_get_counter(self.ctx, name.encode(), C.byref(v)))
        return int(v.value)

    def set_profiling(self, on=True):
        _lib.check(self.L.llicti_set_profiling(self.ctx, int(bool(on))))

    PROF_CATS = ("cnn", "rans_stage", "rans_tail", "cdf_pairs", "rans_encode", "ac", "misc")

    def last_timing_detail(self):
        """-> ({kernel group: ms}, [ms of every band-CNN launch, scale 4..0 x band 0..2]) of the last whole-batch call."""
        cat = (C.c_float * len(self.PROF_CATS))()
        per = (C.c_float * 64)()
        n = C.c_int()
        _lib.check(self.L.llicti_last_timing_detail(self.ctx, cat, per, 64, C.byref(n)))
        return dict(zip(self.PROF_CATS, [float(v) for v in cat])), [float(per[i]) for i in range(min(n.value, 64))]

    def last_cnn_level_ms(self):
        """-> [ms of the band-CNN launches of level 0 .. 4] of the last whole-batch call (profiling on)."""
        ms = (C.c_float * 5)()
        _lib.check(self.L.llicti_last_cnn_level_ms(self.ctx, ms))
        return [float(v) for v in ms]

    def last_timing(self):
        ms = (C.c_float * 4)()
        n = C.c_int()
        _lib.check(self.L.llicti_last_timing(self.ctx, ms, C.byref(n)))
        return list(ms), n.value


# ---------------------------------------------------------------------- container <-> bytestream_list
def levels_of_header(byte0) -> int:
    """Wavelet levels of the model that wrote a container, from its header byte 0: 2 (config B: 2 scales, or its xwide tag 0xE9), else 5."""
    return 2 if int(byte0) in (2, 0xE9) else 5


def container_to_bytestream_list(buf: np.ndarray, seg_len: np.ndarray, nlevels=None):
    """Flat container of one image -> the reference's list of 1 + L lists x 9 `bytes` (L = 5 / 2 levels for config A / B, by default read
    from the header) (LLICTI_nets.py:352-354, :411; loggers/rate.py:133 needs 9 entries per row)."""
    L = levels_of_header(buf[0]) if nlevels is None else int(nlevels)
    segs, pos = [], 0
    for n in seg_len[:4 + 9 * L]:
        segs.append(bytes(buf[pos:pos + int(n)]))
        pos += int(n)
    em = b""
    bl = [[segs[0], segs[1], segs[2], segs[3], em, em, em, em, em]]
    for s in range(L):
        bl.append(segs[4 + 9 * s: 4 + 9 * (s + 1)])
    return bl


def bytestream_list_to_container(bl):
    """-> (flat container, seg_len int32 [NSEG]): a config-B list (3 rows) leaves the lengths past its 22 segments 0."""
    if len(bl) not in (6, 3) or any(len(r) != 9 for r in bl):
        raise ValueError("bytestream_list must be 6 (config A) or 3 (config B) lists of 9 byte strings")
    segs = list(bl[0][:4])
    for s in range(1, len(bl)):
        segs += list(bl[s])
    seg_len = np.zeros(NSEG, dtype=np.int32)
    seg_len[:len(segs)] = [len(s) for s in segs]
    return np.frombuffer(b"".join(segs), dtype=np.uint8).copy(), seg_len


def header_dims(hdr17: bytes):
    H, W = C.c_int(), C.c_int()
    buf = (C.c_uint8 * 17).from_buffer_copy(bytes(hdr17[:17]).ljust(17, b"\0"))
    _lib.check(_lib.lib().llicti_header_dims(buf, C.byref(H), C.byref(W)))
    return H.value, W.value
