"""Shared test helpers (synthetic inputs; no reference code)."""
import numpy as np


def make_image(kind, H, W, seed):
    """Same generators as tests/golden/make_fixtures.py: i.i.d. uniform RGB, or low-pass 'smooth' RGB."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, size=(3, H, W), dtype=np.uint8)
    base = rng.standard_normal((3, H + 16, W + 16))
    k = np.ones(9) / 9.0
    for _ in range(2):
        base = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, base)
        base = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 2, base)
    base = base[:, 8:8 + H, 8:8 + W]
    lum = base[0:1] * 220.0
    img = 128 + lum + base * 60.0 + np.linspace(-40, 40, W)[None, None, :]
    img = img + rng.standard_normal(img.shape) * 2.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def make_batch(kind, B, H, W, seed0=0):
    return np.stack([make_image(kind, H, W, seed0 + i) for i in range(B)])


def make_sampled_image(H, W, seed):
    """An image DRAWN FROM THE MODEL (trained-like weights): the reference-format decoder run on streams of random bytes (an arithmetic decoder
    fed random bits emits symbols with the model's own probabilities), behind the header -- size, value ranges, coarsest pixels -- of the smooth
    image of the same size.  The content class of a model that predicts its data well: cheap symbols (about 4.8 bits each) over the full value
    range -- what the sigma-floor noise batch and the 21-bpp smooth image are not.  Test infrastructure (uses the CPU oracle); deterministic."""
    import os
    from oracle import oracle as orc
    from llicti_amd.weights import pack_state_dict
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    W_o = orc.Weights(pack_state_dict(dict(np.load(os.path.join(gold, "weights_trainedlike.npz")))))
    bl = orc.encode_image(make_image("smooth", H, W, 11), W_o)
    rng = np.random.default_rng(seed)
    bl = [list(bl[0])] + [[rng.integers(0, 256, len(s), dtype=np.uint8).tobytes() for s in row] for row in bl[1:]]
    return orc.decode_image(bl, W_o)


def xwide_stream_header(stream: bytes):
    """(T field = ceil(T / 32), one-chain flag, bits of the main region below the header field) of an xwide v4 stream (oracle/llicti_oracle.h, "stream"):
    bit region | 992 bytes of states; the region's highest set bit is its end marker, the 9 bits below it the header field."""
    nbytes = len(stream) - 992
    assert nbytes >= 2 and stream[nbytes - 1] != 0
    top = 8 * (nbytes - 1) + stream[nbytes - 1].bit_length() - 1
    v = int.from_bytes(stream[:nbytes], "little")
    f9 = (v >> (top - 9)) & 0x1FF
    return f9 & 0xFF, f9 >> 8, top - 9


# Shapes whose band grids put the band CNN's input halo exactly on the last row / column its fast staging path accepts (h - 2, w - 2) and on the
# first one it refuses (h - 1, w - 1), for every tile form, at both parities of the level grid (tile_edge_classes): the tile-edge sweep of
# tests/test_ref64_cpu.py and tests/test_hip_tile_edges.py.  Found by a greedy search over H in 64..200, W in 64..260.
SWEEP_SHAPES = [(H, W) for H in (67, 68, 69, 70) for W in (133, 134, 195, 196)]
TILE_ROWS = (16, 8, 4)            # the band CNN's tile forms (rows; 32 columns each)


def tile_edge_classes(H, W, levels=(0, 1, 2)):
    """Set of (TH, row class, column class, Hl & 1, Wl & 1) the band CNN's tiles of an H x W image fall into at the given levels.  A tile of TH rows
    stages rows ty TH - 2 .. ty TH + TH + 1 and columns 32 tx - 2 .. 32 tx + 33 of the band grid h x w (llicti_amd/csrc/band_cnn.hpp); the
    fast path takes it if they lie inside the grid and end at h - 2 / w - 2 at the latest.  Row class: "fast" (ends at h - 2: the last tile
    accepted) or "border" (ends at h - 1: the first refused); column class: "fast_edge", "border_edge" or "interior" (a fast column range ending
    before w - 2).  Tiles of no class (ending elsewhere) are not counted."""
    out = set()
    for lvl in levels:
        st = 1 << lvl
        Hl, Wl = -(-H // st), -(-W // st)
        h, w = (Hl + 1) // 2, (Wl + 1) // 2
        for TH in TILE_ROWS:
            for ty in range(-(-h // TH)):
                i0, i1 = ty * TH - 2, ty * TH + TH + 1
                rc = "fast" if (i0 >= 0 and i1 == h - 2) else "border" if i1 == h - 1 else None
                if rc is None:
                    continue
                for tx in range(-(-w // 32)):
                    j0, j1 = 32 * tx - 2, 32 * tx + 33
                    cc = "fast_edge" if (j0 >= 0 and j1 == w - 2) else "border_edge" if j1 == w - 1 else "interior" if (j0 >= 0 and j1 < w - 2) else None
                    if cc is not None:
                        out.add((TH, rc, cc, Hl & 1, Wl & 1))
    return out


def all_tile_edge_classes():
    return {(TH, rc, cc, ph, pw) for TH in TILE_ROWS for rc in ("fast", "border") for cc in ("fast_edge", "border_edge", "interior")
            for ph in (0, 1) for pw in (0, 1)}


# Frozen config B rANS containers (tests/golden/rans_b_vectors.npz, written by the HIP encoder: tests/golden/make_rans_b_vectors.py):
# key -> (make_image kind, H, W, seed, config B weight set, xwide streams).  One odd shape, one even.
B_CORRUPT_BASE = "b_noise_33x40_x3"           # ... whose stream 0 is also flipped bit by bit, with the HIP decoders' verdicts recorded
B_VECTORS = {"b_noise_33x40_x3": ("noise", 33, 40, 9, "rand1337", 3), "b_smooth_64x96_x2": ("smooth", 64, 96, 9, "trainedlike", 2)}


def two_valued_image(H, W, seed=5):
    """R = B = 100, G in {100, 101}: the Cg channel has exactly two values (A = 2, n = 31 raw symbols per seed)."""
    r = np.random.default_rng(seed)
    img = np.full((3, H, W), 100, np.uint8)
    img[1] += r.integers(0, 2, (H, W)).astype(np.uint8)
    return img


def bw_image(H, W, seed=7):
    """every sample 0 or 255: the full chroma range (A = 511) from two pixel values"""
    return (np.random.default_rng(seed).integers(0, 2, (3, H, W)) * 255).astype(np.uint8)


def flat_image(H, W):
    return np.full((3, H, W), 201, np.uint8)


# The images of the rANS format tests (tests/test_ref_rans.py, tests/test_hip_ref_rans.py): name -> maker.
RANS_TEST_IMAGES = {
    "smooth67": lambda: make_image("smooth", 67, 93, 3), "noise67": lambda: make_image("noise", 67, 93, 3),
    "smooth33": lambda: make_image("smooth", 33, 64, 4), "noise33": lambda: make_image("noise", 33, 64, 4),
    "smooth32": lambda: make_image("smooth", 32, 32, 2), "smooth32b": lambda: make_image("smooth", 32, 32, 1), "noise32": lambda: make_image("noise", 32, 32, 1),
    "smooth64": lambda: make_image("smooth", 64, 96, 6), "noise64": lambda: make_image("noise", 64, 96, 6),
    "flat33": lambda: flat_image(33, 64), "flat192": lambda: flat_image(192, 192), "two64": lambda: two_valued_image(64, 96), "two67": lambda: two_valued_image(67, 93),
    "bw33": lambda: bw_image(33, 64), "bw32": lambda: bw_image(32, 32),
    "b_noise33x40": lambda: make_image("noise", 33, 40, 9),                # (the image of B_VECTORS' corruption base)
}


def corruptions(stream, L, layout, seed, n_state=32, n_main=32):
    """The fixed, seeded set of single-bit flips of one stream: (name, bit index in the stream's bytes).  Every bit of the bit region's last two
    bytes, its lowest 64 bits (a v4 stream's spill lies there), n_state seeded positions in the states and n_main in the main bits."""
    nstate = 31 * L // 8
    r0 = 16 if layout == "v3" else 0
    r1 = 8 * (len(stream) - nstate)
    rng = np.random.default_rng(seed)
    out = [("top", b) for b in range(max(r0, r1 - 16), r1)]
    out += [("low", b) for b in range(r0, min(r1, r0 + 64))]
    out += [("state", int(b)) for b in r1 + rng.choice(8 * nstate, n_state, replace=False)]
    if r1 - 16 > r0 + 64:
        out += [("main", int(b)) for b in r0 + 64 + rng.choice(r1 - 16 - r0 - 64, min(n_main, r1 - 16 - r0 - 64), replace=False)]
    return out


def corrupted(bl, stream_index, bit):
    bad = [list(r) for r in bl]
    b = bytearray(bad[1][stream_index])
    b[bit >> 3] ^= 1 << (bit & 7)
    bad[1][stream_index] = bytes(b)
    return bad


def padded_to_88(packed):
    """pack_state_dict() of a 60-wide model -> the same model as an 88-wide one: channels 60..87 of every head have zero weights and biases."""
    out = {}
    for b, d in packed.items():
        hw, K0 = int(d["head"]), int(d["K0"])
        assert hw == 60
        w0, b0 = np.zeros((4 * 88, K0), np.float32), np.zeros(4 * 88, np.float32)
        w1, b1 = np.zeros((4 * 88, 88), np.float32), np.zeros(4 * 88, np.float32)
        w2 = np.zeros((60, 88), np.float32)
        for g in range(4):
            w0[g * 88:g * 88 + hw] = d["w0"][g * hw:(g + 1) * hw]
            b0[g * 88:g * 88 + hw] = d["b0"][g * hw:(g + 1) * hw]
            w1[g * 88:g * 88 + hw, :hw] = d["w1"][g * hw:(g + 1) * hw]
            b1[g * 88:g * 88 + hw] = d["b1"][g * hw:(g + 1) * hw]
        w2[:, :hw] = d["w2"]
        out[b] = {"K0": K0, "head": 88, "w0": w0, "b0": b0, "w1": w1, "b1": b1, "w2": w2, "b2": np.ascontiguousarray(d["b2"], dtype=np.float32)}
    return out


class StreamGate:
    """Holds a HIP stream busy so that ordering bugs become deterministic (tests/test_hip_streams.py, DESIGN.md "the gate"): hold(stream, ms)
    enqueues a one-thread spin kernel of about `ms` milliseconds (torch.cuda._sleep; its cycles per millisecond are measured once, with events,
    when the gate is made) and records two timing events around it.  Whatever is enqueued on the stream afterwards starts when the spin ends;
    whatever is NOT ordered behind the stream runs while it spins.  The gate feeds the library nothing and needs no hook in it.  A test asserts
    `end.query() is False` once it has enqueued everything: a gate that ran out before that proves nothing and must fail the test."""

    def __init__(self, torch, device="cuda:0", probe_cycles=4_000_000):
        self.torch, self.device = torch, torch.device(device)
        s = torch.cuda.Stream(device=self.device)
        best = None
        for _ in range(3):                      # (the first launch pays for loading the kernel)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                torch.cuda._sleep(probe_cycles)
                e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        assert best > 0
        self.cycles_per_ms = probe_cycles / best

    def hold(self, stream, ms):
        """-> (begin, end): timing events on `stream` around a spin of about `ms` milliseconds; begin.elapsed_time(end) is its measured length
        once `end` has fired."""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            torch.cuda._sleep(int(ms * self.cycles_per_ms))
            e1.record()
        return e0, e1


# ---- device buffers of the record tests (tests/test_hip_archive.py, tests/test_hip_progressive.py)
DEV = "cuda:0"
POISON = 0xA5
GUARD = 64


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)           # (a writable copy: some inputs are views of `bytes`)


def guarded(torch, nbytes, offset=0):
    """-> (buffer, view, base): a poisoned buffer with GUARD bytes before and at least GUARD after a view of nbytes that starts `offset` bytes
    past a 256-byte boundary"""
    buf = torch.full((256 + GUARD + offset + nbytes + GUARD + 16,), POISON, dtype=torch.uint8, device=DEV)
    base = (-buf.data_ptr()) % 256 + GUARD + offset
    if base < GUARD:
        base += 256
    view = buf[base:base + nbytes]
    assert view.data_ptr() % 16 == offset % 16
    return buf, view, base


def guards_intact(buf, base, nbytes):
    return bool((buf[:base] == POISON).all()) and bool((buf[base + nbytes:] == POISON).all())


def crop_windows(img, y0, x0, ch=None, cw=None, margin=2, levels=5):
    """A crop of a large image that the CPU oracle can afford, and where the crop's band grids equal the image's (tests/test_large_cpu.py holds the
    rule on the oracle; tests/test_hip_large.py uses it on images the oracle cannot run whole).  The band CNN is local -- a 5x5 window of its band
    grid -- so the crop img[:, y0:y0 + ch, x0:x0 + cw], with y0 and x0 multiples of 32 (every level's grid then starts on a grid position of the
    image's) and each side either ending at the image's edge (ch / cw None: the true border and its odd-edge pad are inside the crop) or a
    multiple of 32 long, has bit-equal band_params from `margin` positions inwards of every side the crop CUT; a side that is the image's own needs none.
    -> (crop, [per level: (rows of the image's grid, columns of it, rows of the crop's grid, columns of it)], slices)."""
    H, W = img.shape[-2:]
    ch = H - y0 if ch is None else ch
    cw = W - x0 if cw is None else cw
    assert y0 % 32 == 0 and x0 % 32 == 0 and 0 < ch <= H - y0 and 0 < cw <= W - x0
    assert (y0 + ch == H or ch % 32 == 0) and (x0 + cw == W or cw % 32 == 0)
    crop = img[..., y0:y0 + ch, x0:x0 + cw]
    wins = []
    for lvl in range(levels):
        st = 2 << lvl                                            # pixels per position of the level's band grids
        gh, gw = -(-(-(-ch // (st // 2))) // 2), -(-(-(-cw // (st // 2))) // 2)      # (ceil(ceil(n / 2^lvl) / 2): the grid of the crop)
        oy, ox = y0 // st, x0 // st
        t, l = (margin if y0 else 0), (margin if x0 else 0)
        b, r = (margin if y0 + ch < H else 0), (margin if x0 + cw < W else 0)
        assert gh - t - b > 0 and gw - l - r > 0, "the crop is too small for this margin at level %d" % lvl
        wins.append((slice(oy + t, oy + gh - b), slice(ox + l, ox + gw - r), slice(t, gh - b), slice(l, gw - r)))
    return crop, wins
