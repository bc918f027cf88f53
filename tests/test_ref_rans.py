"""tests/ref_rans.py -- the second, literal reading of the rANS containers -- against the CPU oracle's bytes.

The oracle (oracle/llicti_oracle.c) wrote every rANS byte the suite had seen, and read them back; ref_rans is a decoder written from the format
text alone.  Here it decodes the frozen vectors and the oracle's containers over a matrix of small cases, with every check of the text and every
re-derivation of an encoder choice on (T, the field, the one-chain flag, the "auto" count); two vectors are worked out by hand; every check is
shown to be live on a minimally edited stream; and single-bit corruptions of real containers are put to both readers: they must refuse the same
ones and agree on the pixels of the ones they accept.

CONFIG B (2 levels, byte 0 = 0xE9): the CPU oracle's container code restates config A only, so nothing on a machine without a GPU WRITES config B
bytes or gives a second verdict on corrupted ones.  Its containers are therefore frozen ones written by the HIP encoder
(tests/golden/rans_b_vectors.npz, make_rans_b_vectors.py: an odd and an even shape), with the HIP decoders' verdicts on a fixed set of bit flips
recorded next to them.  The CDF rows do not need the container code: orc.band_params runs the 60-wide heads zero-padded to its 88 channels (bit-exact,
tests/test_hip_border_staging.py) and orc.cdf_rows does not depend on the model.
"""
import os

import numpy as np
import pytest

import ref_rans as rr
from conftest import GOLDEN, load_case
from helpers import B_CORRUPT_BASE, B_VECTORS, RANS_TEST_IMAGES as IMAGES, corrupted, corruptions, make_image, padded_to_88, xwide_stream_header
from oracle import oracle as orc

TOP = 0x80000000


# ------------------------------------------------------------------------------------------------------------------ the matrix
KIND = {"rans": 0, "wrans": 1, "xrans": 2}
# name -> (image, weights, lane kind, M, auto).  Every lane kind x M in 1, 2, 3, 5, wide 14, 32 / 64 / 128; the five content kinds; both weight sets;
# 32x32, 33x64, 67x93, 64x96; 192x192 for the caps (v4: field 255, v3: T = 2047) only; the cheap cases at their own size (T >= 4096, "auto").
MATRIX = {
    "rans1-smooth67": ("smooth67", "trainedlike", "rans", 1, False), "rans2-noise33": ("noise33", "rand1337", "rans", 2, False),
    "rans3-bw33": ("bw33", "trainedlike", "rans", 3, False), "rans5-two64": ("two64", "rand1337", "rans", 5, False),
    "rans32-noise67": ("noise67", "trainedlike", "rans", 32, False), "rans64-smooth67": ("smooth67", "trainedlike", "rans", 64, False),
    "rans128-noise64": ("noise64", "rand1337", "rans", 128, False), "rans1-flat192": ("flat192", "trainedlike", "rans", 1, False),
    "wrans1-noise67": ("noise67", "rand1337", "wrans", 1, False), "wrans2-smooth33": ("smooth33", "trainedlike", "wrans", 2, False),
    "wrans3-flat33": ("flat33", "rand1337", "wrans", 3, False), "wrans5-smooth64": ("smooth64", "trainedlike", "wrans", 5, False),
    "wrans14-noise32": ("noise32", "rand1337", "wrans", 14, False), "wrans1-flat192": ("flat192", "trainedlike", "wrans", 1, False),
    "xrans1-smooth67": ("smooth67", "trainedlike", "xrans", 1, False), "xrans2-two64": ("two64", "trainedlike", "xrans", 2, False),
    "xrans3-noise67": ("noise67", "rand1337", "xrans", 3, False), "xrans5-noise32": ("noise32", "rand1337", "xrans", 5, False),
    "xrans5-flat33": ("flat33", "trainedlike", "xrans", 5, False), "xrans2-bw33": ("bw33", "rand1337", "xrans", 2, False),
    "xrans1-noise67": ("noise67", "rand1337", "xrans", 1, False), "xrans32-two67": ("two67", "trainedlike", "xrans", 32, False),
    "xrans64-smooth67": ("smooth67", "trainedlike", "xrans", 64, False), "xrans128-noise67": ("noise67", "rand1337", "xrans", 128, False),
    "xrans1-flat192": ("flat192", "trainedlike", "xrans", 1, False), "xrans3-smooth32": ("smooth32", "rand1337", "xrans", 3, False),
    "xauto1-noise67": ("noise67", "rand1337", "xrans", 1, True), "xauto2-smooth67": ("smooth67", "trainedlike", "xrans", 2, True),
    "xauto4-cheap-single": ("cheap-single", None, "xrans", 4, True), "xauto4-cheap-sharp": ("cheap-sharp", None, "xrans", 4, True),
}
_results = {}


def _case(name, oracle_weights):
    """(image, oracle weights, bytestream list, ref_rans info) of a matrix case: encoded by the oracle and decoded by ref_rans ONCE per session."""
    if name not in _results:
        iname, wname, kind, M, auto = MATRIX[name]
        if iname.startswith("cheap-"):
            from test_oracle_golden import _cheap_case
            _, W, img = _cheap_case(iname[6:])
        else:
            img, W = IMAGES[iname](), oracle_weights(wname)
        bl = orc.encode_image_rans(img, W, M, KIND[kind], auto=auto)
        segs = rr.segments(bl)
        planes, info = rr.decode_image(segs, rr.OraclePlanes(segs, W))       # canonical=True: every check and every re-derivation
        _results[name] = (img, W, bl, info, orc.unlift(planes))
    return _results[name]


@pytest.mark.parametrize("name", list(MATRIX))
def test_oracle_bytes_decode_with_every_check(name, oracle_weights):
    img, W, bl, info, got = _case(name, oracle_weights)
    assert np.array_equal(got, img), name
    iname, wname, kind, M, auto = MATRIX[name]
    hdr = info["header"]
    assert hdr["L"] == {"rans": 64, "wrans": 128, "xrans": 256}[kind]
    if auto:
        # the header's count is what the rule of include/llicti_hip.h gives for the last stage's frequencies, in plain Python
        assert hdr["M"] == rr.auto_pick(M, info["last_freqs"]), (name, hdr["M"])
    else:
        assert hdr["M"] == M
    if kind == "xrans":
        # the existing parser of the field and this reader agree on every v4 stream seen
        streams = rr.split_streams(rr.segments(bl)[4:], hdr)
        for s, f in zip(streams, info["streams"]):
            assert xwide_stream_header(s) == (f["field"], f["one_chain"], f["main_bits"])


def test_frozen_vectors():
    """Every container of tests/golden/rans_vectors.npz, from its stored bytes and segment lengths alone, decodes to the fixture image."""
    from llicti_amd.weights import pack_state_dict
    vec = np.load(os.path.join(GOLDEN, "rans_vectors.npz"))
    n = 0
    for case, wname in [("smooth_67x93_tl", "trainedlike"), ("noise_32x32_rand", "rand1337"), ("noise_33x64_tl", "trainedlike")]:
        rgb = load_case(case)["rgb"]
        W = orc.Weights(pack_state_dict(dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz")))))
        for key, L, M in (("M1", 64, 1), ("M4", 64, 4), ("W3", 128, 3), ("X4", 256, 3)):
            flat, lens = vec[f"{case}_{key}_bytes"].tobytes(), list(vec[f"{case}_{key}_seglen"])
            segs, pos = [], 0
            for ln in lens:
                segs.append(flat[pos:pos + ln])
                pos += ln
            segs = segs[:4] + segs[9:]                       # the bytestream list's first row is 4 header segments + 5 empty ones
            planes, info = rr.decode_image(segs, rr.OraclePlanes(segs, W))
            assert (info["header"]["L"], info["header"]["M"]) == (L, M)
            assert np.array_equal(orc.unlift(planes), rgb), (case, key)
            n += 1
    assert n == 12


# ------------------------------------------------------------------------------------------------------------------ config B
_b = {}


def _b_weights(wname):
    from llicti_amd.weights import pack_state_dict
    if wname not in _b:
        _b[wname] = orc.Weights(padded_to_88(pack_state_dict(dict(np.load(os.path.join(GOLDEN, f"weights_b_{wname}.npz"))))))
    return _b[wname]


def _b_vector(key):
    """(image, oracle weights for config B, segments) of a frozen config B container"""
    kind, H, W, seed, wname, M = B_VECTORS[key]
    vec = np.load(os.path.join(GOLDEN, "rans_b_vectors.npz"))
    flat, pos, segs = vec[f"{key}_bytes"].tobytes(), 0, []
    for ln in vec[f"{key}_seglen"]:
        segs.append(flat[pos:pos + int(ln)])
        pos += int(ln)
    return make_image(kind, H, W, seed), _b_weights(wname), segs, vec


@pytest.mark.parametrize("key", list(B_VECTORS))
def test_config_b_frozen_containers(key):
    """Config B's xwide v4 containers as the HIP encoder wrote them, an odd and an even shape: 22 segments, two levels, the DC band at stride 4; decoded
    with every check and re-derivation on, to the image."""
    import hashlib
    img, W, segs, vec = _b_vector(key)
    assert hashlib.sha256(b"".join(segs)).digest() == vec[f"{key}_sha256"].tobytes()
    assert len(segs) == 22 and segs[0][0] == 0xE9
    planes, info = rr.decode_image(segs, rr.OraclePlanes(segs, W))
    assert info["header"]["nlevels"] == 2 and info["header"]["M"] == B_VECTORS[key][5]
    assert np.array_equal(orc.unlift(planes), img), key
    assert any(f["T"] for f in info["streams"])
    with pytest.raises(RuntimeError):
        orc.decode_image_rans([segs[:4] + [b""] * 5] + [segs[4 + 9 * r:13 + 9 * r] for r in range(2)] + [[b""] * 9] * 3, _b_weights("rand1337"))   # the A-only reader refuses the tag


def test_config_b_corrupted_container_against_recorded_hip_verdicts():
    """The config B corruption base: the fixed set of single-bit flips of its stream 0.  The second opinion here is the HIP decoders' -- image_status and
    the decoded pixels' SHA-256, recorded on an MI355X when the fixture was written: ref_rans refuses if and only if the device did, and decodes
    to the same pixels where both accept.  Both outcomes occur."""
    import hashlib
    img, W, segs, vec = _b_vector(B_CORRUPT_BASE)
    flips = corruptions(segs[4], 256, "v4", seed=11)
    assert [b for _, b in flips] == list(vec[f"{B_CORRUPT_BASE}_flip_bits"])
    refused, digests = vec[f"{B_CORRUPT_BASE}_flip_refused"], vec[f"{B_CORRUPT_BASE}_flip_sha256"]
    cache = {}
    n_acc = 0
    for k, (name, bit) in enumerate(flips):
        bad = list(segs)
        b = bytearray(bad[4])
        b[bit >> 3] ^= 1 << (bit & 7)
        bad[4] = bytes(b)
        try:
            planes, _ = rr.decode_image(bad, rr.OraclePlanes(bad, W, cache), canonical=False)
            got = orc.unlift(planes)
        except rr.Refused:
            got = None
        assert (got is None) == bool(refused[k]), (name, bit, "ref_rans " + ("refuses" if got is None else "accepts"))
        if got is not None:
            assert hashlib.sha256(got.tobytes()).digest() == digests[k].tobytes(), (name, bit)
            n_acc += 1
    assert 0 < n_acc < len(flips), n_acc


# ------------------------------------------------------------------------------------------------------------------ coverage
REQUIRED = {"v4-one-chain", "v4-two-chains", "spill>0", "T=whole-share", "T<share", "field-255", "cheap-T>=4096", "empty-stream", "A=2-two-chains"}
ALSO = {"A=1", "A=511", "share<2n", "silent-start", "v3-T=2047", "v3-length-table", "v4-length-table", "v3-64-lanes", "v3-128-lanes",
        "two-chains-gap", "auto-cheap", "auto-expensive", "auto-ordinary", "auto-unfilled"}


def _classes(name, info):
    out = set()
    hdr = info["header"]
    auto = MATRIX[name][4]
    if hdr["per_seg"] > 1:
        out.add(hdr["layout"] + "-length-table")
    if hdr["layout"] == "v3":
        out.add(f"v3-{hdr['L']}-lanes")
    if auto:
        Mlo, n, S = MATRIX[name][3], len(info["last_freqs"]), sum(16 - rr.floor_log2(f) for f in info["last_freqs"])
        M = hdr["M"]
        out.add("auto-expensive" if (S >= 11 * n and M > Mlo) else "auto-cheap" if (S < 4 * n and Mlo // 2 < M < Mlo)
                else "auto-ordinary" if M == Mlo else "auto-unfilled")
    for f in info["streams"]:
        T, share = f["T"], f["share"]
        if share == 0:
            out.add("empty-stream")
        if hdr["layout"] == "v3":
            if T == 2047:
                out.add("v3-T=2047")
            continue
        if T and f["one_chain"]:
            out.add("v4-one-chain")
            if f["tail_final_state"] < TOP:
                out.add("silent-start")
        if T and not f["one_chain"]:
            out.add("v4-two-chains")
            if f["A"] == 2:
                out.add("A=2-two-chains")
            if f["gap"]:
                out.add("two-chains-gap")
        if f["spill"]:
            out.add("spill>0")
        if T and T == share:
            out.add("T=whole-share")
        if T < share:
            out.add("T<share")
        if f["field"] == 255 and T == 8160:
            out.add("field-255")
        if "cheap" in name and T >= 4096:
            out.add("cheap-T>=4096")
        if 0 < share < 2 * f["n_seed"]:
            out.add("share<2n")
        if f["A"] in (1, 511):
            out.add(f"A={f['A']}")
    return out


def test_matrix_covers_every_format_class(oracle_weights):
    """The matrix above reaches every class of stream the format text distinguishes -- so that an edit of the matrix cannot drop one silently (as
    test_sweep_shapes_cover_every_tile_edge_class does for the tile sweep).  REQUIRED: both v4 tail forms, a spill, a tail that is the stream's whole
    share and one that is not, the field's cap (255: T = 8,160), a tail beyond 4,095 symbols on a cheap source, a stream without symbols, two chains
    at the smallest alphabet that has symbols to code (A = 2: 31 raw symbols per seed).  ALSO, each reached by an input of a few seconds: A = 1 and
    the silent start (a flat image), A = 511 (a 0 / 255 image), a share shorter than the 2 n seed symbols (15 symbols: the 67x93 two-valued image in
    32 streams), v3's T = 2047 (the flat 192x192 image), both length-table modes, zeros between two chains, the four outcomes of the "auto" rule."""
    got = set()
    for name in MATRIX:
        got |= _classes(name, _case(name, oracle_weights)[3])
    assert REQUIRED <= got, sorted(REQUIRED - got)
    assert ALSO <= got, sorted(ALSO - got)
    assert {MATRIX[n][1] for n in MATRIX} >= {"trainedlike", "rand1337"}
    for kind, extra in (("rans", {32, 64, 128}), ("wrans", {14}), ("xrans", {32, 64, 128})):
        assert {MATRIX[n][3] for n in MATRIX if MATRIX[n][2] == kind and not MATRIX[n][4]} >= {1, 2, 3, 5} | extra, kind


# ------------------------------------------------------------------------------------------------------------------ header
def test_header_every_tag():
    """byte 0 and the pad field's bits 10 .. 15 for every value: what the text defines is read as it says, everything else is refused -- and
    llicti_amd.codec.mode_of_header (the product's reading) agrees on which are which and on the count."""
    from llicti_amd.codec import mode_of_header
    seen = {}
    for b0 in range(256):
        for hi in range(64):
            pad = hi << 10
            try:
                h = rr.parse_header(b0, pad)
            except rr.Refused:
                h = None
            try:
                mode = mode_of_header(b0, pad=pad)
                if mode < 0x100:
                    mode = None                  # a reference-format header, not a rANS container
            except ValueError:
                mode = None
            if h is None:
                assert mode is None, (hex(b0), hi, mode)
                continue
            seen[(b0, hi)] = h
            assert mode is not None, (hex(b0), hi, h)
            assert mode & 0xFF == h["M"] and (mode >> 8) & 7 == {64: 1, 128: 3, 256: 5}[h["L"]], (hex(b0), hi, hex(mode))
    tags = {b0 for b0, _ in seen}
    assert tags == {0x88 | (v & 7) | ((v >> 3) << 4) for v in range(32)} | {0xC8 | (v & 7) | ((v >> 3) << 4) for v in range(18)}
    assert rr.parse_header(0x88, 0) == dict(L=64, M=1, per_seg=1, layout="v3", nlevels=5, nflags=10)
    assert rr.parse_header(0xBF, 0x3FF)["M"] == 32 and rr.parse_header(0xC8, 0)["M"] == 64 and rr.parse_header(0xC9, 0)["per_seg"] == 4
    assert [rr.parse_header(t, 0)["M"] for t in (0xCA, 0xCC, 0xDF)] == [1, 3, 14] and rr.parse_header(0xDF, 0)["L"] == 128
    assert rr.parse_header(0xE8, 34 << 10) == dict(L=256, M=128, per_seg=4, layout="v4", nlevels=5, nflags=10)
    assert rr.parse_header(0xE9, (18 << 10) | 0xF) == dict(L=256, M=18, per_seg=1, layout="v4", nlevels=2, nflags=4)     # config B
    # config B's header carries the count "as in 0xE8"; its container has 18 stream segments, and a count that needs more is refused there
    for u in (19, 32, 33):
        with pytest.raises(rr.Refused) as e:
            rr.split_streams([b""] * 18, rr.parse_header(0xE9, u << 10))
        assert e.value.check == "segments"
    for b0, pad in ((0x05, 0), (0x80, 0), (0xE8, 0), (0xE8, 35 << 10), (0xE9, 35 << 10), (0xE9, (3 << 10) | 0x10), (0x88, 1 << 10), (0xCC, 1 << 15),
                    (0xEA, 3 << 10), (0xF8, 3 << 10), (0xFF, 3 << 10)):
        with pytest.raises(rr.Refused):
            rr.parse_header(b0, pad)


# ------------------------------------------------------------------------------------------------------------------ hand-worked vectors
def _stream8(region_bytes, payload, v3_field=None):
    """A toy stream of L = 8 lanes (248 payload bits): [u16 T field |] bit region | 31 bytes of states."""
    head = b"" if v3_field is None else int(v3_field).to_bytes(2, "little")
    return head + bytes(region_bytes) + int(payload).to_bytes(31, "little")


def test_hand_vector_main_region_two_steps_two_lanes():
    """Two steps of a two-lane main region on the table [0, 0x4000, 0xC000): symbols 0, 1, 2 with f = 2^14, 2^15, 2^14.

    The ENCODER runs the steps backwards and the lanes descending, from the end states x0 = 0x80000001, x1 = 0xC0000003:
      step 1, lane 1, symbol 2 (f 2^14, c_low 0xC000): n minimal with (x >> n) < 2^30 is 2; bits 0b11 out -> region bits 0, 1;
               x = ((0x30000000 / 0x4000) << 16) + 0 + 0xC000 = 0xC000C000
      step 1, lane 0, symbol 0 (f 2^14, c_low 0): n = 2, bits 0b01 -> region bits 2, 3; x = (0x20000000 / 0x4000) << 16 = 0x80000000
      step 0, lane 1, symbol 1 (f 2^15, c_low 0x4000): (x >> n) < 2^31 needs n = 1, bit 0 -> region bit 4;
               x = ((0x60006000 / 0x8000) << 16) + 0x6000 + 0x4000 = 0xC000A000
      step 0, lane 0, symbol 2: n = 2, bits 0b00 -> region bits 5, 6; x = (0x8000 << 16) + 0xC000 = 0x8000C000
    region = 0b0000111 = 0x07, 7 bits (one pad bit in its byte); states in the stream: 0x8000C000, 0xC000A000.
    The DECODER, step 0: lane 0 slot 0xC000 -> symbol 2, x = 0x4000 * 0x8000 = 0x20000000; lane 1 slot 0xA000 -> symbol 1,
      x = 0x8000 * 0xC000 + 0xA000 - 0x4000 = 0x60006000; then lane 0 takes clz = 2 bits [5, 7) = 00 -> 0x80000000, lane 1 one bit [4] = 0 -> 0xC000C000.
    Step 1: lane 0 slot 0 -> symbol 0, x = 0x20000000; lane 1 slot 0xC000 -> symbol 2, x = 0x4000 * 0xC000 = 0x30000000;
      lane 0 takes bits [2, 4) = 01 -> 0x80000001, lane 1 bits [0, 2) = 11 -> 0xC0000003.  The cursor ends at 0."""
    row = [0, 0x4000, 0xC000, 0]
    payload = 0x0000C000 | (0x4000A000 << 31)
    s = rr.Stream(_stream8([0x07], payload, v3_field=1 << 11), 8, "v3")
    assert s.nbits == 7 and s.x[:3] == [0x8000C000, 0xC000A000, TOP]
    assert s.step([row, row]) == [2, 1] and s.x[:2] == [0x80000000, 0xC000C000] and s.cursor == 4
    assert s.step([row, row]) == [0, 2] and s.x[:2] == [0x80000001, 0xC0000003] and s.cursor == 0


ROW_A = [0, 1, 4, 0]            # symbol 0: [0, 1) f 1;  1: [1, 4) f 3;  2: [4, 65536)
ROW_B = [0, 7, 8, 0]            # symbol 0: [0, 7) f 7;  1: [7, 8) f 1;  2: [8, 65536)
V4_TAIL3 = 0x80010000 | (0b11 << 32) | (1 << 34)


def _tail3(arena=V4_TAIL3, f9=0x101, T=3, table=(ROW_A, ROW_B, ROW_A), A=3, canonical=True):
    s = rr.Stream(_stream8(int(f9 | 0x200).to_bytes(2, "little"), arena), 8, "v4")
    out = [None] * len(table)
    rr._tail_v4(s, list(range(len(table))), min(T, len(table)), list(table), out, A, canonical)
    return out, s.facts


def test_hand_vector_v4_one_chain_tail_of_three():
    """A v4 one-chain tail of three symbols (forward order 0, 1, 2; A = 3), rows ROW_A, ROW_B, ROW_A.

    The chain starts from the stream's LAST symbol itself: x = 2.
      push symbol 1 of ROW_B (f 1, c_low 7): 2 < 1 << 16, nothing out; x = ((2 / 1) << 16) + 0 + 7 = 0x20007
      push symbol 0 of ROW_A (f 1, c_low 0): n minimal with (0x20007 >> n) < 0x10000 is 2; bits 0b11 out; x = (0x8001 / 1) << 16 = 0x80010000
    arena: bits [0, 32) the final state 0x80010000, the field 0b11 at bits 32, 33, the end marker at bit 34: 0x7_8001_0000.
    Bit region: nothing of the main coder, the field ceil(3 / 32) = 1 with the one-chain bit = 0x101, the end marker on top: 0x301.
    The DECODER: x = 0x80010000, slot 0 -> symbol 0 of ROW_A, x = 1 * 0x8001 + 0 - 0 = 0x8001; clz = 16, two bits left under the marker: takes
    min(16, 2) = 2 -> x = 0x20007; slot 7 -> symbol 1 of ROW_B, x = 1 * 2 + 7 - 7 = 2; no bit left; the final state 2 < A is the last symbol."""
    out, facts = _tail3()
    assert out == [0, 1, 2]
    assert facts["raw_alen"] == 35 and facts["spill"] == 0 and facts["tail_final_state"] == 0x80010000 and facts["two_rule"] is False


# ------------------------------------------------------------------------------------------------------------------ the checks are live
ROW_U = list(range(511)) + [0]          # 511 symbols (A = 511, n = 3): symbol s < 510 has f = 1 and c_low = s -- 16 bits each


def _two_chain(arena, T, canonical=True, A=511):
    """A toy two-chain stream of 8 lanes: spill 0, so the arena is the 248 payload bits -- chain A's state at bits [0, 32), chain B's at [216, 248)."""
    s = rr.Stream(_stream8(int(0x200 | -(-T // 32)).to_bytes(2, "little"), arena), 8, "v4")
    out = [None] * T
    rr._tail_v4(s, list(range(T)), T, [ROW_U] * T, out, A, canonical)
    return out, s.facts


TWO_OK = TOP | (TOP << 216)             # both chains end at seed 0; every pop of symbol 0 (f = 1) reads 16 zero bits


def test_checks_are_live_v4_two_chains():
    """Each check of the two-chain form fires on a stream edited to violate exactly it.  Base: 16 symbols 0 of frequency 1 -- six of them in the seeds,
    five popped from each chain, 80 bits read at either end, 24 zero bits between the cursors."""
    out, facts = _two_chain(TWO_OK, 16)
    assert out == [0] * 16 and facts["gap"] == 24 and facts["raw_alen"] == 64 + 160
    seeds = TOP | (1 + 2 * 511 + 3 * 511 ** 2)
    assert _two_chain(seeds | ((TOP | 510) << 216), 6)[0] == [0, 0, 510, 3, 2, 1]            # sym(j) = digit j of chain A's seed, of B's from j = n; j counts from the END
    for arena, T, check in ((TWO_OK & ~TOP, 16, "leading-one"), (TWO_OK & ~(TOP << 216), 16, "leading-one"),
                            (TWO_OK, 20, "cross"),                            # seven pops a chain: 112 + 112 bits do not fit 184
                            (TWO_OK | (1 << 120), 16, "between"), (TWO_OK | (1 << 112), 16, "between"), (TWO_OK | (1 << 135), 16, "between"),
                            (TOP | 511 ** 3 | (TOP << 216), 6, "seed"), (TOP | ((TOP | 511 ** 3) << 216), 6, "seed"),
                            (TWO_OK, 5, "seed")):                             # two chains without 2 n symbols to seed them
        with pytest.raises(rr.Refused) as e:
            _two_chain(arena, T, canonical=False)
        assert e.value.check == check, (hex(arena), T, e.value.check)
    assert _two_chain(TOP | (511 ** 3 - 1) | (TOP << 216), 6, canonical=False)[0][-3:] == [510, 510, 510][::-1]     # the largest seed passes


def test_checks_are_live_v4_one_chain():
    """Base: the hand-worked tail of three, and a tail of one (arena = the symbol under its marker)."""
    assert _tail3(2 | (1 << 32), T=1, table=(ROW_A,))[0] == [2]
    # state 0x40000000 pops (symbol 0 of ROW_A, f 1) to 0x4000: clz 17 with 17 bits under the marker -- a field no encoder wrote
    for kw, check in ((dict(arena=0x40000000 | (1 << 49)), "clz16"),
                      (dict(arena=2 | (1 << 33), T=1, table=(ROW_A,)), "unread"),       # a bit under the marker that no symbol takes
                      (dict(arena=3 | (1 << 32), T=1, table=(ROW_A,)), "final"),        # sym(0) = 3 is no symbol of A = 3
                      (dict(arena=(V4_TAIL3 & ~(0b11 << 32)) | (0b10 << 32)), "final"), # field 0b10: x = 0x20006, slot 6 -> symbol 0 of ROW_B, x = 7 * 2 + 6 = 20
                      (dict(arena=2, T=1, table=(ROW_A,)), "marker"),                   # no end marker above the state
                      (dict(arena=0, T=0, table=()), "marker")):
        with pytest.raises(rr.Refused) as e:
            _tail3(canonical=False, **kw)
        assert e.value.check == check, (kw, e.value.check)
    # clz above what is left is the encoder's silent start, not an error: state 0x00010000 pops to 1 (clz 31, two bits left: both taken, x = 7),
    # slot 7 is symbol 1 of ROW_B, x = 0
    assert _tail3(arena=V4_TAIL3 & ~TOP, canonical=False)[0] == [0, 1, 0]
    # a stream without tail symbols is the one-chain form with nothing pushed: state 0 under the marker
    assert _tail3(1 << 32, f9=0x100, T=0, table=())[1]["raw_alen"] == 33
    with pytest.raises(rr.Refused) as e:
        _tail3(1 | (1 << 32), f9=0x100, T=0, table=())
    assert e.value.check == "final"


def test_checks_are_live_v4_stream_and_spill():
    """The stream's frame: the last byte of the bit region holds the end marker, nine bits of field under it; a spill stays below 512 bits and --
    one chain -- ends with the chain's end marker."""
    for region, check in (([0x00, 0x00], "marker"), ([0xFF], "length"), ([0x01, 0x01], "marker")):
        with pytest.raises(rr.Refused) as e:
            rr.Stream(_stream8(region, 0), 8, "v4")
        assert e.value.check == check
    with pytest.raises(rr.Refused) as e:
        rr.Stream(b"\x01\x03" + bytes(30), 8, "v4")
    assert e.value.check == "length"
    # 512 bits under the header field and no symbol for the main coder to take them: a spill of 512
    s = rr.Stream(_stream8(bytes(64) + b"\x01\x03", 0), 8, "v4")
    assert s.cursor == 512
    with pytest.raises(rr.Refused) as e:
        rr._tail_v4(s, [0], 1, [ROW_A], [None], 3, False)
    assert e.value.check == "spill"
    # one chain, a spill of 8 bits whose top bit is not the marker
    s = rr.Stream(_stream8(b"\x01" + b"\x01\x03", 2), 8, "v4")
    assert s.cursor == 8
    with pytest.raises(rr.Refused) as e:
        rr._tail_v4(s, [0], 1, [ROW_A], [None], 3, False)
    assert e.value.check == "marker"
    # a main coder that wants more bits than the region holds
    s = rr.Stream(_stream8(b"\x01\x03", 0), 8, "v4")
    s.x[0] = 0x8000C000
    with pytest.raises(rr.Refused) as e:
        s.step([[0, 0x4000, 0xC000, 0]])
    assert e.value.check == "underrun"
    # A slot below the table's first entry (which need not be 0) is symbol 0 -- entry 0 is the floor of the search, in the oracle and in every HIP
    # decoder -- and the state is updated in 32-bit arithmetic: x = 16379 * 0x8000 + 3 - 5 = 0x1FFD7FFE, clz 3, three bits (0b101) from the region.
    s = rr.Stream(_stream8(b"\x0d\x18", 0), 8, "v4")            # region 0x180D: 0b101, the field 0x101 at bit 3, the marker at bit 12
    assert s.cursor == 3
    s.x[0] = 0x80000003
    assert s.step([[5, 0x4000, 0xC000, 0]]) == [0] and s.x[0] == (0x1FFD7FFE << 3 | 0b101) and s.cursor == 0
    # ... f = 1 and c_low far above the slot: 0x8000 + 3 - 0x9000 wraps to 0xFFFFF003, a state like any other
    s.x[0] = 0x80000003
    assert s.step([[0x9000, 0x9001, 0xC000, 0]]) == [0] and s.x[0] == 0xFFFFF003
    # ... and what such a forgery usually leaves is a state below 2^15, which no push produces (x / f >= 2^15): 0x8000 + 0 - 2 = 0x7FFE, clz 17
    s.x[0] = 0x80000000
    with pytest.raises(rr.Refused) as e:
        s.step([[2, 3, 0xC000, 0]])
    assert e.value.check == "clz16"


V3_ROW = [0, 0x4000, 0xC000, 0]
V3_TAIL2 = 0x8000A000 << 1


def _tail_v3(payload, T, region=(), field=None, nsym=2, canonical=False, presym=()):
    s = rr.Stream(_stream8(region, payload, v3_field=T if field is None else field), 8, "v3")
    out = list(presym) + [None] * (nsym - len(presym))
    rr._tail_v3(s, list(range(nsym)), T, [V3_ROW] * nsym, out, canonical)
    return out


def test_checks_are_live_v3():
    """The 64- / 128-lane tail on a toy stream of 8 lanes, symbols (1, 2) on the table [0, 0x4000, 0xC000).

    Encoder: the first pushed symbol, 2 (f 2^14, c_low 0xC000), starts from f << 15 = 0x20000000 and codes to 2^31 + 0xC000 without a bit; symbol 1
    (f 2^15, c_low 0x4000): n = 1, bit 0 out at payload bit 0, x = ((0x40006000 / 0x8000) << 16) + 0x6000 + 0x4000 = 0x8000A000: the final state, on
    top of the bit: payload = 0x8000A000 << 1.  Decoder: leading one at bit 32; slot 0xA000 -> symbol 1, x = 0x8000 * 0x8000 + 0x6000 = 0x40006000,
    one bit (0) -> 0x8000C000; slot 0xC000 -> symbol 2, x = 0x4000 * 0x8000 = 0x20000000 = f << 15, no bit left."""
    assert _tail_v3(V3_TAIL2, 2, canonical=True) == [1, 2]
    assert _tail_v3(TOP, 0, nsym=0, canonical=True) == []                             # no tail: the tail coder's state 2^31 and nothing else
    for kw, check in ((dict(payload=V3_TAIL2 ^ 2, T=2), "v3-end-state"),              # x = 0x8000A001 ... ends at 0x20000002
                      (dict(payload=V3_TAIL2 << 1, T=2), "v3-end-bits"),              # a zero bit under the tail that no symbol takes
                      (dict(payload=V3_TAIL2, T=2, region=[0x00], field=2 | (7 << 11)), "v3-main"),     # one bit of main region, nobody to read it
                      (dict(payload=0, T=0, nsym=0), "v3-end-state"), (dict(payload=TOP | 1, T=0, nsym=0), "v3-end-state"),
                      (dict(payload=0x7FFFFFFF, T=2), "leading-one"),
                      (dict(payload=V3_TAIL2, T=2, field=2 | (1 << 14)), "pad"), (dict(payload=V3_TAIL2, T=2, field=2 | (1 << 15)), "pad"),
                      (dict(payload=V3_TAIL2, T=2, field=2 | (1 << 11)), "pad"),                        # pad bits without a byte
                      (dict(payload=V3_TAIL2, T=2, region=[0x80], field=2 | (1 << 11)), "pad")):        # the unused bit on top of the region is set
        with pytest.raises(rr.Refused) as e:
            _tail_v3(**kw)
        assert e.value.check == check, (kw, e.value.check)


def test_encoder_choices_are_rederived():
    """A stream that decodes but was not written by the rule is refused as NotCanonical -- and accepted with canonical=False."""
    # v4: the field is ceil(T / 32)
    assert _tail3(f9=0x102, canonical=False)[0] == [0, 1, 2]
    with pytest.raises(rr.NotCanonical) as e:
        _tail3(f9=0x102)
    assert e.value.check == "T-rule"
    # v4: one chain on six symbols of 16 bits each (A = 511, n = 3): the rule -- 2 n sum(16 - floor(log2 f)) = 576 >= k (64 + n) = 402 -- says two
    kw = dict(arena=1 << 32, f9=0x101, T=6, table=(ROW_U,) * 6, A=511)
    assert _tail3(canonical=False, **kw)[0] == [0] * 6
    with pytest.raises(rr.NotCanonical) as e:
        _tail3(**kw)
    assert e.value.check == "flag-rule"
    # ... and two chains on six symbols of ~0 bits (f = 65026 of ROW_U's top symbol 510)
    cheap = TOP | (510 * (1 + 511 + 511 ** 2))
    assert _two_chain(cheap | (cheap << 216), 6, canonical=False)[0] == [510] * 6
    with pytest.raises(rr.NotCanonical) as e:
        _two_chain(cheap | (cheap << 216), 6)
    assert e.value.check == "flag-rule"
    # v4: a tail that stopped although the arena was short of the payload and the share had symbols left
    s = rr.Stream(_stream8(int(0x301).to_bytes(2, "little"), V4_TAIL3), 8, "v4")
    out = [0] + [None] * 3
    with pytest.raises(rr.NotCanonical) as e:
        rr._tail_v4(s, [0, 1, 2, 3], 3, [ROW_A, ROW_A, ROW_B, ROW_A], out, 3, True)
    assert e.value.check == "T-rule" and out == [0, 0, 1, 2]
    # v3: T is maximal -- a third symbol in front of the tail of two would have fitted the 248 payload bits
    assert _tail_v3(V3_TAIL2, 2, nsym=3, presym=(0,)) == [0, 1, 2]
    with pytest.raises(rr.NotCanonical) as e:
        _tail_v3(V3_TAIL2, 2, nsym=3, presym=(0,), canonical=True)
    assert e.value.check == "T-rule"
    # "auto": the four outcomes of the rule, and their order (include/llicti_hip.h, LLICTI_MODE_RANS_X_AUTO)
    assert rr.auto_pick(15, [16] * 200000) == 20 and rr.auto_pick(30, [16] * 400000) == 32        # 12 per symbol: a third more, at most 32
    assert rr.auto_pick(15, [16384] * 200000) == 10                                               # 2 per symbol: two thirds
    assert rr.auto_pick(15, [1024] * 200000) == 15 and rr.auto_pick(15, []) == 15
    assert rr.auto_pick(15, [1024] * 20000) == 8 and rr.auto_pick(15, [16384] * 20000) == 8       # cannot fill the payloads: half
    assert rr.auto_pick(15, [16] * 15000) == 15 and rr.auto_pick(15, [16] * 11000) == 8           # 20 unfilled but 15 filled: the size rule's count


# ------------------------------------------------------------------------------------------------------------------ corrupted containers
CORRUPT_BASES = {"rans2": ("noise32", "rand1337", 0, 2), "wrans2": ("smooth32", "trainedlike", 1, 2),
                 "xrans1-one-chain": ("smooth32b", "trainedlike", 2, 1), "xrans1-two-chains": ("noise32", "rand1337", 2, 1)}


_outcomes = {}


def _corruption_outcomes(base, oracle_weights):
    """(refused by both, accepted by both) over the base's flips; the two readers' agreement is asserted flip by flip.  Once per session."""
    if base in _outcomes:
        return _outcomes[base]
    iname, wname, wide, M = CORRUPT_BASES[base]
    img, W = IMAGES[iname](), oracle_weights(wname)
    bl = orc.encode_image_rans(img, W, M, wide)
    hdr = rr.parse_header(bl[0][0][0], int.from_bytes(bl[0][2], "little"))
    if hdr["layout"] == "v4":
        assert xwide_stream_header(bl[1][0])[1] == (base == "xrans1-one-chain"), base         # the base has the tail form its name says
    cache = {}
    n_ref = n_acc = 0
    for name, bit in corruptions(bl[1][0], hdr["L"], hdr["layout"], seed=11):
        bad = corrupted(bl, 0, bit)
        try:
            want = orc.decode_image_rans(bad, W)
        except RuntimeError:
            want = None
        segs = rr.segments(bad)
        try:
            planes, _ = rr.decode_image(segs, rr.OraclePlanes(segs, W, cache), canonical=False)
            got = orc.unlift(planes)
        except rr.Refused:
            got = None
        assert (got is None) == (want is None), (base, name, bit, "ref_rans " + ("refuses" if got is None else "accepts"))
        if got is not None:
            assert np.array_equal(got, want), (base, name, bit)
            n_acc += 1
        else:
            n_ref += 1
    _outcomes[base] = (n_ref, n_acc)
    return _outcomes[base]


@pytest.mark.parametrize("base", list(CORRUPT_BASES))
def test_corrupted_containers_both_readers_agree(base, oracle_weights):
    """A third opinion on what the format's checks catch: for each single-bit flip ref_rans refuses if and only if the oracle's decoder does, and where
    both accept the pixels are equal.  (Encoder choices are not a reader's business: canonical=False.)  Segment lengths are not touched."""
    n_ref, n_acc = _corruption_outcomes(base, oracle_weights)
    assert n_ref > 0, base


def test_corrupted_containers_both_outcomes_occur(oracle_weights):
    """The comparison above is live: some flips are refused by both readers and some accepted by both, in both v4 tail forms.  (A v3 stream has no
    slack: its payload is used to the tail state's leading one and, now that the pad bits on top of the bit region are checked, every flip of the
    64- and 128-lane bases is refused by both.)"""
    got = {base: _corruption_outcomes(base, oracle_weights) for base in CORRUPT_BASES}
    assert all(r > 0 for r, _ in got.values()), got
    for base in ("xrans1-one-chain", "xrans1-two-chains"):
        assert got[base][1] > 0, got
