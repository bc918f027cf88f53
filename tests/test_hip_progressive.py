"""Progressive records on the device: HipCodec.level_cuts / pack_progressive / unpack_progressive against tests/ref_progressive.py and the
cursors of tests/ref_rans.py (CDF rows from the HIP kernels), the prefixes alone uploaded and decoded, malformed records, alignments, chunks,
offsets past 4 GiB, a caller's stream, the counters, the model with a `.llpa` file, and the CLI.  Run with -m gpu on an MI355X."""
import os
import sys

import numpy as np
import pytest

import ref_progressive as rp
import ref_rans as rr
from conftest import GOLDEN, load_state_dict
from helpers import DEV, GUARD, POISON, StreamGate, _dev, guarded, guards_intact, make_image          # noqa: F401
from test_hip_ref_rans import HipPlanes, _segs

pytestmark = pytest.mark.gpu
EFORMAT = -5
sys.path.insert(0, GOLDEN)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _new_codec(wname):
    from llicti_amd.codec import HipCodec
    c = HipCodec(DEV)
    if wname.startswith("b_"):
        c.set_model(60, 2)
    c.load_state_dict(load_state_dict(wname))
    return c


@pytest.fixture(scope="module")
def codecs(torch_mod):
    cache = {}

    def get(wname):
        if wname not in cache:
            cache[wname] = _new_codec(wname)
        return cache[wname]
    yield get
    for c in cache.values():
        c.close()


def _mode(c, name, H, W):
    """The encoder mode of a container name.  "auto" is the size rule's xwide mode (MODE_RANS_AUTO: the encoder picks the count); an image
    too small for the rule to give it an xwide stream (below ~160 x 160: container "auto" codes it in 64 lanes, which level_cuts refuses --
    test_cuts_pack_and_prefixes holds that) takes the rule's smallest, MODE_RANS_AUTO(1)."""
    from llicti_amd import codec as cd
    if name != "auto":
        return cd.mode_of_name(name)
    return cd.MODE_RANS_AUTO(max(1, cd.image_streams(H, W, c.nlevels)))


class Built:
    pass


_BUILT = {}


def built(torch, c, wname, sizes, names, kind=None, ref=True):
    """One encoded batch and everything the tests compare against, computed once: images, device containers, the modes the headers name, the
    device's cuts, ref_rans' cursors, the plain and the reference's progressive records."""
    key = (wname, tuple(sizes), tuple(names), None if kind is None else tuple(kind), ref)
    if key in _BUILT:
        return _BUILT[key]
    from llicti_amd import fileio
    from llicti_amd.codec import container_to_bytestream_list
    b = Built()
    kinds = kind if kind is not None else ["smooth" if "trained" in wname else "noise"] * len(sizes)
    b.imgs = [make_image(k, h, w, 50 + i) for i, ((h, w), k) in enumerate(zip(sizes, kinds))]
    b.Hs, b.Ws = [h for h, _ in sizes], [w for _, w in sizes]
    enc_modes = [_mode(c, n, h, w) for n, (h, w) in zip(names, sizes)]
    b.cont, b.seg = c.encode_v(_dev(torch, np.concatenate([im.reshape(-1) for im in b.imgs])), b.Hs, b.Ws, enc_modes if len(set(enc_modes)) > 1 else enc_modes[0])
    c.check()
    b.modes = c.container_modes(b.cont)
    b.cuts = c.level_cuts(b.cont, b.seg, b.Hs, b.Ws, b.modes)
    c.check()
    assert (c.image_status(len(sizes)) == 0).all()
    cont_np, seg_np = b.cont.cpu().numpy(), b.seg.cpu().numpy()
    b.S = [int(seg_np[i].sum()) for i in range(len(sizes))]
    b.plain = [fileio.dumps_llic(container_to_bytestream_list(cont_np[i], seg_np[i], nlevels=c.nlevels)) for i in range(len(sizes))]
    L = c.nlevels
    cuts_np = b.cuts.cpu().numpy()
    b.M = [rr.parse_header(int(cont_np[i, 0]), int(cont_np[i, 15]) | (int(cont_np[i, 16]) << 8))["M"] for i in range(len(sizes))]
    b.dev_cuts = [[tuple(int(v) for v in cuts_np[i, m, 1:L]) for m in range(b.M[i])] for i in range(len(sizes))]
    for i in range(len(sizes)):
        assert not cuts_np[i, b.M[i]:].any() and not cuts_np[i, :, 0].any() and not cuts_np[i, :, L:].any()
    if ref:
        b.ref_cuts = []
        for i in range(len(sizes)):
            segs = _segs(b.cont[i], b.seg[i])[:4 + 9 * L]
            b.ref_cuts.append(rp.ref_cuts(segs, HipPlanes(segs, c, torch).rows)[0])
    b.rec = [rp.to_progressive(p, cu) for p, cu in zip(b.plain, b.ref_cuts if ref else b.dev_cuts)]
    _BUILT[key] = b
    return b


def unpack_prefixes(torch, c, b, reds, stride=None, offset=0, cont_offset=0):
    """Uploads ONLY the prefixes P_{r_b} back to back and unpacks them into POISON-filled, guarded containers -> (cont view [B, stride], seg, buffers)"""
    pre = [rec[:rp.prefixes(rec)[r]] for rec, r in zip(b.rec, reds)]
    ro = np.concatenate(([0], np.cumsum([len(p) for p in pre]))).astype(np.int64)
    bbuf, blob, bbase = guarded(torch, int(ro[-1]), offset)
    blob.copy_(_dev(torch, np.frombuffer(b"".join(pre), np.uint8)))
    stride = stride or (max(b.S) + 15) // 16 * 16
    B = len(pre)
    cbuf, cflat, cbase = guarded(torch, B * stride, cont_offset)
    out = cflat.view(B, stride)
    seg = torch.full((B, 49), -3, dtype=torch.int32, device=DEV)
    c.unpack_progressive(blob, ro, reduce=list(reds), out=out, seg_len=seg)
    return out, seg, (bbuf, bbase, int(ro[-1]), cbuf, cbase, B * stride)


def expect_unpacked(b, reds, stride):
    """The reference's containers: the delivered bytes at their places, POISON everywhere else"""
    want = np.full((len(reds), stride), POISON, np.uint8)
    for i, r in enumerate(reds):
        pay, sl, mask = rp.from_progressive(b.rec[i][:rp.prefixes(b.rec[i])[r]], r, fill=POISON)
        want[i, :len(pay)] = pay
    return want


def decoded(torch, c, cont, seg, b, reds):
    c.poison_workspace()
    flat = c.decode_v(cont, seg, b.Hs, b.Ws, b.modes if len(set(b.modes)) > 1 else b.modes[0], reduce=list(reds)).cpu().numpy()
    out, pos = [], 0
    for h, w, r in zip(b.Hs, b.Ws, reds):
        hr, wr = -(-h // (1 << r)), -(-w // (1 << r))
        out.append(flat[pos:pos + 3 * hr * wr].reshape(3, hr, wr))
        pos += 3 * hr * wr
    return out


# ------------------------------------------------------------------------------------------------ 1. the frozen vectors
def test_cuts_and_records_equal_the_frozen_vectors(torch_mod, codecs):
    import make_progressive_vectors as mk
    torch = torch_mod
    vec = np.load(os.path.join(GOLDEN, "progressive_vectors.npz"))
    for key, (model, wname, M) in mk.CASES.items():
        c = codecs(wname if model == "A" else "b_" + wname)
        img = mk.image(key)
        H, W = img.shape[1:]
        from llicti_amd.codec import MODE_RANS
        cont, seg = c.encode(_dev(torch, img[None]), mode=MODE_RANS(M, wide=2))
        c.check()
        S = int(seg.sum().item())
        assert cont[0, :S].cpu().numpy().tobytes() == vec[f"{key}_bytes"].tobytes(), key          # the HIP encoder reproduces the container
        cuts = c.level_cuts(cont, seg, [H], [W], MODE_RANS(M, wide=2))
        c.check()
        assert (c.image_status(1) == 0).all()
        L = c.nlevels
        assert np.array_equal(cuts[0, :M, 1:L].cpu().numpy(), vec[f"{key}_cuts"]), key
        blob, ro, pre = c.pack_progressive(cont, seg, cuts)
        c.check()
        rec = vec[f"{key}_record"].tobytes()
        assert ro.tolist() == [0, len(rec)] and blob[:len(rec)].cpu().numpy().tobytes() == rec, key
        assert pre[0, :L + 1].tolist() == rp.prefixes(rec) and not pre[0, L + 1:].any()


# ------------------------------------------------------------------------------------------------ 2. every shape, mode and weight set
SHAPES = [(67, 93), (96, 128), (33, 40)]
MODES = ["xrans1", "xrans3", "auto", "xrans64", "xrans128"]
CASES = [(w, s, m) for w in ("trainedlike", "rand1337") for s in SHAPES for m in MODES]


@pytest.mark.parametrize("wname,size,name", CASES, ids=[f"{w}-{s[0]}x{s[1]}-{m}" for w, s, m in CASES])
def test_cuts_pack_and_prefixes(torch_mod, codecs, wname, size, name):
    torch = torch_mod
    c = codecs(wname)
    if name == "auto":
        from llicti_amd import codec as cd
        from llicti_amd._lib import EINVAL, LlictiError
        small = cd.image_mode(size[0], size[1])
        if (small >> 8) & 0xFF != 5:                                             # container "auto" of this size is not xwide: refused, nothing launched
            img = _dev(torch, make_image("smooth", size[0], size[1], 50)[None])
            cont, seg = c.encode(img, mode=small)
            c.check()
            with pytest.raises(LlictiError) as e:
                c.level_cuts(cont, seg, [size[0]], [size[1]], small)
            assert e.value.code == EINVAL
    b = built(torch, c, wname, [size], [name])
    L = c.nlevels
    assert b.dev_cuts == b.ref_cuts                                              # level_cuts == ref_rans' cursors >> 3
    # pack: the reference's record byte for byte, offsets and prefix table; nothing past rec_off[B]
    rec = b.rec[0]
    buf, blob, base = guarded(torch, len(rec) + 100)
    ro = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    pre = torch.full((1, 6), -7, dtype=torch.int64, device=DEV)
    c.pack_progressive(b.cont, b.seg, b.cuts, out=blob, rec_off=ro, prefix=pre)
    c.check()
    assert (c.image_status(1) == 0).all()
    assert ro.tolist() == [0, len(rec)] and blob[:len(rec)].cpu().numpy().tobytes() == rec
    assert bool((blob[len(rec):] == POISON).all()) and guards_intact(buf, base, len(rec) + 100)
    assert pre[0].tolist() == rp.prefixes(rec)
    from llicti_amd import progressive as pg
    assert pg.to_llic(rec) == b.plain[0]
    # unpack, r = 0 ... L: only the prefix is uploaded; delivered bytes at their places, everything else (bytes >= S too) still POISON
    stride = (b.S[0] + 15) // 16 * 16 + 32
    for r in range(L + 1):
        out, seg, (bbuf, bbase, bn, cbuf, cbase, cn) = unpack_prefixes(torch, c, b, [r], stride=stride)
        c.check()
        assert (c.image_status(1) == 0).all()
        assert np.array_equal(out.cpu().numpy(), expect_unpacked(b, [r], stride)), r
        assert np.array_equal(seg.cpu().numpy(), b.seg.cpu().numpy())
        assert guards_intact(bbuf, bbase, bn) and guards_intact(cbuf, cbase, cn)
        if r == 0:
            assert torch.equal(out[0, :b.S[0]], b.cont[0, :b.S[0]])
        got = decoded(torch, c, out, seg, b, [r])[0]
        c.check()
        assert (c.image_status(1) == 0).all(), r
        assert np.array_equal(got, b.imgs[0][:, ::1 << r, ::1 << r]), r


def test_mixed_batch_mixed_reduces_and_a_fresh_context(torch_mod, codecs):
    torch = torch_mod
    sizes, names = [(67, 93), (96, 128), (33, 40), (64, 96)], ["xrans3", "auto", "xrans1", "xrans2"]
    c = codecs("trainedlike")
    b = built(torch, c, "trainedlike", sizes, names, kind=["smooth", "noise", "smooth", "noise"])
    assert b.dev_cuts == b.ref_cuts
    B = len(sizes)
    total = sum(len(r) for r in b.rec)
    buf, blob, base = guarded(torch, total + 64)
    blob2, ro, pre = c.pack_progressive(b.cont, b.seg, b.cuts, out=blob)
    c.check()
    assert blob[:total].cpu().numpy().tobytes() == b"".join(b.rec) and guards_intact(buf, base, total + 64) and bool((blob[total:] == POISON).all())
    assert ro.tolist() == np.concatenate(([0], np.cumsum([len(r) for r in b.rec]))).tolist()
    assert [row[:6] for row in pre.tolist()] == [rp.prefixes(r) for r in b.rec]
    stride = (max(b.S) + 15) // 16 * 16
    fresh = _new_codec("trainedlike")
    try:
        for cc, reds in ((c, [2, 0, 5, 1]), (c, [0, 3, 1, 4]), (fresh, [1, 2, 0, 3])):
            out, seg, (bbuf, bbase, bn, cbuf, cbase, cn) = unpack_prefixes(torch, cc, b, reds)
            cc.check()
            assert (cc.image_status(B) == 0).all()
            assert np.array_equal(out.cpu().numpy(), expect_unpacked(b, reds, stride))
            assert guards_intact(bbuf, bbase, bn) and guards_intact(cbuf, cbase, cn)
            for got, im, r in zip(decoded(torch, cc, out, seg, b, reds), b.imgs, reds):
                assert np.array_equal(got, im[:, ::1 << r, ::1 << r])
            cc.check()
            assert (cc.image_status(B) == 0).all()
    finally:
        fresh.close()


def test_config_b(torch_mod, codecs):
    torch = torch_mod
    c = codecs("b_rand1337")
    b = built(torch, c, "b_rand1337", [(40, 33)], ["xrans3"])
    assert c.nlevels == 2 and b.dev_cuts == b.ref_cuts and len(b.dev_cuts[0][0]) == 1
    blob, ro, pre = c.pack_progressive(b.cont, b.seg, b.cuts)
    c.check()
    assert blob[:int(ro[1])].cpu().numpy().tobytes() == b.rec[0] and pre[0].tolist() == rp.prefixes(b.rec[0]) + [0, 0, 0]
    for r in range(3):
        out, seg, _ = unpack_prefixes(torch, c, b, [r])
        c.check()
        assert np.array_equal(out.cpu().numpy(), expect_unpacked(b, [r], out.shape[1]))
        assert np.array_equal(decoded(torch, c, out, seg, b, [r])[0], b.imgs[0][:, ::1 << r, ::1 << r])
        c.check()
        assert (c.image_status(1) == 0).all()
    # a config A record is not this context's
    a = built(torch, codecs("rand1337"), "rand1337", [(33, 40)], ["xrans1"])
    out, seg, _ = unpack_prefixes(torch, c, a, [0])
    with pytest.raises(Exception):
        c.check()
    assert c.image_status(1)[0] == EFORMAT and not seg.any() and bool((out == POISON).all())


def test_more_images_than_one_launch_of_the_unpack(torch_mod, codecs):
    """B = 1025: five rounds of the pack's offset scan (256 images each, the last of one) and two launches of the unpack kernels (1024 images'
    reduces travel with a launch, the second carries ONE).  One config B container tiled on the device with its cuts, reduces cycling
    0 .. L: every record and every unpacked container against the single image's, the offsets against the cumulative sizes."""
    torch = torch_mod
    c = codecs("b_rand1337")
    b = built(torch, c, "b_rand1337", [(40, 33)], ["xrans3"])
    B, L, rec = 1025, c.nlevels, b.rec[0]
    stride = (b.S[0] + 15) // 16 * 16
    blob, ro, pre = c.pack_progressive(b.cont[:, :stride].repeat(B, 1), b.seg.repeat(B, 1), b.cuts.repeat(B, 1, 1))
    c.check()
    assert (c.image_status(B) == 0).all()
    assert ro.tolist() == [len(rec) * k for k in range(B + 1)] and pre.tolist() == [rp.prefixes(rec) + [0, 0, 0]] * B
    assert torch.equal(blob[:B * len(rec)].view(B, len(rec)), _dev(torch, np.frombuffer(rec, np.uint8)).expand(B, -1))
    reds = [k % (L + 1) for k in range(B)]
    assert reds[1022:] == [2, 0, 1]                                          # images 1023, 1024 and 1025: one on either side of the launch boundary
    cuts_at = rp.prefixes(rec)
    ro_h = np.concatenate(([0], np.cumsum([cuts_at[r] for r in reds]))).astype(np.int64)
    cbuf, cflat, cbase = guarded(torch, B * stride, 5)
    out = cflat.view(B, stride)
    seg = torch.full((B, 49), -3, dtype=torch.int32, device=DEV)
    c.unpack_progressive(_dev(torch, np.frombuffer(b"".join(rec[:cuts_at[r]] for r in reds), np.uint8)), ro_h, reduce=reds, out=out, seg_len=seg)
    c.check()
    assert (c.image_status(B) == 0).all() and guards_intact(cbuf, cbase, B * stride)
    want = np.stack([expect_unpacked(b, [r], stride)[0] for r in range(L + 1)])          # the single image at each reduce
    assert len({w.tobytes() for w in want}) == L + 1
    assert torch.equal(out, _dev(torch, want)[torch.tensor(reds, device=DEV)]) and torch.equal(seg, b.seg.expand(B, -1))
    for k in (1022, 1023, 1024):
        assert np.array_equal(out[k].cpu().numpy(), want[reds[k]]), k


# ------------------------------------------------------------------------------------------------ 3. what is refused
def test_pack_refuses_cuts_that_overlap_another_buffer(torch_mod, codecs):
    """All buffers of a record call are pairwise disjoint: d_cuts over d_rec_off, the containers or the segment lengths is LLICTI_EINVAL
    before anything is launched -- the error names both, and the poisoned outputs stay as they were."""
    import ctypes as C
    torch = torch_mod
    from llicti_amd._lib import EINVAL
    c = codecs("trainedlike")
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    B, cuts_bytes = 2, 2 * 128 * 5 * 4
    # one arena, so that what lies next to every buffer is known: at least cuts_bytes of nobody's bytes in front of seg_len and rec_off
    at = dict(cont=0, seg=24576, ro=32768, blob=36864, pre=40960, cuts=45056)
    arena = torch.full((51200,), POISON, dtype=torch.uint8, device=DEV)
    arena[at["seg"]:at["seg"] + 4 * 49 * B] = 0
    before = arena.clone()
    p = lambda name, off=0: C.c_void_p(arena.data_ptr() + at[name] + off)
    err = lambda: c.L.llicti_last_error().decode()

    def pack(cuts, ro=p("ro"), pre=p("pre")):
        return c.L.llicti_pack_progressive(c.ctx, p("cont"), 8192, p("seg"), B, cuts, p("blob"), 4096, ro, pre, s)
    assert pack(p("ro", 8 - cuts_bytes)) == EINVAL and "the cuts" in err() and "the record offsets" in err()       # the cuts' last 8 bytes are d_rec_off[0]
    assert pack(p("cont", 4096)) == EINVAL and "the cuts" in err() and "the containers" in err()
    assert pack(p("seg", 4 - cuts_bytes)) == EINVAL and "the cuts" in err() and "the segment lengths" in err()
    assert pack(p("cuts"), pre=p("ro", 16)) == EINVAL and "the prefix table" in err() and "the record offsets" in err()      # (refused before, too)
    torch.cuda.synchronize()
    c.check()
    assert torch.equal(arena, before)
    assert pack(p("cuts")) == 0                                              # the same call with disjoint buffers is admitted
    with pytest.raises(Exception):
        c.check()                                                            # (all-zero length rows: no records, EFORMAT)
    ro = arena[at["ro"]:at["ro"] + 8 * (B + 1)].view(torch.int64)
    assert c.image_status(B).tolist() == [EFORMAT, EFORMAT] and ro.tolist() == [0, 0, 0] and torch.equal(arena[at["blob"]:at["blob"] + 4096], before[at["blob"]:at["blob"] + 4096])


# ------------------------------------------------------------------------------------------------ 3b. level_cuts
def test_level_cuts_refuses_other_containers_and_flags_a_corrupt_one_alone(torch_mod, codecs):
    torch = torch_mod
    from llicti_amd._lib import EINVAL, LlictiError
    from llicti_amd.codec import MODE_AC, MODE_RANS
    c = codecs("trainedlike")
    img = _dev(torch, make_image("smooth", 64, 96, 3)[None])
    for mode in (MODE_AC, MODE_RANS(4), MODE_RANS(3, wide=1)):
        cont, seg = c.encode(img, mode=mode)
        c.check()
        with pytest.raises(LlictiError) as e:
            c.level_cuts(cont, seg, [64], [96], mode)
        assert e.value.code == EINVAL
    b = built(torch, c, "trainedlike", [(67, 93), (67, 93), (67, 93)], ["xrans3"] * 3, ref=False)
    bad = b.cont.clone()
    off = int(b.seg[1, :4].sum().item())
    # image 1's stream 0 (segment 4) loses its end marker: an xwide stream is its bit region, then the 256 lanes' states of 31 bits each
    # (ref_rans.Stream), and a region whose last byte is zero has no marker
    hdr = rr.parse_header(int(b.cont[1, 0]), int(b.cont[1, 15]) | (int(b.cont[1, 16]) << 8))
    state_bytes = rr.STATE_BITS * hdr["L"] // 8
    stream_len = int(b.seg[1, 4].item())
    assert hdr["layout"] == "v4" and hdr["per_seg"] == 1 and stream_len > state_bytes
    bad[1, off + stream_len - state_bytes - 1] = 0
    cuts = c.level_cuts(bad, b.seg, b.Hs, b.Ws, b.modes)
    with pytest.raises(LlictiError):
        c.check()
    st = c.image_status(3)
    assert st[0] == 0 and st[1] == EFORMAT and st[2] == 0
    assert torch.equal(cuts[0], b.cuts[0]) and torch.equal(cuts[2], b.cuts[2])
    # ... and pack refuses an image whose cuts do not hold together, alone
    cuts2 = b.cuts.clone()
    cuts2[1, 0, 2] = cuts2[1, 0, 1] - 1 if int(cuts2[1, 0, 1]) > 0 else 10 ** 8
    blob, ro, pre = c.pack_progressive(b.cont, b.seg, cuts2)
    with pytest.raises(LlictiError):
        c.check()
    assert c.image_status(3).tolist() == [0, EFORMAT, 0]
    n = [len(r) for r in b.rec]
    assert ro.tolist() == [0, n[0], n[0], n[0] + n[2]] and not pre[1].any()
    assert blob[:n[0] + n[2]].cpu().numpy().tobytes() == b.rec[0] + b.rec[2]
    # a blob too small: ENOSPACE, the total it needs, nothing past the capacity
    buf, small, base = guarded(torch, n[0] + 10)
    _, ro2, _ = c.pack_progressive(b.cont, b.seg, b.cuts, out=small)
    with pytest.raises(LlictiError) as e:
        c.check()
    assert e.value.code == -4 and int(ro2[3]) == sum(n) and guards_intact(buf, base, n[0] + 10)
    assert small[:n[0]].cpu().numpy().tobytes() == b.rec[0] and bool((small[n[0]:] == POISON).all())


def test_malformed_records(torch_mod, codecs):
    """Each malformed case between two good neighbours: EFORMAT for that image, a zero row, its container untouched, the guards of blob and
    containers unchanged; the neighbours unpack and decode."""
    torch = torch_mod
    from llicti_amd._lib import LlictiError
    c = codecs("trainedlike")
    b = built(torch, c, "trainedlike", [(67, 93), (67, 93), (67, 93)], ["xrans3"] * 3, ref=False)
    good, S = b.rec[0], b.S[0]
    stride = (max(b.S) + 15) // 16 * 16
    cases = rp.malformed_cases(b.rec[1])
    assert len(cases) >= 21
    for name, bad, kw in cases:
        recs, reds, st = [good, bad, b.rec[2]], [0, kw.get("r", 0), 0], stride
        ro = np.concatenate(([0], np.cumsum([len(r) for r in recs]))).astype(np.int64)
        bbuf, blob, bbase = guarded(torch, int(ro[-1]), 3)
        blob.copy_(_dev(torch, np.frombuffer(b"".join(recs), np.uint8)))
        if name == "S>stride":                                                 # (the stride a call gives holds for all its images: image 1 alone here)
            recs, reds, ro = [bad], [0], np.array([len(good), len(good) + len(bad)], np.int64)
            st = kw["stride"]
        B = len(recs)
        cbuf, cflat, cbase = guarded(torch, B * st, 5)
        out = cflat.view(B, st)
        seg = torch.full((B, 49), -3, dtype=torch.int32, device=DEV)
        c.unpack_progressive(blob, ro, reduce=reds, out=out, seg_len=seg)
        with pytest.raises(LlictiError) as e:
            c.check()
        assert e.value.code == EFORMAT, name
        k = B // 2
        status = c.image_status(B)
        assert status[k] == EFORMAT and not seg[k].any() and bool((out[k] == POISON).all()), name
        assert guards_intact(bbuf, bbase, int(ro[-1]) if B == 3 else len(good) + len(bad) + len(b.rec[2])) and guards_intact(cbuf, cbase, B * st), name
        if B == 3:
            assert status[0] == 0 and status[2] == 0 and torch.equal(out[0, :S], b.cont[0, :S]) and torch.equal(out[2, :b.S[2]], b.cont[2, :b.S[2]]), name
    # the neighbours of the last case decode
    keep = torch.tensor([0, 2], device=DEV)
    flat = c.decode_v(out[keep].contiguous(), seg[keep].contiguous(), [67, 67], [93, 93], b.modes[0]).cpu().numpy().reshape(2, 3, 67, 93)
    c.check()
    assert np.array_equal(flat[0], b.imgs[0]) and np.array_equal(flat[1], b.imgs[2])
    # offsets that leave the blob, descend or are negative
    for ro in ([0, len(good) + 10 ** 6], [len(good), 0], [-5, len(good)]):
        blob = _dev(torch, np.frombuffer(good, np.uint8))
        out = torch.full((1, stride), POISON, dtype=torch.uint8, device=DEV)
        seg = torch.full((1, 49), -3, dtype=torch.int32, device=DEV)
        c.unpack_progressive(blob, np.array(ro, np.int64), reduce=0, out=out, seg_len=seg)
        with pytest.raises(LlictiError):
            c.check()
        assert c.image_status(1)[0] == EFORMAT and not seg.any() and bool((out == POISON).all())


# ------------------------------------------------------------------------------------------------ 4. alignment, chunks, large offsets
def test_all_alignments(torch_mod, codecs):
    torch = torch_mod
    c = codecs("trainedlike")
    b = built(torch, c, "trainedlike", [(67, 93), (33, 40)], ["xrans3", "xrans1"], ref=False)
    reds = [1, 0]
    stride = (max(b.S) + 15) // 16 * 16 + 16
    want = expect_unpacked(b, reds, stride)
    for bo in range(16):
        for co in range(16):
            out, seg, (bbuf, bbase, bn, cbuf, cbase, cn) = unpack_prefixes(torch, c, b, reds, stride=stride, offset=bo, cont_offset=co)
            assert np.array_equal(out.cpu().numpy(), want), (bo, co)
            assert guards_intact(bbuf, bbase, bn) and guards_intact(cbuf, cbase, cn), (bo, co)
    total = sum(len(r) for r in b.rec)
    for bo in range(16):
        buf, blob, base = guarded(torch, total, bo)
        c.pack_progressive(b.cont, b.seg, b.cuts, out=blob)
        assert blob.cpu().numpy().tobytes() == b"".join(b.rec) and guards_intact(buf, base, total), bo
    c.check()


def test_pieces_of_several_chunks(torch_mod, codecs):
    """256 x 384 noise in one stream: a record of ~300 KB whose level-0 piece alone spans several LLICTI_RECORD_CHUNK ranges"""
    torch = torch_mod
    from llicti_amd._lib import RECORD_CHUNK
    c = codecs("rand1337")
    b = built(torch, c, "rand1337", [(256, 384), (67, 93)], ["xrans1", "xrans3"], ref=False)
    pre = rp.prefixes(b.rec[0])
    assert pre[0] - pre[1] > 3 * RECORD_CHUNK and pre[1] - pre[2] > RECORD_CHUNK
    blob, ro, p = c.pack_progressive(b.cont, b.seg, b.cuts)
    c.check()
    assert blob[:int(ro[2])].cpu().numpy().tobytes() == b"".join(b.rec)
    for reds in ([0, 0], [1, 2], [2, 0]):
        out, seg, (bbuf, bbase, bn, cbuf, cbase, cn) = unpack_prefixes(torch, c, b, reds)
        c.check()
        assert np.array_equal(out.cpu().numpy(), expect_unpacked(b, reds, out.shape[1])), reds
        assert guards_intact(bbuf, bbase, bn) and guards_intact(cbuf, cbase, cn)
        for got, im, r in zip(decoded(torch, c, out, seg, b, reds), b.imgs, reds):
            assert np.array_equal(got, im[:, ::1 << r, ::1 << r])
        c.check()


def test_a_record_past_4_gib(torch_mod, codecs):
    torch = torch_mod
    c = codecs("trainedlike")
    b = built(torch, c, "trainedlike", [(67, 93), (33, 40)], ["xrans3", "xrans1"], ref=False)
    at = (1 << 32) + 12345
    pre = [b.rec[0][:rp.prefixes(b.rec[0])[1]], b.rec[1]]
    blob = torch.empty((at + len(b.rec[0]) + len(pre[1]) + 7,), dtype=torch.uint8, device=DEV)
    blob[:len(pre[1])] = _dev(torch, np.frombuffer(pre[1], np.uint8))
    blob[at:at + len(pre[0])] = _dev(torch, np.frombuffer(pre[0], np.uint8))
    blob[at + len(pre[0]):] = POISON
    # rec_off need not ascend between records: image 0 sits past 4 GiB, image 1 at the blob's start -- two calls, one offset pair each
    stride = (max(b.S) + 15) // 16 * 16
    want = expect_unpacked(b, [1, 0], stride)
    for i, ro in ((0, [at, at + len(pre[0])]), (1, [0, len(pre[1])])):
        out = torch.full((1, stride), POISON, dtype=torch.uint8, device=DEV)
        _, seg = c.unpack_progressive(blob, np.array(ro, np.int64), reduce=[1, 0][i], out=out)
        c.check()
        assert np.array_equal(out[0].cpu().numpy(), want[i]) and np.array_equal(seg[0].cpu().numpy(), b.seg[i].cpu().numpy())
    # ... and packed there
    big = blob
    cont1 = b.cont[:1].contiguous()
    _, ro, pre = c.pack_progressive(cont1, b.seg[:1].contiguous(), b.cuts[:1].contiguous(), out=big[at - 5:at - 5 + len(b.rec[0])])
    assert ro.tolist() == [0, len(b.rec[0])] and pre[0].tolist() == rp.prefixes(b.rec[0])
    c.check()
    assert big[at - 5:at - 5 + len(b.rec[0])].cpu().numpy().tobytes() == b.rec[0]


# ------------------------------------------------------------------------------------------------ 5. streams and counters
def test_on_a_callers_stream_behind_a_gate(torch_mod, codecs):
    """The three calls on a side stream whose inputs arrive BEHIND a gate on that stream: a call issued on another stream reads the decoys."""
    torch = torch_mod
    c = codecs("trainedlike")
    b = built(torch, c, "trainedlike", [(67, 93), (33, 40)], ["xrans3", "xrans1"], ref=False)
    reds = [1, 0]
    pre = [rec[:rp.prefixes(rec)[r]] for rec, r in zip(b.rec, reds)]
    ro = np.concatenate(([0], np.cumsum([len(p) for p in pre]))).astype(np.int64)
    stride = (max(b.S) + 15) // 16 * 16
    gate = StreamGate(torch, DEV)
    s = torch.cuda.Stream(device=DEV)
    cont_in, seg_in = torch.zeros_like(b.cont), torch.zeros_like(b.seg)          # the decoys
    blob_in = torch.zeros((int(ro[-1]),), dtype=torch.uint8, device=DEV)
    blob_real = _dev(torch, np.frombuffer(b"".join(pre), np.uint8))
    ro_d = _dev(torch, ro)
    out = torch.full((2, stride), POISON, dtype=torch.uint8, device=DEV)
    with torch.cuda.stream(s):                                                 # (an ungated pass: the first use of a kernel loads its code)
        c.unpack_progressive(blob_real, ro_d, reduce=reds, out=out.clone())
        c.pack_progressive(b.cont, b.seg, c.level_cuts(b.cont, b.seg, b.Hs, b.Ws, b.modes))
    torch.cuda.synchronize()
    c.check()
    begin, end = gate.hold(s, 80)
    with torch.cuda.stream(s):
        cont_in.copy_(b.cont, non_blocking=True)
        seg_in.copy_(b.seg, non_blocking=True)
        blob_in.copy_(blob_real, non_blocking=True)
        cuts = c.level_cuts(cont_in, seg_in, b.Hs, b.Ws, b.modes)
        packed, pro, ppre = c.pack_progressive(cont_in, seg_in, cuts)
        got, seg = c.unpack_progressive(blob_in, ro_d, reduce=reds, out=out)
    assert end.query() is False, "the gate ran out before everything was enqueued: the run shows nothing"
    s.synchronize()
    c.check()
    total = sum(len(r) for r in b.rec)
    assert torch.equal(cuts, b.cuts) and packed[:total].cpu().numpy().tobytes() == b"".join(b.rec)
    assert np.array_equal(got.cpu().numpy(), expect_unpacked(b, reds, stride))


def test_warm_calls_neither_synchronise_nor_allocate(torch_mod, codecs):
    torch = torch_mod
    c = codecs("trainedlike")
    b = built(torch, c, "trainedlike", [(67, 93), (33, 40)], ["xrans3", "xrans1"], ref=False)
    c.level_cuts(b.cont, b.seg, b.Hs, b.Ws, b.modes)
    before = {k: c.counter(k) for k in ("device_syncs", "device_allocs")}
    cuts = c.level_cuts(b.cont, b.seg, b.Hs, b.Ws, b.modes)
    blob, ro, pre = c.pack_progressive(b.cont, b.seg, cuts)
    out, seg = c.unpack_progressive(blob, ro, reduce=[5, 0], stride=(max(b.S) + 15) // 16 * 16)
    c.check()
    assert {k: c.counter(k) for k in before} == before
    # (the output it made itself: image 0 holds its header alone, and its row must not trip the decoders' stream parser)
    got = decoded(torch, c, out, seg, b, [5, 0])
    c.check()
    assert (c.image_status(2) == 0).all()
    assert np.array_equal(got[0], b.imgs[0][:, ::32, ::32]) and np.array_equal(got[1], b.imgs[1])


# ------------------------------------------------------------------------------------------------ 6. the model, a file, the CLI
def test_through_the_model_and_a_file(torch_mod, tmp_path):
    torch = torch_mod
    from llicti_amd import archive, codec as cd, progressive as pg
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    m = LLICTI(default_config(container="auto")).to(DEV).eval()
    sizes = [(160, 176), (192, 160), (176, 176), (224, 160)]                       # (large enough for container "auto" to give xwide streams)
    rgbs = [make_image("smooth", h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    enc = m.encode_batch_async(rgbs)
    blob, rec_off = enc.records()
    pblob, prec_off, prefix = enc.records(progressive=True)
    recs = [bytes(pblob[int(prec_off[i]):int(prec_off[i + 1])]) for i in range(4)]
    for i in range(4):
        assert pg.to_llic(recs[i]) == bytes(blob[int(rec_off[i]):int(rec_off[i + 1])])
        assert [int(v) for v in prefix[i]] == rp.prefixes(recs[i])
    pa, pp = str(tmp_path / "m.llia"), str(tmp_path / "m.llpa")
    with archive.ArchiveWriter(pa, m.codec().nseg) as aw:
        aw.append_records(blob, rec_off, list("abcd"))
    with pg.ProgressiveWriter(pp, m.codec().nseg) as pw:
        pw.append_records(pblob, prec_off, list("abcd"))
    order = [2, 0, 3, 1, 0]
    boxes_full = [(3, 8, 60, 70), (16, 32, 128, 96), (0, 0, 128, 128), (10, 20, 80, 100), (40, 8, 100, 120)]
    reds, boxes = cd.resized_crop_plan([sizes[i] for i in order], boxes_full, (24, 20), per_image=True)
    assert len(set(reds)) > 1
    tensor = dict(size=(24, 20), boxes=boxes, flip=[0, 1, 0, 1, 0], mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), dtype=torch.float16)
    with archive.ArchiveReader(pa) as ar, pg.ProgressiveReader(pp) as pr:
        assert pr.sizes == ar.sizes and pr.modes == ar.modes
        want = m.decode_batch_async(ar.read_batch(order), reduce=reds, tensor=dict(tensor))
        m.codec().check()
        pbatch = pr.read_batch(order, reduce=reds)
        assert pbatch.blob.numel() == sum(rp.prefixes(recs[i])[r] for i, r in zip(order, reds)) < ar.read_batch(order).blob.numel()
        got = m.decode_batch_async(pbatch, tensor=dict(tensor))                       # reduce= defaults to the batch's
        m.codec().check()
        assert (m.codec().image_status(len(order)) == 0).all()
        assert got.dtype == want.dtype and torch.equal(got, want)                     # bit for bit the .llia path's tensor
        coarser = [min(r + 1, 5) for r in reds]
        flat, Hs, Ws = m.decode_batch_async(pbatch, reduce=coarser)
        m.codec().check()
        assert Hs == [-(-sizes[i][0] // (1 << r)) for i, r in zip(order, coarser)]
        if any(r > 0 for r in reds):
            with pytest.raises(ValueError):
                m.decode_batch_async(pbatch, reduce=[max(r - 1, 0) for r in reds], tensor=dict(tensor))
            with pytest.raises(ValueError):
                m.decode_batch_async(pbatch, reduce=0)
        full = pr.read_batch([1, 3])
        flat, Hs, Ws = m.decode_batch_async(full, flat=True)
        m.codec().check()
        offs, _ = m.codec().flat_offsets(Hs, Ws)
        for o, h, w, i in zip(offs, Hs, Ws, (1, 3)):
            assert np.array_equal(flat[int(o):int(o) + 3 * h * w].view(3, h, w).cpu().numpy(), rgbs[i])


def test_cli_pack_info_unpack_round_trip(torch_mod, tmp_path, capsys):
    from llicti_amd import cli, fileio, progressive as pg
    sizes = [(160, 176), (168, 160), (160, 176)]
    rgbs = [make_image("smooth" if i != 1 else "noise", h, w, 60 + i) for i, (h, w) in enumerate(sizes)]
    srcs = []
    for i, r in enumerate(rgbs):
        srcs.append(str(tmp_path / f"img_{i}.ppm"))
        fileio.write_image(srcs[-1], r)
    arc, out, out2 = str(tmp_path / "set.llpa"), str(tmp_path / "out"), str(tmp_path / "out2")
    assert cli.main(["pack", "--progressive", arc] + srcs + ["--container", "rans4"]) == 2
    assert "--container auto" in capsys.readouterr().err
    assert cli.main(["pack", "--progressive", arc] + srcs + ["--container", "auto", "--batch", "2"]) == 0
    assert f"3 images -> {arc}" in capsys.readouterr().out
    with pg.ProgressiveReader(arc) as ar:
        assert ar.names == ["img_0", "img_1", "img_2"] and ar.sizes == sizes and ar.nseg == 49
        p1 = [int(v) for v in ar.prefix[1]]
    assert cli.main(["info", arc]) == 0
    text = capsys.readouterr().out
    assert "3 images, n = 49" in text and "img_1: 160x168" in text and ", ".join(f"P_{r}={v}" for r, v in enumerate(p1)) in text
    assert cli.main(["unpack", arc, out, "--as", "ppm"]) == 0
    for i, r in enumerate(rgbs):
        assert np.array_equal(fileio.read_image(os.path.join(out, f"img_{i}.ppm")), r), i
    assert cli.main(["unpack", arc, out2]) == 0                                    # .llic files, on the host
    capsys.readouterr()
    assert cli.main(["info", os.path.join(out2, "img_2.llic")]) == 0
    assert "176x160" in capsys.readouterr().out
