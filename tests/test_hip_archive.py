"""llicti_pack_records / llicti_unpack_records and the archive path on the GPU (run with -m gpu on an MI355X).  Every check is EXACT: the
yardsticks are fileio.dumps_llic (the file format the blob must equal), tests/ref_records.py (a numpy restatement of both calls, refusals and
what they leave behind included) and the original pixels.  Buffers the calls write are filled with 0xA5 first, with guard bytes on both sides;
the shapes are the smallest that reach each path: 32x32 and (33, 35) give payloads of a few kilobytes (one copy chunk, odd lengths), a 512x768
noise image more than three chunks."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_records as rr
from helpers import DEV, GUARD, POISON, _dev, guarded, guards_intact, make_image          # noqa: F401
from test_hip_streams import Run, codecs, env, torch_mod          # noqa: F401  (the gated queue and its fixtures; that file stays as it is)

pytestmark = pytest.mark.gpu

MIXED = [(32, 32), (33, 35), (67, 93), (64, 96)]


def _mode(name):
    from llicti_amd.codec import mode_of_name
    return mode_of_name(name)


_IMAGES, _ENC = {}, {}


def image(H, W, seed):
    key = (H, W, seed)
    if key not in _IMAGES:
        _IMAGES[key] = make_image("smooth" if seed % 2 == 0 else "noise", H, W, 7000 + seed)
    return _IMAGES[key]


def encoded(torch, c, wname, sizes, mode, seeds=None):
    """The batch's images and their device containers, computed once per (weights, sizes, mode): (imgs, cont, seg, cont_np, seg_np, modes)"""
    seeds = list(range(len(sizes))) if seeds is None else seeds
    key = (wname, tuple(sizes), str(mode), tuple(seeds))
    if key not in _ENC:
        imgs = [image(h, w, s) for (h, w), s in zip(sizes, seeds)]
        if mode == 0:
            cont, seg = c.encode(_dev(torch, np.stack(imgs)), mode=0)
        else:
            cont, seg = c.encode_v(_dev(torch, np.concatenate([im.reshape(-1) for im in imgs])), [h for h, _ in sizes], [w for _, w in sizes], mode)
        c.check()
        modes = c.container_modes(cont)
        _ENC[key] = (imgs, cont, seg, cont.cpu().numpy(), seg.cpu().numpy(), modes[0] if all(m == modes[0] for m in modes) else modes)
    return _ENC[key]


def llic_files(cont_np, seg_np, nlevels):
    from llicti_amd import fileio
    from llicti_amd.codec import container_to_bytestream_list
    return [fileio.dumps_llic(container_to_bytestream_list(cont_np[b], seg_np[b], nlevels=nlevels)) for b in range(len(cont_np))]


def decoded_images(torch, c, cont, seg, sizes, mode):
    Hs, Ws = [h for h, _ in sizes], [w for _, w in sizes]
    flat = c.decode_v(cont, seg, Hs, Ws, mode).cpu().numpy()
    offs, _ = c.flat_offsets(Hs, Ws)
    return [flat[int(o):int(o) + 3 * h * w].reshape(3, h, w) for o, (h, w) in zip(offs, sizes)]


# ------------------------------------------------------------------------------------------------ 1. pack equals the file format
PACK_CASES = [("trainedlike", MIXED, "xrans2"), ("trainedlike", MIXED, "auto"), ("trainedlike", [(67, 93)] * 3, "ac"), ("b_trainedlike", [(33, 40), (64, 96), (40, 33)], "xrans2")]


@pytest.mark.parametrize("wname,sizes,container", PACK_CASES, ids=[f"{w}-{k}-{len(s)}" for w, s, k in PACK_CASES])
def test_pack_equals_the_file_format_and_round_trips(torch_mod, codecs, wname, sizes, container):
    torch = torch_mod
    from llicti_amd import codec as cd
    c = codecs(wname)
    n = c.nseg
    assert n == (22 if wname.startswith("b_") else 49)
    mode = cd.auto_modes(sizes, c.nlevels) if container == "auto" else _mode(container)
    imgs, cont, seg, cont_np, seg_np, dmode = encoded(torch, c, wname, sizes, mode)
    B = len(sizes)
    files = llic_files(cont_np, seg_np, c.nlevels)
    want = b"".join(files)
    want_off = np.concatenate(([0], np.cumsum([len(f) for f in files])))
    for b in range(B):                       # the host helper agrees, for this context's n
        assert c.record_bytes(seg_np[b]) == len(files[b])
    buf, blob, base = guarded(torch, len(want) + 100)
    ro = torch.full((B + 1,), -7, dtype=torch.int64, device=DEV)
    before = {k: c.counter(k) for k in ("device_syncs", "device_allocs")}
    c.pack_records(cont, seg, out=blob, rec_off=ro)
    c.check()
    assert (c.image_status(B) == 0).all()
    ro_h = ro.cpu().numpy()
    assert list(ro_h) == list(want_off)
    assert blob[:len(want)].cpu().numpy().tobytes() == want                  # == b"".join(dumps_llic(...))
    assert bool((blob[len(want):] == POISON).all()) and guards_intact(buf, base, blob.numel())      # untouched from rec_off[B] on
    ref_blob, ref_off, ref_img, ref_st = rr.pack(cont_np, seg_np, n, np.full(blob.numel(), POISON, np.uint8))
    assert ref_st == 0 and np.array_equal(ref_off, ro_h) and np.array_equal(ref_blob, blob.cpu().numpy())
    # the default output (worst-case capacity) gives the same records
    blob2, ro2 = c.pack_records(cont, seg)
    assert torch.equal(ro2, ro) and torch.equal(blob2[:len(want)], blob[:len(want)])

    # ---- 2. round trip: tight default stride, exact seg_len rows, the containers' own bytes, the original pixels
    cont2, seg2 = c.unpack_records(blob[:len(want)], ro_h)
    c.check()
    assert (c.image_status(B) == 0).all()
    pay = max(len(f) for f in files) - (6 + 4 * n)
    assert cont2.shape == (B, (pay + 15) // 16 * 16) and cont2.shape[1] < cont.shape[1]
    seg2_np = seg2.cpu().numpy()
    assert np.array_equal(seg2_np, seg_np) and (seg2_np[:, n:] == 0).all()
    cont2_np = cont2.cpu().numpy()
    for b in range(B):
        m = int(seg_np[b].sum())
        assert np.array_equal(cont2_np[b, :m], cont_np[b, :m]), b
    # ... with device offsets and a given stride, into poisoned outputs: the numpy restatement to the byte (bytes past a payload stay)
    out = torch.full((B, cont2.shape[1] + 5), POISON, dtype=torch.uint8, device=DEV)
    sl = torch.full((B, 49), -7, dtype=torch.int32, device=DEV)
    c.unpack_records(blob[:len(want)], ro, out=out, seg_len=sl)
    c.check()
    ref_out, ref_seg, ref_img, _ = rr.unpack(np.frombuffer(want, np.uint8), ro_h, n, np.full(tuple(out.shape), POISON, np.uint8))
    assert np.array_equal(out.cpu().numpy(), ref_out) and np.array_equal(sl.cpu().numpy(), ref_seg)
    after = {k: c.counter(k) for k in before}
    assert after == before, "pack / unpack on a warm context neither synchronise the device nor allocate"
    for got, im in zip(decoded_images(torch, c, cont2, seg2, sizes, dmode), imgs):
        assert np.array_equal(got, im)
    c.check()
    assert (c.image_status(B) == 0).all()


def test_record_bytes_follows_the_context_model(torch_mod, codecs):
    seg = np.zeros(49, np.int32)
    seg[:22] = 7
    assert codecs("trainedlike").record_bytes(seg) == 6 + 4 * 49 + 7 * 22 and codecs("b_trainedlike").record_bytes(seg) == 6 + 4 * 22 + 7 * 22


# ------------------------------------------------------------------------------------------------ 3. every alignment
def test_every_alignment_of_blob_and_containers(torch_mod, codecs):
    """Blob view at each of 16 byte offsets x container view at each of 16: 256 pairs, both directions, against ref_records, with poisoned
    guards on both sides of both buffers.  The container stride is odd, so the two images of a call differ in alignment too."""
    torch = torch_mod
    c = codecs("trainedlike")
    sizes = [(32, 32), (33, 35)]
    _, cont, seg, cont_np, seg_np, _ = encoded(torch, c, "trainedlike", sizes, _mode("rans1"), seeds=[1, 2])
    B, n = 2, 49
    pays = seg_np.sum(axis=1)
    stride = (int(pays.max()) + 15) // 16 * 16 + 5
    src_np = np.full((B, stride), 0x3C, np.uint8)
    for b in range(B):
        src_np[b, :pays[b]] = cont_np[b, :pays[b]]
    seg_d = _dev(torch, seg_np)
    cap = int(pays.sum()) + B * (6 + 4 * n) + 9
    want_blob, want_off, _, _ = rr.pack(src_np, seg_np, n, np.full(cap, POISON, np.uint8))
    total = int(want_off[-1])
    want_blob_d, want_off_d = _dev(torch, want_blob), _dev(torch, want_off)
    want_cont, want_seg, _, _ = rr.unpack(want_blob[:total], want_off, n, np.full((B, stride), POISON, np.uint8))
    want_cont_d, want_seg_d = _dev(torch, want_cont.reshape(-1)), _dev(torch, want_seg)
    src_flat = _dev(torch, src_np.reshape(-1))
    bad = []
    for ca in range(16):
        sbuf, sview, sbase = guarded(torch, B * stride, ca)
        sview.copy_(src_flat)
        for ba in range(16):
            # pack: containers at offset ca -> blob at offset ba
            bbuf, bview, bbase = guarded(torch, cap, ba)
            ro = torch.full((B + 1,), -7, dtype=torch.int64, device=DEV)
            c.pack_records(sview.view(B, stride), seg_d, out=bview, rec_off=ro)
            ok = torch.equal(bview, want_blob_d) and torch.equal(ro, want_off_d) and guards_intact(bbuf, bbase, cap)
            # unpack: that blob (offset ba) -> containers at offset ca
            obuf, oview, obase = guarded(torch, B * stride, ca)
            sl = torch.full((B, 49), -7, dtype=torch.int32, device=DEV)
            c.unpack_records(bview[:total], ro, out=oview.view(B, stride), seg_len=sl)
            ok2 = torch.equal(oview, want_cont_d) and torch.equal(sl, want_seg_d) and guards_intact(obuf, obase, B * stride)
            ok2 = ok2 and torch.equal(bview, want_blob_d) and guards_intact(bbuf, bbase, cap)            # (the source side stays as it was)
            if not (ok and ok2):
                bad.append((ca, ba, ok, ok2))
        assert torch.equal(sview, src_flat) and guards_intact(sbuf, sbase, B * stride)
    c.check()
    assert not bad, bad


def test_a_payload_of_several_chunks(torch_mod, codecs):
    """a 512x768 noise image: its payload spans more than three of the copy kernel's per-workgroup chunks and ends in an odd tail"""
    torch = torch_mod
    from llicti_amd import _lib
    from llicti_amd import codec as cd
    c = codecs("trainedlike")
    sizes = [(512, 768)]
    mode = cd.auto_modes(sizes)
    _, cont, seg, cont_np, seg_np, _ = encoded(torch, c, "trainedlike", sizes, mode, seeds=[1])
    pay = int(seg_np[0].sum())
    assert pay > 3 * _lib.RECORD_CHUNK and pay % _lib.RECORD_CHUNK
    n, hb = 49, 6 + 4 * 49
    want = llic_files(cont_np, seg_np, 5)[0]
    want_d = _dev(torch, np.frombuffer(want, np.uint8))
    odd_tail = 0
    for ba, ca in ((0, 0), (3, 7), (11, 2), (8, 12)):
        sbuf, sview, sbase = guarded(torch, pay, ca)
        sview.copy_(cont[0, :pay])
        bbuf, bview, bbase = guarded(torch, len(want), ba)
        ro = torch.full((2,), -7, dtype=torch.int64, device=DEV)
        c.pack_records(sview.view(1, pay), seg, out=bview, rec_off=ro)             # (stride = the payload itself, blob_cap = the record itself)
        assert torch.equal(bview, want_d) and ro.tolist() == [0, len(want)] and guards_intact(bbuf, bbase, len(want)), (ba, ca)
        obuf, oview, obase = guarded(torch, pay, ca)
        sl = torch.full((1, 49), -7, dtype=torch.int32, device=DEV)
        c.unpack_records(bview, ro, out=oview.view(1, pay), seg_len=sl)
        assert torch.equal(oview, cont[0, :pay]) and torch.equal(sl, seg) and guards_intact(obuf, obase, pay), (ba, ca)
        last = pay % _lib.RECORD_CHUNK                        # the last chunk: head bytes up to the destination's 16-byte boundary, then vectors, then the tail
        for dst0 in ((bview.data_ptr() + hb + pay - last), (oview.data_ptr() + pay - last)):
            odd_tail += ((last - (-dst0) % 16) % 16) != 0
    c.check()
    assert odd_tail >= 4


# ------------------------------------------------------------------------------------------------ 4. malformed records
MAL_SIZES = [(32, 32), (67, 93), (33, 35), (64, 96)]
MAL_SEEDS = [2, 1, 4, 6]                # record 1 is the noise image: the batch's largest payload


@pytest.mark.parametrize("case", sorted(rr.malformed_cases(49)))
def test_malformed_record_is_refused_and_its_neighbours_are_not(torch_mod, codecs, case):
    torch = torch_mod
    from llicti_amd import _lib
    c = codecs("trainedlike")
    n, mode = 49, _mode("xrans2")
    imgs, cont, seg, cont_np, seg_np, _ = encoded(torch, c, "trainedlike", MAL_SIZES, mode, seeds=MAL_SEEDS)
    pays = seg_np.sum(axis=1)
    assert int(np.argmax(pays)) == 1
    stride = (int(pays.max()) + 15) // 16 * 16
    blob = np.frombuffer(b"".join(llic_files(cont_np, seg_np, 5)), np.uint8)
    off = np.concatenate(([0], np.cumsum(pays + 6 + 4 * n))).astype(np.int64)
    f, bad = rr.malformed_cases(n)[case]
    blob2, off2, stride2, nb = f(blob, off, stride)
    want_out, want_seg, want_img, want_st = rr.unpack(blob2[:nb], off2, n, np.full((4, stride2), POISON, np.uint8))
    assert list(want_img) == [_lib.EFORMAT if b == bad else 0 for b in range(4)] and want_st == _lib.EFORMAT
    bbuf, bview, bbase = guarded(torch, nb, 3)
    bview.copy_(_dev(torch, blob2[:nb]))
    obuf, oview, obase = guarded(torch, 4 * stride2, 0)
    sl = torch.full((4, 49), -7, dtype=torch.int32, device=DEV)
    out = oview.view(4, stride2)
    c.unpack_records(bview, _dev(torch, off2), out=out, seg_len=sl)
    assert list(c.image_status(4)) == list(want_img)                    # exactly that image
    with pytest.raises(_lib.LlictiError) as ei:
        c.check()
    assert ei.value.code == _lib.EFORMAT
    sl_np, out_np = sl.cpu().numpy(), out.cpu().numpy()
    assert (sl_np[bad] == 0).all() and (out_np[bad] == POISON).all()     # zero row, container untouched
    assert np.array_equal(sl_np, want_seg) and np.array_equal(out_np, want_out)      # the verdict and every byte: ref_records
    assert guards_intact(obuf, obase, 4 * stride2) and guards_intact(bbuf, bbase, nb)
    for b in set(range(4)) - {bad}:
        assert np.array_equal(sl_np[b], seg_np[b]) and np.array_equal(out_np[b, :pays[b]], cont_np[b, :pays[b]])
    # a decode behind it flags the same image and no other, and the neighbours' pixels are exact
    got = decoded_images(torch, c, out, sl, MAL_SIZES, mode)
    assert list(c.image_status(4)) == list(want_img)
    with pytest.raises(_lib.LlictiError) as ei:
        c.check()
    assert ei.value.code == _lib.EFORMAT
    for b in set(range(4)) - {bad}:
        assert np.array_equal(got[b], imgs[b]), b


# ------------------------------------------------------------------------------------------------ 5. pack refusals
def test_pack_refusals(torch_mod, codecs):
    torch = torch_mod
    from llicti_amd import _lib
    c = codecs("trainedlike")
    n = 49
    _, cont, seg, cont_np, seg_np, _ = encoded(torch, c, "trainedlike", MAL_SIZES, _mode("xrans2"), seeds=MAL_SEEDS)
    files = llic_files(cont_np, seg_np, 5)
    need = sum(len(f) for f in files)
    # blob_cap one byte short
    buf, view, base = guarded(torch, need - 1, 5)
    ro = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    c.pack_records(cont, seg, out=view, rec_off=ro)
    with pytest.raises(_lib.LlictiError) as ei:
        c.check()
    assert ei.value.code == _lib.ENOSPACE
    ro_h = ro.cpu().numpy()
    assert int(ro_h[-1]) == need and list(ro_h) == list(np.concatenate(([0], np.cumsum([len(f) for f in files]))))       # the size the caller needs
    assert int(buf[base + need - 1]) == POISON and guards_intact(buf, base, need - 1)                                  # the byte at blob_cap
    ref_blob, ref_off, ref_img, ref_st = rr.pack(cont_np, seg_np, n, np.full(need - 1, POISON, np.uint8))
    assert ref_st == _lib.ENOSPACE and np.array_equal(ref_blob, view.cpu().numpy()) and (c.image_status(4) == 0).all()
    assert view[:int(ro_h[3])].cpu().numpy().tobytes() == b"".join(files[:3])          # (the records that fit are there)
    # a negative entry: a zero-length record and a flag, the neighbours intact
    seg_bad = seg_np.copy()
    seg_bad[2, 6] = -1
    buf, view, base = guarded(torch, need, 9)
    c.pack_records(cont, _dev(torch, seg_bad), out=view, rec_off=ro)
    assert list(c.image_status(4)) == [0, 0, _lib.EFORMAT, 0]
    with pytest.raises(_lib.LlictiError) as ei:
        c.check()
    assert ei.value.code == _lib.EFORMAT
    ro_h = ro.cpu().numpy()
    assert ro_h[2] == ro_h[3] and int(ro_h[-1]) == need - len(files[2])
    got = view.cpu().numpy()
    assert got[:int(ro_h[-1])].tobytes() == files[0] + files[1] + files[3] and (got[int(ro_h[-1]):] == POISON).all() and guards_intact(buf, base, need)
    ref_blob, ref_off, ref_img, _ = rr.pack(cont_np, seg_bad, n, np.full(need, POISON, np.uint8))
    assert np.array_equal(ref_blob, got) and np.array_equal(ref_off, ro_h)
    # a row whose sum exceeds the stride it is packed with
    small = int(seg_np[0].sum())
    c.pack_records(cont[:, :small].contiguous(), seg, out=view, rec_off=ro)
    st = c.image_status(4)
    assert st[0] == 0 and st[1] == _lib.EFORMAT
    with pytest.raises(_lib.LlictiError):
        c.check()


def test_host_side_refusals_launch_nothing(torch_mod, codecs):
    torch = torch_mod
    from llicti_amd import _lib
    c = codecs("trainedlike")
    L, s = c.L, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    cont = torch.full((2, 256), POISON, dtype=torch.uint8, device=DEV)
    seg = torch.zeros((2, 49), dtype=torch.int32, device=DEV)
    blob = torch.full((1024,), POISON, dtype=torch.uint8, device=DEV)
    ro = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    pack, unpack = L.llicti_pack_records, L.llicti_unpack_records
    E = _lib.EINVAL
    assert pack(None, p(cont), 256, p(seg), 2, p(blob), 1024, p(ro), s) == E
    assert pack(c.ctx, None, 256, p(seg), 2, p(blob), 1024, p(ro), s) == E and pack(c.ctx, p(cont), 256, None, 2, p(blob), 1024, p(ro), s) == E
    assert pack(c.ctx, p(cont), 256, p(seg), 2, None, 1024, p(ro), s) == E and pack(c.ctx, p(cont), 256, p(seg), 2, p(blob), 1024, None, s) == E
    assert pack(c.ctx, p(cont), 256, p(seg), 0, p(blob), 1024, p(ro), s) == E and pack(c.ctx, p(cont), 256, p(seg), -1, p(blob), 1024, p(ro), s) == E
    assert pack(c.ctx, p(cont), 0, p(seg), 2, p(blob), 1024, p(ro), s) == E
    assert pack(c.ctx, p(cont), 256, p(seg), 2, C.c_void_p(cont.data_ptr() + 500), 1024, p(ro), s) == E          # the blob overlaps the containers
    assert unpack(c.ctx, C.c_void_p(cont.data_ptr() + 100), 64, p(ro), 2, p(cont), 256, p(seg), s) == E
    assert unpack(c.ctx, None, 1024, p(ro), 2, p(cont), 256, p(seg), s) == E and unpack(c.ctx, p(blob), 1024, None, 2, p(cont), 256, p(seg), s) == E
    assert unpack(c.ctx, p(blob), 1024, p(ro), 2, None, 256, p(seg), s) == E and unpack(c.ctx, p(blob), 1024, p(ro), 2, p(cont), 256, None, s) == E
    assert unpack(c.ctx, p(blob), 1024, p(ro), 0, p(cont), 256, p(seg), s) == E
    assert unpack(c.ctx, p(blob), 1024, p(ro), 2, p(cont), 256, C.c_void_p(blob.data_ptr() + 8), s) == E         # the segment lengths inside the blob
    torch.cuda.synchronize()
    c.check()
    assert bool((cont == POISON).all()) and bool((blob == POISON).all()) and bool((ro == -7).all()) and bool((seg == 0).all())


@pytest.mark.parametrize("B", [257, 513])
def test_more_images_than_one_round_of_the_scan(torch_mod, codecs, B):
    """The offsets come from a scan of 256 images a round: B = 257 and 513 make the total of a round carry into the next one (two and three
    rounds, the last of ONE image), with a malformed row / record at index 256, the first of the second round.  Synthetic containers of 22
    segments against the numpy restatement: offsets, blob, containers, and every image's status -- the bad one's neighbours included."""
    torch = torch_mod
    from llicti_amd import _lib
    c = codecs("b_trainedlike")
    n, stride, bad = c.nseg, 160, 256
    assert n == 22
    cont_np, seg_np = rr.synthetic_containers(np.random.default_rng(B), B, n, stride)
    # pack: row 256 has a negative length
    seg_bad = seg_np.copy()
    seg_bad[bad, 7] = -1
    cap = sum(rr.record_size(seg_bad[b], n, stride) for b in range(B)) + 7
    ref_blob, ref_off, ref_img, ref_st = rr.pack(cont_np, seg_bad, n, np.full(cap, POISON, np.uint8))
    assert ref_st == _lib.EFORMAT and ref_off[bad] == ref_off[bad + 1] and ref_off[-1] == cap - 7
    buf, view, base = guarded(torch, cap, 3)
    ro = torch.full((B + 1,), -7, dtype=torch.int64, device=DEV)
    c.pack_records(_dev(torch, cont_np), _dev(torch, seg_bad), out=view, rec_off=ro)
    status = c.image_status(B)
    with pytest.raises(_lib.LlictiError) as ei:
        c.check()
    assert ei.value.code == _lib.EFORMAT
    assert np.array_equal(ro.cpu().numpy(), ref_off) and np.array_equal(view.cpu().numpy(), ref_blob) and guards_intact(buf, base, cap)
    assert np.array_equal(status, ref_img) and list(status[bad - 1:bad + 2]) == [0, _lib.EFORMAT, 0][:B - bad + 1]
    # unpack: the well-formed blob with record 256's magic damaged
    good_blob, good_off, img0, st0 = rr.pack(cont_np, seg_np, n, np.zeros(int(ref_off[-1]) + stride + 6 + 4 * n, np.uint8))
    assert st0 == rr.OK and (img0 == 0).all()
    blob_np = good_blob[:good_off[-1]].copy()
    blob_np[good_off[bad] + 2] ^= 0x40
    ref_cont, ref_seg, ref_img, ref_st = rr.unpack(blob_np, good_off, n, np.full((B, stride), POISON, np.uint8))
    assert ref_st == _lib.EFORMAT and (ref_cont[bad] == POISON).all()
    cbuf, cflat, cbase = guarded(torch, B * stride, 5)
    seg = torch.full((B, 49), -3, dtype=torch.int32, device=DEV)
    c.unpack_records(_dev(torch, blob_np), good_off, out=cflat.view(B, stride), seg_len=seg)
    status = c.image_status(B)
    with pytest.raises(_lib.LlictiError) as ei:
        c.check()
    assert ei.value.code == _lib.EFORMAT
    assert np.array_equal(cflat.view(B, stride).cpu().numpy(), ref_cont) and np.array_equal(seg.cpu().numpy(), ref_seg) and guards_intact(cbuf, cbase, B * stride)
    assert np.array_equal(status, ref_img) and list(status[bad - 1:bad + 2]) == [0, _lib.EFORMAT, 0][:B - bad + 1]


# ------------------------------------------------------------------------------------------------ 6. offsets past 4 GiB
def test_offsets_past_4_gib(torch_mod, codecs):
    torch = torch_mod
    c = codecs("trainedlike")
    sizes = [(32, 32), (32, 32)]
    imgs, cont, seg, cont_np, seg_np, _ = encoded(torch, c, "trainedlike", sizes, 0, seeds=[1, 2])
    want = b"".join(llic_files(cont_np, seg_np, 5))
    first = (1 << 32) + 5
    try:
        big = torch.empty(((1 << 32) + (64 << 10),), dtype=torch.uint8, device=DEV)         # (no fill)
    except RuntimeError as e:
        pytest.skip(f"no 4 GiB + 64 KiB allocation on this device: {e}")
    try:
        assert len(want) + 16 < big.numel() - first
        big[first - 16:].fill_(POISON)
        ro = torch.full((3,), -7, dtype=torch.int64, device=DEV)
        c.pack_records(cont, seg, out=big[first:], rec_off=ro)          # the records land at byte 2^32 + 5 of the allocation
        c.check()
        ro_h = ro.cpu().numpy()
        assert int(ro_h[-1]) == len(want)
        assert big[first:first + len(want)].cpu().numpy().tobytes() == want
        assert bool((big[first - 16:first] == POISON).all()) and bool((big[first + len(want):] == POISON).all())
        # ... and are unpacked from there: offsets above 2^32 into the whole allocation as the blob
        cont2, seg2 = c.unpack_records(big, ro_h + first)
        c.check()
        assert (c.image_status(2) == 0).all() and np.array_equal(seg2.cpu().numpy(), seg_np)
        for b in range(2):
            m = int(seg_np[b].sum())
            assert np.array_equal(cont2[b, :m].cpu().numpy(), cont_np[b, :m])
        got = c.decode(cont2, seg2, 32, 32, mode=0).cpu().numpy()
        c.check()
        assert np.array_equal(got, np.stack(imgs))
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 7. the caller's stream
def test_both_calls_on_a_gated_stream(env, codecs):
    """pack and unpack behind a gated queue (tests/test_hip_streams.py): the inputs hold a DECOY (another valid batch) until the gate opens, the
    outputs poison.  A snapshot taken on the null stream while the gate is still closed must be all poison; after the gate the results are those
    of the real inputs."""
    torch = env.torch
    c = codecs("trainedlike")
    n, mode = 49, _mode("xrans2")
    sizes = [(33, 35), (32, 32)]
    _, _, _, cont_a, seg_a, _ = encoded(torch, c, "trainedlike", sizes, mode, seeds=[1, 2])
    _, _, _, cont_b, seg_b, _ = encoded(torch, c, "trainedlike", sizes, mode, seeds=[3, 4])
    stride = (int(max(seg_a.sum(axis=1).max(), seg_b.sum(axis=1).max())) + 15) // 16 * 16
    real_c, decoy_c = np.ascontiguousarray(cont_a[:, :stride]), np.ascontiguousarray(cont_b[:, :stride])
    cap = 2 * (6 + 4 * n + stride)
    null = torch.cuda.default_stream(DEV)
    # pack
    want_blob, want_off, _, _ = rr.pack(real_c, seg_a, n, np.full(cap, POISON, np.uint8))
    run = Run(env, "s")
    d_cont, d_seg = run.stage(decoy_c, real_c), run.stage(seg_b, seg_a)
    blob, ro = run.poison((cap,)), run.poison((3,), torch.int64, -7)
    with run:
        c.pack_records(d_cont, d_seg, out=blob, rec_off=ro)
        k_blob, k_ro = run.keep(blob), run.keep(ro)
        with torch.cuda.stream(null):
            early_blob, early_ro = blob.clone(), ro.clone()
        null.synchronize()
        run.enqueued()
    assert bool((early_blob == POISON).all()) and bool((early_ro == -7).all()), "pack wrote before the gate opened"
    assert np.array_equal(k_blob.cpu().numpy(), want_blob) and np.array_equal(k_ro.cpu().numpy(), want_off)
    c.check()
    # unpack
    decoy_blob, decoy_off, _, _ = rr.pack(decoy_c, seg_b, n, np.full(cap, POISON, np.uint8))
    assert not np.array_equal(decoy_off, want_off)
    want_cont, want_seg, _, _ = rr.unpack(want_blob, want_off, n, np.full((2, stride), POISON, np.uint8))
    run = Run(env, "s")
    d_blob, d_off = run.stage(decoy_blob, want_blob), run.stage(decoy_off, want_off)
    out, sl = run.poison((2, stride)), run.poison((2, 49), torch.int32, -7)
    with run:
        c.unpack_records(d_blob, d_off, out=out, seg_len=sl)
        k_out, k_sl = run.keep(out), run.keep(sl)
        with torch.cuda.stream(null):
            early_out, early_sl = out.clone(), sl.clone()
        null.synchronize()
        run.enqueued()
    assert bool((early_out == POISON).all()) and bool((early_sl == -7).all()), "unpack wrote before the gate opened"
    assert np.array_equal(k_out.cpu().numpy(), want_cont) and np.array_equal(k_sl.cpu().numpy(), want_seg)
    c.check()
    assert (c.image_status(2) == 0).all()


# ------------------------------------------------------------------------------------------------ 8. through the model and a file
def _model(torch, container):
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    torch.manual_seed(1337)
    return LLICTI(default_config(container=container)).to(DEV).eval()


def test_through_the_model_and_a_file(torch_mod, tmp_path):
    torch = torch_mod
    from llicti_amd import archive, fileio
    m = _model(torch, "xrans2")
    sizes = [(150, 131), (96, 160), (67, 93)]
    rgbs = [make_image("smooth", h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    enc = m.encode_batch_async(rgbs)
    lists = enc.lists()
    blob, rec_off = enc.records()
    files = [fileio.dumps_llic(bl) for bl in lists]
    assert bytes(blob) == b"".join(files) and list(rec_off) == list(np.concatenate(([0], np.cumsum([len(f) for f in files]))))
    path = str(tmp_path / "m.llia")
    with archive.ArchiveWriter(path, m.codec().nseg) as aw:
        aw.append_records(blob, rec_off, ["a", "b", "c"])
    with archive.ArchiveReader(path) as ar:
        assert len(ar) == 3 and ar.sizes == sizes and ar.names == ["a", "b", "c"]
        for i in range(3):
            assert ar[i] == lists[i]
        order = [2, 0, 1, 0]
        batch = ar.read_batch(order)
        groups = [dict(size=(32, 28), image=[0, 1, 1, 3], boxes=[(3, 8, 50, 60), (0, 20, 96, 100), (10, 0, 80, 70), (5, 5, 90, 90)], flip=[1, 0, 1, 0], dtype=torch.float16),
                  dict(size=(12, 12), image=[2, 0], boxes=[(40, 50, 30, 30), (10, 9, 40, 41)])]
        mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        got = m.decode_batch_async(batch, tensor=dict(views=groups, mean=mean, std=std))
        m.codec().check()
        assert (m.codec().image_status(4) == 0).all()
        want = m.decode_batch_async([lists[i] for i in order], tensor=dict(views=groups, mean=mean, std=std))
        m.codec().check()
        assert len(got) == len(want) == 2
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g, w)                       # bit for bit
        # ... and the plain decode of a batch gives the pixels
        flat, Hs, Ws = m.decode_batch_async(ar.read_batch([1, 2]), flat=True)
        m.codec().check()
        offs, _ = m.codec().flat_offsets(Hs, Ws)
        for o, h, w, i in zip(offs, Hs, Ws, (1, 2)):
            assert np.array_equal(flat[int(o):int(o) + 3 * h * w].view(3, h, w).cpu().numpy(), rgbs[i])


def test_cli_pack_info_unpack_round_trip(torch_mod, tmp_path, capsys):
    from llicti_amd import archive, cli, fileio
    sizes = [(67, 93), (64, 96), (67, 93)]
    rgbs = [make_image("smooth" if i != 1 else "noise", h, w, 60 + i) for i, (h, w) in enumerate(sizes)]
    srcs = []
    for i, r in enumerate(rgbs):
        srcs.append(str(tmp_path / f"img_{i}.ppm"))
        fileio.write_image(srcs[-1], r)
    arc, out = str(tmp_path / "set.llia"), str(tmp_path / "out")
    assert cli.main(["pack", arc] + srcs + ["--container", "xrans2", "--batch", "2"]) == 0
    assert f"3 images -> {arc}" in capsys.readouterr().out
    with archive.ArchiveReader(arc) as ar:
        assert ar.names == ["img_0", "img_1", "img_2"] and ar.sizes == sizes and ar.nseg == 49
    assert cli.main(["info", arc]) == 0
    text = capsys.readouterr().out
    assert "3 images, n = 49" in text and "img_1: 96x64, container xrans2" in text
    assert cli.main(["unpack", arc, out, "--as", "ppm"]) == 0
    for i, r in enumerate(rgbs):
        assert np.array_equal(fileio.read_image(os.path.join(out, f"img_{i}.ppm")), r), i
