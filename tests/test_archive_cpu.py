"""Image archives, the host side (no GPU): llicti_record_bytes, the `.llia` writer and reader against a second, literal reader of the layout
(tests/ref_records.py), read_batch, what a damaged file is refused for, the CLI parsers, and the numpy restatement of the device's pack and
unpack (the yardstick of tests/test_hip_archive.py) on synthetic containers."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import ref_records as rr
from conftest import GOLDEN
from llicti_amd import _lib, archive, cli, fileio
from llicti_amd import codec as cd


# ------------------------------------------------------------------------------------------------ records of real containers (frozen vectors)
def _lists_a():
    """config A bytestream_lists from the frozen rANS containers (tests/golden/rans_vectors.npz: bytes + the 6 x 9 lengths)"""
    vec = np.load(os.path.join(GOLDEN, "rans_vectors.npz"))
    keys = sorted(k[:-6] for k in vec.files if k.endswith("_bytes"))
    out = {}
    for key in keys:
        flat, lens, pos, segs = vec[key + "_bytes"].tobytes(), [int(v) for v in vec[key + "_seglen"]], 0, []
        for ln in lens:
            segs.append(flat[pos:pos + ln])
            pos += ln
        assert pos == len(flat) and len(segs) == 54
        out[key] = [segs[9 * r:9 * r + 9] for r in range(6)]
    return out


def _lists_b():
    vec = np.load(os.path.join(GOLDEN, "rans_b_vectors.npz"))
    out = {}
    for key in sorted(k[:-6] for k in vec.files if k.endswith("_bytes")):
        flat, pos, segs = vec[key + "_bytes"].tobytes(), 0, []
        for ln in vec[key + "_seglen"]:
            segs.append(flat[pos:pos + int(ln)])
            pos += int(ln)
        out[key] = fileio.segments_to_bytestream_list(segs)
    return out


@pytest.fixture(scope="module")
def lists_a():
    return _lists_a()


@pytest.fixture(scope="module")
def lists_b():
    return _lists_b()


def test_new_symbols_are_declared_exported_and_bound():
    import re
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "llicti_hip.h")).read()
    L = _lib.lib()
    for name in ("llicti_record_bytes", "llicti_record_bytes_n", "llicti_pack_records", "llicti_unpack_records"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
        decl = re.search(r"(?:int|size_t) %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGS[name][1]) == len(getattr(L, name).argtypes), name
    assert int(re.search(r"#define LLICTI_RECORD_CHUNK (\d+)", header).group(1)) == _lib.RECORD_CHUNK


def test_record_bytes_equals_dumps_llic_for_both_models(lists_a, lists_b):
    L = _lib.lib()
    for n, lists in ((49, lists_a), (22, lists_b)):
        assert lists
        for key, bl in lists.items():
            _, seg = cd.bytestream_list_to_container(bl)
            want = len(fileio.dumps_llic(bl))
            assert int(L.llicti_record_bytes_n(n, seg.ctypes.data_as(C.c_void_p))) == want == 6 + 4 * n + int(seg.sum()), key
            if n == 49:              # (without a context: config A)
                assert int(L.llicti_record_bytes(None, seg.ctypes.data_as(C.c_void_p))) == want
    seg = np.zeros(49, np.int32)
    seg[7] = -1
    assert int(L.llicti_record_bytes_n(49, seg.ctypes.data_as(C.c_void_p))) == 0
    assert int(L.llicti_record_bytes_n(49, None)) == 0 and int(L.llicti_record_bytes_n(48, seg.ctypes.data_as(C.c_void_p))) == 0


# ------------------------------------------------------------------------------------------------ writer -> reader
def _write(path, lists, n, how="mixed"):
    files = [fileio.dumps_llic(bl) for bl in lists.values()]
    names = list(lists)
    with archive.ArchiveWriter(path, n) as aw:
        if how == "blob":
            aw.append_records(b"".join(files), np.concatenate(([0], np.cumsum([len(f) for f in files]))), names)
        else:
            half = len(files) // 2
            blob = b"\x00" * 5 + b"".join(files[:half])           # (offsets need not start at 0)
            aw.append_records(blob, 5 + np.concatenate(([0], np.cumsum([len(f) for f in files[:half]]))), names[:half])
            for f, nm in zip(files[half:], names[half:]):
                aw.append_llic(f, nm)
        assert len(aw) == len(files)
    return files, names


@pytest.mark.parametrize("model", ["a", "b"])
@pytest.mark.parametrize("how", ["blob", "mixed"])
def test_writer_reader_round_trip(tmp_path, lists_a, lists_b, model, how):
    lists, n = (lists_a, 49) if model == "a" else (lists_b, 22)
    path = str(tmp_path / "x.llia")
    files, names = _write(path, lists, n, how)
    raw = open(path, "rb").read()
    lit = rr.read_llia(raw)
    with archive.ArchiveReader(path) as ar:
        assert len(ar) == len(files) == lit["count"] and ar.nseg == n == lit["n"]
        assert raw[:ar.total_bytes] == b"".join(files)                        # the record region IS the concatenated .llic files
        assert list(ar.offsets) == lit["offsets"] and ar.sizes == lit["sizes"] and ar.modes == lit["modes"] and ar.names == lit["names"] == names
        for k, (key, bl) in enumerate(lists.items()):
            assert ar.record(k) == files[k] == lit["records"][k]
            assert ar[k] == [[bytes(s) for s in row] for row in bl]
            hdr = bytes(bl[0][0]) + bytes(bl[0][1]) + bytes(bl[0][2])
            assert ar.sizes[k] == cd.header_dims(hdr) and ar.modes[k] == cd.mode_of_header(hdr)
        assert ar[-1] == ar[len(ar) - 1]
        with pytest.raises(IndexError):
            ar[len(ar)]


def test_names_default_to_the_running_index_and_hold_utf8(tmp_path, lists_b):
    files = [fileio.dumps_llic(bl) for bl in lists_b.values()]
    path = str(tmp_path / "n.llia")
    with archive.ArchiveWriter(path, 22) as aw:
        aw.append_llic(files[0])
        aw.append_llic(files[1], "bäume/ü.png")
        with pytest.raises(ValueError):
            aw.append_llic(files[0], "a\0b")
        with pytest.raises(ValueError):
            aw.append_llic(files[0][:-1])                 # a record whose payload is short
    with archive.ArchiveReader(path) as ar:
        assert ar.names == ["0", "bäume/ü.png"] == rr.read_llia(open(path, "rb").read())["names"]
    with pytest.raises(ValueError):
        archive.ArchiveWriter(str(tmp_path / "bad.llia"), 48)


def test_writer_refuses_a_record_of_the_other_model(tmp_path, lists_a):
    with archive.ArchiveWriter(str(tmp_path / "m.llia"), 22) as aw:
        with pytest.raises(ValueError):
            aw.append_llic(fileio.dumps_llic(next(iter(lists_a.values()))))
        assert len(aw) == 0


def test_read_batch_scattered_repeated_consecutive(tmp_path, lists_a):
    path = str(tmp_path / "b.llia")
    files, _ = _write(path, lists_a, 49, "blob")
    assert len(files) >= 6
    with archive.ArchiveReader(path) as ar:
        for idx in ([0, 1, 2, 3], [5, 0, 3], [2, 2, 2], [1, 2, 3, 0, 1, 5, 4], [len(files) - 1], [-1, 0]):
            bt = ar.read_batch(idx, pinned=False)
            want = [files[i] for i in idx]
            assert bt.blob.numpy().tobytes() == b"".join(want)
            assert list(bt.rec_off) == list(np.concatenate(([0], np.cumsum([len(f) for f in want])))) and bt.rec_off.dtype == np.int64
            assert bt.Hs == [ar.sizes[i][0] for i in idx] and bt.Ws == [ar.sizes[i][1] for i in idx] and bt.modes == [ar.modes[i] for i in idx]
            pay = max(len(f) for f in want) - (6 + 4 * 49)
            assert bt.stride == (pay + 15) // 16 * 16 and bt.stride % 16 == 0 and bt.stride >= pay
            assert bt.stride == cd.HipCodec.tight_stride(bt.rec_off, 49)
        assert ar.read_batch([0, 1]).blob.numpy().tobytes() == files[0] + files[1]        # (pinned=True without a GPU runtime: an ordinary buffer)
        with pytest.raises(IndexError):
            ar.read_batch([len(files)])


def test_damaged_files_are_refused(tmp_path, lists_b):
    path = str(tmp_path / "d.llia")
    _write(path, lists_b, 22, "blob")
    raw = bytearray(open(path, "rb").read())
    size = len(raw)
    index_offset = struct.unpack_from("<Q", raw, size - 28 + 16)[0]

    def refused(data):
        p = str(tmp_path / "t.llia")
        open(p, "wb").write(bytes(data))
        with pytest.raises(ValueError):
            archive.ArchiveReader(p)
        with pytest.raises(ValueError):
            rr.read_llia(bytes(data))

    archive.ArchiveReader(path).close()
    refused(raw[:-1])                                   # truncated (the trailer is read from the end)
    refused(raw[:size - 28])                            # the trailer gone
    refused(raw[:10])                                   # shorter than a trailer
    bad = bytearray(raw); bad[size - 28] ^= 0x20; refused(bad)                 # magic
    bad = bytearray(raw); bad[size - 28 + 4] = 2; refused(bad)                 # version
    bad = bytearray(raw); bad[size - 28 + 5] = 48; refused(bad)                # n
    for k in (index_offset, index_offset + 9, size - 29):                    # a flipped index byte: offsets, sizes, names
        bad = bytearray(raw); bad[k] ^= 1; refused(bad)
    bad = bytearray(raw); struct.pack_into("<Q", bad, size - 28 + 16, size); refused(bad)           # index_offset past the file
    bad = bytearray(raw); struct.pack_into("<Q", bad, size - 28 + 16, 1 << 62); refused(bad)
    bad = bytearray(raw); struct.pack_into("<Q", bad, size - 28 + 8, 1 << 40); refused(bad)         # a count the index cannot hold


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_parsers_pack_unpack_info():
    ap = cli.build_parser()
    a = ap.parse_args(["pack", "out.llia", "a.ppm", "b.png", "c.llic", "--container", "auto", "--config", "llicti_B.json", "--batch", "8"])
    assert (a.cmd, a.archive, a.src, a.container, a.config, a.checkpoint, a.batch) == ("pack", "out.llia", ["a.ppm", "b.png", "c.llic"], "auto", "llicti_B.json", None, 8)
    a = ap.parse_args(["pack", "out.llia", "a.ppm"])
    assert a.container == "ac" and a.batch == 24                   # --container as for encode
    a = ap.parse_args(["unpack", "in.llia", "dir"])
    assert (a.cmd, a.archive, a.dir, a.fmt) == ("unpack", "in.llia", "dir", "llic")
    assert ap.parse_args(["unpack", "in.llia", "dir", "--as", "ppm"]).fmt == "ppm" and ap.parse_args(["unpack", "in.llia", "dir", "--as", "png"]).fmt == "png"
    for bad in (["pack", "out.llia"], ["unpack", "in.llia"], ["unpack", "in.llia", "d", "--as", "jpg"], ["pack", "o.llia", "a.ppm", "--batch", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    # the existing subcommands keep their parsers
    e = ap.parse_args(["encode", "a.ppm", "a.llic"])
    assert (e.src, e.dst, e.container) == ("a.ppm", "a.llic", "ac")
    assert ap.parse_args(["info", "x.llia"]).src == "x.llia" and ap.parse_args(["decode", "a.llic", "a.ppm", "--reduce", "2"]).reduce == 2


def test_cli_info_and_unpack_llic_need_no_gpu(tmp_path, lists_b, capsys):
    path = str(tmp_path / "i.llia")
    files, names = _write(path, lists_b, 22, "blob")
    assert cli.main(["info", path]) == 0
    out = capsys.readouterr().out
    assert f"{len(files)} images" in out and "n = 22" in out and all(nm in out for nm in names) and "40x33" in out and "xrans3" in out
    d = str(tmp_path / "out")
    assert cli.main(["unpack", path, d]) == 0
    for f, nm in zip(files, names):
        assert open(os.path.join(d, nm + ".llic"), "rb").read() == f
    # ... and pack of .llic files alone gives the same archive
    p2 = str(tmp_path / "j.llia")
    assert cli.main(["pack", p2] + [os.path.join(d, nm + ".llic") for nm in names]) == 0
    assert open(p2, "rb").read() == open(path, "rb").read()


# ------------------------------------------------------------------------------------------------ the numpy restatement
@pytest.mark.parametrize("n", [49, 22])
def test_ref_unpack_of_pack_is_the_identity(n):
    rng = np.random.default_rng(n)
    for B, stride in ((1, 64), (4, 1000), (7, 4099)):
        cont, seg = rr.synthetic_containers(rng, B, n, stride)
        cap = sum(rr.record_size(seg[b], n, stride) for b in range(B))
        blob, off, img, st = rr.pack(cont, seg, n, np.full(cap + 7, 0xA5, np.uint8))
        assert st == rr.OK and (img == 0).all() and off[-1] == cap and (blob[cap:] == 0xA5).all()
        for b in range(B):
            bl = cd.container_to_bytestream_list(cont[b], seg[b], nlevels=(n - 4) // 9)
            assert blob[off[b]:off[b + 1]].tobytes() == fileio.dumps_llic(bl)
        back, seg2, img2, st2 = rr.unpack(blob, off, n, np.full((B, stride), 0x5A, np.uint8))
        assert st2 == rr.OK and (img2 == 0).all() and np.array_equal(seg2, seg)
        for b in range(B):
            m = int(seg[b].sum())
            assert np.array_equal(back[b, :m], cont[b, :m]) and (back[b, m:] == 0x5A).all()


def four_records(n, seed):
    """four synthetic containers whose record 1 holds the largest payload, packed by the numpy restatement -> (cont, seg, blob, off, stride)"""
    rng = np.random.default_rng(seed)
    B, stride = 4, 2048
    cont, seg = rr.synthetic_containers(rng, B, n, stride, max_seg=20)
    seg[:, 4] = np.maximum(seg[:, 4], 2)
    seg[1, 4] = 600
    blob, off, img, st = rr.pack(cont, seg, n, np.zeros(B * (rr.header_bytes(n) + stride), np.uint8))
    assert st == rr.OK and (img == 0).all()
    return cont, seg, blob[:off[-1]], off, stride


@pytest.mark.parametrize("n", [49, 22])
def test_ref_unpack_refuses_each_malformed_record(n):
    cont, seg, blob, off, stride = four_records(n, 100 + n)
    cases = rr.malformed_cases(n)
    assert len(cases) == 10
    for name, (f, bad) in cases.items():
        b2, o2, s2, nb = f(blob, off, stride)
        out, seg2, img, st = rr.unpack(b2[:nb], o2, n, np.full((4, s2), 0x5A, np.uint8))
        assert list(img) == [rr.EFORMAT if b == bad else 0 for b in range(4)] and st == rr.EFORMAT, name
        assert (seg2[bad] == 0).all() and (out[bad] == 0x5A).all(), name
        for b in set(range(4)) - {bad}:
            m = int(seg[b].sum())
            assert np.array_equal(seg2[b], seg[b]) and np.array_equal(out[b, :m], cont[b, :m]) and (out[b, m:] == 0x5A).all(), (name, b)
    _, _, img, _ = rr.unpack(blob, off - 1, n, np.zeros((4, stride), np.uint8))
    assert img[0] == rr.EFORMAT                                      # a negative offset


def test_ref_pack_refusals():
    n, B, stride = 22, 3, 300
    rng = np.random.default_rng(5)
    cont, seg = rr.synthetic_containers(rng, B, n, stride)
    need = sum(rr.record_size(seg[b], n, stride) for b in range(B))
    blob, off, img, st = rr.pack(cont, seg, n, np.full(need + 4, 0xA5, np.uint8), blob_cap=need - 1)
    assert st == rr.ENOSPACE and off[-1] == need and (img == 0).all() and (blob[off[2]:] == 0xA5).all()        # the last record does not fit: not written
    assert not (blob[:off[2]] == 0xA5).all()
    seg2 = seg.copy(); seg2[1, 4] = -3
    blob, off, img, st = rr.pack(cont, seg2, n, np.full(need, 0xA5, np.uint8))
    assert st == rr.EFORMAT and list(img) == [0, rr.EFORMAT, 0] and off[1] == off[2]
    seg3 = seg.copy(); seg3[2, 4] = stride
    _, off, img, _ = rr.pack(cont, seg3, n, np.full(need, 0xA5, np.uint8))
    assert list(img) == [0, 0, rr.EFORMAT] and off[2] == off[3]
