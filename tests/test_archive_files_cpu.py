"""Whole archive files pinned byte for byte (no GPU): tests/golden/archive_files.npz holds a `.llia` of each model and a `.llpa` as the writers
wrote them BEFORE archive.py's file layer served both kinds (tests/golden/make_archive_files.py).  The writers of today must write the same
bytes, and the readers of today must read from them what a second, literal reader of the layout (tests/ref_records.py) reads."""
import os
import sys

import numpy as np
import pytest

import ref_progressive as rp
import ref_records as rr
from conftest import GOLDEN
from llicti_amd import archive, fileio, progressive

sys.path.insert(0, GOLDEN)
import make_archive_files as mk  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    path = os.path.join(GOLDEN, "archive_files.npz")
    assert os.path.getsize(path) < 100_000
    vec = np.load(path)
    assert sorted(vec.files) == sorted(mk.KINDS)
    return {k: vec[k].tobytes() for k in mk.KINDS}


@pytest.mark.parametrize("kind", mk.KINDS)
def test_writers_write_the_pinned_bytes(tmp_path, golden, kind):
    path = str(tmp_path / kind)
    mk.write(kind, path)
    assert open(path, "rb").read() == golden[kind]


def _file(tmp_path, golden, kind):
    path = str(tmp_path / (kind + (progressive.EXT if kind == "llpa" else archive.EXT)))
    open(path, "wb").write(golden[kind])
    return path


def _common(ar, path, lit, n):
    """every attribute the two readers share, against the literal reading"""
    count = lit["count"]
    assert (ar.path, ar.nseg, ar.count, len(ar)) == (path, n, count, count) and lit["n"] == n
    assert ar.index_offset == ar.total_bytes == lit["offsets"][-1]
    assert ar.offsets.dtype == np.int64 and list(ar.offsets) == lit["offsets"]
    assert ar.sizes == lit["sizes"] and ar.modes == lit["modes"] and ar.names == lit["names"]
    assert all(isinstance(v, int) for hw in ar.sizes for v in hw) and all(isinstance(m, int) for m in ar.modes)
    for k in range(count):
        assert ar.record(k) == lit["records"][k] == ar.record(k - count)
    for bad in (count, -count - 1):
        with pytest.raises(IndexError):
            ar.record(bad)


@pytest.mark.parametrize("model", ["a", "b"])
def test_llia_reader_reads_the_pinned_file(tmp_path, golden, model):
    kind, n = "llia_" + model, 49 if model == "a" else 22
    path = _file(tmp_path, golden, kind)
    lit = rr.read_llia(golden[kind])
    files = list(mk.llic_files(model).values())
    assert lit["records"] == files and lit["names"] == mk.names_of(model) and mk.UTF8_NAME in lit["names"]
    with archive.ArchiveReader(path) as ar:
        _common(ar, path, lit, n)
        assert [ar[k] for k in range(len(ar))] == [fileio.loads_llic(f) for f in files]
        idx = [len(files) - 1, 0, 1, 1]
        bt = ar.read_batch(idx, pinned=False)
        assert bt.blob.numpy().tobytes() == b"".join(files[i] for i in idx)
        assert bt.rec_off.dtype == np.int64 and bt.rec_off.tolist() == np.concatenate(([0], np.cumsum([len(files[i]) for i in idx]))).tolist()
        assert (bt.Hs, bt.Ws, bt.modes) == ([lit["sizes"][i][0] for i in idx], [lit["sizes"][i][1] for i in idx], [lit["modes"][i] for i in idx])
        pay = max(len(files[i]) for i in idx) - (6 + 4 * n)
        assert bt.stride == (pay + 15) // 16 * 16
    with archive.open_archive(path) as ar:
        assert type(ar) is archive.ArchiveReader and ar.names == lit["names"]
    with pytest.raises(ValueError):
        progressive.ProgressiveReader(path)


def test_llpa_layout_read_literally(tmp_path, golden):
    """The `.llpa` index -- offsets, sizes, modes, P_1 .. P_L, names -- from the written layout, against ProgressiveReader."""
    path = _file(tmp_path, golden, "llpa")
    recs = mk.progressive_records()
    recs = [recs[0], recs[1], recs[0]]
    lit = rr.read_archive(golden["llpa"], b"LLPA", 5)
    assert lit["records"] == recs and lit["names"] == mk.LLPA_NAMES + ["2"]
    assert [[len(r)] + e for r, e in zip(recs, lit["extra"])] == [rp.prefixes(r) for r in recs]
    with pytest.raises(ValueError):
        rr.read_archive(golden["llpa"], b"LLIA", 5)
    with pytest.raises(ValueError):
        rr.read_archive(golden["llpa"], b"LLPA", 2)            # config B's row width: the names do not end where the index does
    with progressive.ProgressiveReader(path) as ar:
        _common(ar, path, lit, 49)
        assert ar.nlevels == 5 and ar.prefix.dtype == np.int64 and ar.prefix.shape == (3, 6)
        assert ar.prefix.tolist() == [[o1 - o0] + e for o0, o1, e in zip(lit["offsets"], lit["offsets"][1:], lit["extra"])]
        assert [ar.payload_bytes(k) for k in range(3)] == [rp.check(r)["S"] for r in recs]
        assert [ar[k] for k in range(3)] == [fileio.loads_llic(progressive.to_llic(r)) for r in recs]
        idx, red = [2, 1, 1], [5, 0, 3]
        bt = ar.read_batch(idx, reduce=red, pinned=False)
        want = [recs[i][:rp.prefixes(recs[i])[r]] for i, r in zip(idx, red)]
        assert bt.blob.numpy().tobytes() == b"".join(want) and bt.rec_off.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()
        assert (bt.Hs, bt.Ws, bt.modes, bt.reduce) == ([lit["sizes"][i][0] for i in idx], [lit["sizes"][i][1] for i in idx], [lit["modes"][i] for i in idx], red)
        assert bt.stride == (max(rp.check(recs[i])["S"] for i in idx) + 15) // 16 * 16
    with archive.open_archive(path) as ar:
        assert type(ar) is progressive.ProgressiveReader and ar.names == lit["names"]


def test_open_archive_refuses_what_is_no_archive(tmp_path, golden):
    for name, data in (("empty", b""), ("short", golden["llpa"][-20:]), ("llic", next(iter(mk.llic_files("b").values()))),
                       ("magic", golden["llia_b"][:-28] + b"LLIX" + golden["llia_b"][-24:])):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        with pytest.raises(archive.NotAnArchive):
            archive.open_archive(p)
    p = str(tmp_path / "crc.llia")                                           # an archive by its magic, damaged: its reader's refusal
    open(p, "wb").write(golden["llia_b"][:-40] + bytes([golden["llia_b"][-40] ^ 1]) + golden["llia_b"][-39:])
    with pytest.raises(ValueError) as e:
        archive.open_archive(p)
    assert not isinstance(e.value, archive.NotAnArchive) and issubclass(archive.NotAnArchive, ValueError)
