"""Progressive records without a GPU: the frozen vectors re-derived, the two Python readings of the format against each other, the CPU proof
that a prefix suffices (tests/ref_rans.py stopped behind level r on a container whose undelivered bytes are 0xA5), every malformed table
refused by the reference and by the library's host helper, `.llpa` files, the CLI's parsers, and the shared table code under sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import ref_progressive as rp
import ref_rans as rr
from conftest import GOLDEN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, GOLDEN)
KEYS = ["a_smooth_67x93_x3", "a_noise_33x40_x64", "b_noise_40x33_x3"]


@pytest.fixture(scope="module")
def vec():
    return np.load(os.path.join(GOLDEN, "progressive_vectors.npz"))


def _segs(vec, key):
    flat, pos, segs = vec[f"{key}_bytes"].tobytes(), 0, []
    for ln in vec[f"{key}_seglen"]:
        segs.append(flat[pos:pos + int(ln)])
        pos += int(ln)
    return segs


_full = {}


def _case(vec, key):
    """(segments, plain record, progressive record, cuts, the full decode's stages) of a frozen case; the decode is shared"""
    if key not in _full:
        import make_progressive_vectors as mk
        segs = _segs(vec, key)
        model = rr.OraclePlanes(segs, mk.weights(key))
        cuts, stages = rp.ref_cuts(segs, model.rows)
        _full[key] = (segs, rp.plain_record(segs), vec[f"{key}_record"].tobytes(), cuts, stages)
    return _full[key]


def test_fixture_is_small_and_rederived(vec):
    """The file is what its maker writes: config A's containers from the CPU oracle, every case's cuts from ref_rans' cursors and its record
    from ref_progressive (config B's container is the HIP encoder's: its bytes are taken as frozen)."""
    import make_progressive_vectors as mk
    assert os.path.getsize(os.path.join(GOLDEN, "progressive_vectors.npz")) < 100_000
    for key in KEYS:
        segs = _segs(vec, key)
        if mk.CASES[key][0] == "A":
            assert mk.container(key) == segs, key
        cuts, rec = mk.derive(key, segs)
        assert np.array_equal(cuts, vec[f"{key}_cuts"]) and rec == vec[f"{key}_record"].tobytes(), key
    hdr = rr.parse_header(_segs(vec, KEYS[1])[0][0], int.from_bytes(_segs(vec, KEYS[1])[2], "little"))
    assert (hdr["M"], hdr["per_seg"]) == (64, 2)
    assert sum(1 for row in vec[f"{KEYS[1]}_cuts"] if not row.any()) > 32          # mostly empty streams


@pytest.mark.parametrize("key", KEYS)
def test_round_trip_and_the_two_readings_agree(vec, key):
    from llicti_amd import fileio, progressive as pg
    segs, plain, rec, cuts, _ = _case(vec, key)
    assert rp.to_progressive(plain, cuts) == rec
    assert pg.to_llic(rec) == plain                                              # to_llic(to_progressive(x)) == x
    bl = fileio.loads_llic(pg.to_llic(rec))
    assert rr.segments(bl) == segs
    t, h = rp.check(rec), pg.parse_head(rec)
    assert pg.prefix_bytes(rec[:t["T"]]) == t["prefix"] == h.prefix
    assert (h.n, h.L, h.M, h.T, h.S, h.F) == (t["n"], t["L"], t["M"], t["T"], t["S"], t["F"])
    assert t["prefix"][0] == len(rec) == t["T"] + t["S"] and t["prefix"][t["L"]] == t["T"] + t["F"]
    assert all(a >= b for a, b in zip(t["prefix"], t["prefix"][1:]))
    # r = 0 delivers everything; every r delivers exactly the frame bytes and the levels >= r
    pay, sl, mask = rp.from_progressive(rec, 0)
    assert pay.tobytes() == b"".join(segs) and mask.all() and sl == [len(s) for s in segs]
    for r in range(t["L"] + 1):
        pay, _, mask = rp.from_progressive(rec[:t["prefix"][r]], r, fill=0xA5)
        assert int(mask.sum()) == t["prefix"][r] - t["T"]
        assert np.array_equal(pay[mask], np.frombuffer(b"".join(segs), np.uint8)[mask]) and (pay[~mask] == 0xA5).all()
        with pytest.raises(rp.Refused):
            rp.from_progressive(rec[:t["prefix"][r] - 1], r)


@pytest.mark.parametrize("key", KEYS)
def test_prefix_suffices(vec, key):
    """For every r: the container rebuilt from the first P_r bytes alone, 0xA5 wherever nothing was delivered, decoded by ref_rans and stopped
    behind level r, gives the symbols of the full decode's stages -- with the table rows computed from what that decode itself has decoded."""
    import make_progressive_vectors as mk
    segs, plain, rec, cuts, full = _case(vec, key)
    t = rp.check(rec)
    L = t["L"]
    assert len(full) == 9 * L
    for r in range(L):
        pay, sl, mask = rp.from_progressive(rec[:t["prefix"][r]], r, fill=0xA5)
        if r > 0:
            assert not mask.all(), "the prefix holds the whole record: the case shows nothing"
        pos, part = 0, []
        for ln in sl:
            part.append(pay[pos:pos + ln].tobytes())
            pos += ln
        model = rr.OraclePlanes(part, mk.weights(key))
        got_cuts, stages = rp.ref_cuts(part, model.rows, stop_level=r)
        assert len(stages) == 9 * (L - r) and stages == full[:9 * (L - r)], (key, r)
        assert got_cuts == [tuple(c[max(r, 1) - 1:]) for c in cuts]           # (the cursors of the levels that ran: the same)
    # r = L: the header alone -- the DC band
    pay, sl, mask = rp.from_progressive(rec[:t["prefix"][L]], L)
    assert pay[:sum(sl[:4])].tobytes() == b"".join(segs[:4]) and int(mask.sum()) == t["F"]


def _library():
    from llicti_amd import _lib
    _lib.build()
    return _lib.lib()


def _host_prefix(L_, data):
    out = (C.c_int64 * 6)()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data.ljust(1, b"\0"))
    rc = L_.llicti_progressive_prefix(buf, len(data), out)
    return rc, list(out)


@pytest.mark.parametrize("key", KEYS)
def test_malformed_tables_are_refused(vec, key):
    from llicti_amd import _lib, progressive as pg
    L_ = _library()
    rec = vec[f"{key}_record"].tobytes()
    t = rp.check(rec)
    rc, pre = _host_prefix(L_, rec[:t["T"]])
    assert rc == 0 and pre[:t["L"] + 1] == t["prefix"] and not any(pre[t["L"] + 1:])
    cases = rp.malformed_cases(rec)
    names = {c[0] for c in cases}
    assert {"magic", "version", "n", "L", "zero7", "zero10", "M=0", "M=129", "seg-2^31", "off-2^31", "len-2^31", "cut-2^31", "past-S", "cut>len", "overlap",
            "table-cut-short", "other-model", "S>stride", "r>L", "short-of-P_r"} <= names
    assert ("cuts-descend" in names) == (t["L"] >= 3)
    for name, bad, kw in cases:
        kw = dict(kw)
        kind = kw.pop("kind")
        with pytest.raises(rp.Refused):
            rp.check(bad, **kw)
        if kind == "table":
            assert _host_prefix(L_, bad)[0] == _lib.EFORMAT, name
            with pytest.raises(ValueError):
                pg.parse_head(bad)
    assert L_.llicti_progressive_prefix(None, 0, None) == _lib.EINVAL


def _write_archive(tmp_path, vec, name="t.llpa"):
    from llicti_amd import progressive as pg
    path = str(tmp_path / name)
    recs = [vec[f"{k}_record"].tobytes() for k in KEYS[:2]]
    with pg.ProgressiveWriter(path, 49) as w:
        w.append_records(b"".join(recs), [0, len(recs[0]), len(recs[0]) + len(recs[1])], ["smooth", "noise64"])
        w.append(recs[0])
        with pytest.raises(ValueError):
            w.append(vec[f"{KEYS[2]}_record"].tobytes())                     # a config B record in an archive of 49 segments
        with pytest.raises(ValueError):
            w.append(recs[0][:-1])
    return path, recs


def test_llpa_files(tmp_path, vec):
    from llicti_amd import archive, fileio, progressive as pg
    path, recs = _write_archive(tmp_path, vec)
    with pg.ProgressiveReader(path) as ar:
        assert len(ar) == 3 and ar.names == ["smooth", "noise64", "2"] and ar.sizes == [(67, 93), (33, 40), (67, 93)]
        assert ar.record(1) == recs[1] and ar.record(-1) == recs[0]
        assert [list(map(int, p)) for p in ar.prefix] == [rp.prefixes(recs[0]), rp.prefixes(recs[1]), rp.prefixes(recs[0])]
        assert ar[0] == fileio.loads_llic(pg.to_llic(recs[0]))
        idx, red = [2, 0, 1, 1, 0], [3, 0, 5, 2, 1]                          # scattered, repeated, mixed r
        bt = ar.read_batch(idx, reduce=red, pinned=False)
        want = [recs[[0, 1, 0][i]][:rp.prefixes(recs[[0, 1, 0][i]])[r]] for i, r in zip(idx, red)]
        assert bt.blob.numpy().tobytes() == b"".join(want) and bt.blob.numel() == sum(len(w) for w in want)
        assert bt.rec_off.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()
        assert (bt.Hs, bt.Ws, bt.reduce) == ([67, 67, 33, 33, 67], [93, 93, 40, 40, 93], red)
        S = max(rp.check(r)["S"] for r in recs)
        assert bt.stride == (S + 15) // 16 * 16
        one = ar.read_batch([1], reduce=0, pinned=False)
        assert one.blob.numpy().tobytes() == recs[1] and one.reduce == [0]
        with pytest.raises(ValueError):
            ar.read_batch([0], reduce=6)
        with pytest.raises(IndexError):
            ar.read_batch([3])
    # damaged files
    data = open(path, "rb").read()
    for name, bad in (("magic", data[:-28] + b"LLIA" + data[-24:]), ("version", data[:-24] + b"\x02" + data[-23:]),
                      ("crc", data[:-40] + bytes([data[-40] ^ 1]) + data[-39:]), ("short", data[-20:]), ("cut", data[:-29] + data[-28:])):
        p = str(tmp_path / f"bad_{name}.llpa")
        open(p, "wb").write(bad)
        with pytest.raises(ValueError):
            pg.ProgressiveReader(p)
    with pytest.raises(ValueError):
        archive.ArchiveReader(path)                                          # a .llpa is no .llia


def test_cli_parsers_and_host_side(tmp_path, vec, capsys):
    from llicti_amd import cli, progressive as pg
    a = cli.build_parser().parse_args(["pack", "--progressive", "x.llpa", "a.png", "b.png", "--container", "auto"])
    assert a.progressive and a.container == "auto" and a.src == ["a.png", "b.png"]
    assert not cli.build_parser().parse_args(["pack", "x.llia", "a.png"]).progressive
    assert cli.progressive_container_ok("auto") and cli.progressive_container_ok("xrans3")
    assert not any(cli.progressive_container_ok(c) for c in ("ac", "rans8", "wrans3", "xrans"))
    assert cli.main(["pack", "--progressive", str(tmp_path / "no.llpa"), "a.png", "--container", "ac"]) == 2      # refused before any GPU work
    assert "--container auto" in capsys.readouterr().err
    path, recs = _write_archive(tmp_path, vec)
    assert cli.main(["info", path]) == 0
    out = capsys.readouterr().out
    assert "P_0=%d" % len(recs[0]) in out and "P_5=%d" % rp.prefixes(recs[1])[5] in out
    assert cli.main(["unpack", path, str(tmp_path / "out")]) == 0            # --as llic: through to_llic, no GPU
    assert open(str(tmp_path / "out" / "noise64.llic"), "rb").read() == pg.to_llic(recs[1])


def test_table_code_under_asan_and_ubsan(tmp_path, vec):
    """tests/sanitize_progressive_host.cpp over llicti_amd/csrc/progressive.hpp: g++ with AddressSanitizer + UBSan, run directly, on the
    fixture's records, every malformed table and random tables (its head lists what it holds)."""
    cases = str(tmp_path / "cases.bin")
    n_good = n_bad = 0
    with open(cases, "wb") as fh:
        for key in KEYS:
            rec = vec[f"{key}_record"].tobytes()
            pre = rp.prefixes(rec)
            fh.write(struct.pack("<BI6q", 1, len(rec), *(pre + [0] * (6 - len(pre)))) + rec)
            n_good += 1
            for name, bad, kw in rp.malformed_cases(rec):
                if kw["kind"] == "table":
                    fh.write(struct.pack("<BI6q", 0, len(bad), 0, 0, 0, 0, 0, 0) + bad)
                    n_bad += 1
    exe = str(tmp_path / "sanitize_progressive_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "sanitize_progressive_host.cpp")])
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    m = re.search(r"progressive tables ok: (\d+) good and (\d+) malformed records of the cases file, (\d+) random tables", out.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (n_good, n_bad) and int(m.group(3)) == 4000, out.stdout
