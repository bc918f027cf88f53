"""The scalar functions of llicti_amd/csrc/numerics.hpp over every fp32 input, on the GPU: tests/numerics_probe.hip (a stand-alone program
that includes the header itself and is built with the library's flags) is run once, in a child process, and what it reports is held against
the CPU oracle's side of the same sweep (tests/golden/numerics_sums.npz, guarded by tests/test_numerics_cpu.py).  Each claim the kernels
rest on is its own test:
  * erfc_spec on the device has the oracle's bits on all 2^32 inputs (two sums per chunk of 2^20 inputs);
  * erfc_spec_nobranch (mix_cdf: the pairs kernel, the decoders, cdf_entry) has erfc_spec's bits (the table and likelihood kernels) everywhere;
  * recip_2_9 is the IEEE division 1.0f / d on every float of [2, 9], and the device's division is the host's;
  * div255_exact is the division by 255.0f on every regular sample point and every plane value."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import numerics_sums as ns

pytestmark = pytest.mark.gpu


def _probe_exe():
    from llicti_amd import _lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if os.path.exists(hipcc) or shutil.which(hipcc):
        return _lib.build_probe()                   # (a no-op when __graft_entry__.build() has made it and nothing changed since)
    if os.path.exists(_lib.PROBE_PATH):
        return _lib.PROBE_PATH
    pytest.skip("no hipcc on this box and no prebuilt tests/numerics_probe")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """One run of the probe: its JSON, the per-chunk sums it wrote beside it, the executable."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    exe = _probe_exe()
    sums = str(tmp_path_factory.mktemp("numerics_probe") / "erfc_sums.bin")
    r = subprocess.run([exe, "--out", sums], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    rep = json.loads(r.stdout)
    assert rep["chunks"] == ns.NCHUNKS and rep["chunk_bits"] == ns.CHUNK_BITS and rep["sums_file"] == sums
    s = np.fromfile(sums, dtype="<u8")
    assert s.size == 2 * ns.NCHUNKS
    print(f"numerics_probe: erfc sweep of 2^32 inputs {rep['erfc_sweep_ms']:.1f} ms, all sweeps with copies {rep['wall_ms']:.1f} ms")
    return {"rep": rep, "s1": s[:ns.NCHUNKS], "s2": s[ns.NCHUNKS:], "exe": exe}


@pytest.fixture(scope="module")
def fx():
    return np.load(ns.FIXTURE)


def _first_difference(probe, chunk, tmp_path):
    """One more child process each side: the device's and the oracle's output words of the chunk -> a message naming the first input that differs."""
    dev_path = str(tmp_path / "dev.bin")
    r = subprocess.run([probe["exe"], "--dump", str(chunk), dev_path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    dev = np.fromfile(dev_path, dtype="<u4")
    host = ns.host_dump(ns.build_host(tmp_path), chunk, tmp_path / "host.bin")
    d = np.flatnonzero(dev != host)
    if d.size == 0:
        return f"chunk {chunk}: the sums differ but the dumps agree"
    u = (chunk << ns.CHUNK_BITS) + int(d[0])
    return (f"chunk {chunk}: {d.size} of 2^20 outputs differ, first at x = {ns.bits_to_float(u)!r} (0x{u:08x}): "
            f"device 0x{int(dev[d[0]]):08x}, oracle 0x{int(host[d[0]]):08x}")


def test_device_erfc_sums_equal_oracle(probe, fx, tmp_path):
    """numerics.hpp's erfc_spec == the oracle's erfc_spec, bit for bit, on all 2^32 inputs: S1 and S2 of each of the 4096 chunks."""
    bad = np.flatnonzero((probe["s1"] != fx["erfc_s1"]) | (probe["s2"] != fx["erfc_s2"]))
    if bad.size:
        pytest.fail(f"{bad.size} of {ns.NCHUNKS} chunks differ (first {list(bad[:8])}); " + _first_difference(probe, int(bad[0]), tmp_path))


def test_erfc_nobranch_has_erfc_spec_bits(probe):
    """bits(erfc_spec_nobranch(x)) == bits(erfc_spec(x)) for every fp32 x (NaNs, infinities, both zeros, denormals included): an input
    where they differed would be an encoder / decoder disagreement waiting for an image that reaches it."""
    rep = probe["rep"]
    assert rep["nobranch_mismatches"] == 0, (rep["nobranch_mismatches"], hex(rep["nobranch_first"]), ns.bits_to_float(rep["nobranch_first"]))


def test_recip_2_9_is_the_division(probe, fx):
    """recip_2_9(d) == 1.0f / d bit for bit on each of the 17,825,793 floats of [2, 9] with the compiler that built the library, and that
    device division is the host's IEEE division (the oracle's 1 / (x + 2)): a compiler that expands the division differently shows here."""
    rep = probe["rep"]
    assert rep["recip_checked"] == ns.RECIP_HI - ns.RECIP_LO + 1 == 17_825_793
    assert rep["recip_mismatches"] == 0, (rep["recip_mismatches"], hex(rep["recip_first"]), ns.bits_to_float(rep["recip_first"]))
    assert rep["recip_chunk0"] == int(fx["recip_chunk0"])
    assert [int(v, 16) for v in rep["recip_s1"]] == [int(v) for v in fx["recip_s1"]]
    assert [int(v, 16) for v in rep["recip_s2"]] == [int(v) for v in fx["recip_s2"]]


def test_div255_exact_is_the_division(probe):
    """div255_exact(x) == x / 255.0f on the device == numpy's float32 division, for every half-integer |x| <= 350 (1401 values: every regular
    sample point of any table) and every integer |v| <= 255 (511 values: every plane value) -- the kernels use the two forms side by side
    (cdf.hpp's pairs and table kernels, the rANS coder, the lift)."""
    rep = probe["rep"]
    x = np.array(rep["div255_x"], dtype=np.uint32).view(np.float32)
    want_x = np.concatenate([np.arange(-700, 701, dtype=np.float32) * np.float32(0.5), np.arange(-255, 256, dtype=np.float32)])
    assert x.size == 1401 + 511 and np.array_equal(x.view(np.uint32), want_x.view(np.uint32))
    exact = np.array(rep["div255_exact"], dtype=np.uint32)
    div = np.array(rep["div255_div"], dtype=np.uint32)
    ref = (x / np.float32(255)).astype(np.float32).view(np.uint32)
    bad = np.flatnonzero(exact != div)
    assert bad.size == 0, (x[bad][:5], exact[bad][:5], div[bad][:5])
    bad = np.flatnonzero(div != ref)
    assert bad.size == 0, (x[bad][:5], div[bad][:5], ref[bad][:5])
