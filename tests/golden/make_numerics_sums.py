"""tests/golden/numerics_sums.npz: the CPU oracle's erfc_spec over ALL 2^32 fp32 bit patterns, reduced to sums, and its error against
float64 erfc, per chunk of 2^20 consecutive patterns (tests/numerics_sums_host.c says what a chunk, S1 and S2 are).

  erfc_s1, erfc_s2          uint64 [4096]   the two sums of bits(erfc_spec(u)) modulo 2^64
  erfc_min, erfc_max        uint32 [4096]   smallest / largest output word of the chunk
  rel_max, rel_arg          float64 / uint32 [4096]   largest |f - erfc| / erfc over 0 <= x < 7 of the chunk, and the bits of its x
  abs_max, abs_arg          the same for |f - erfc| over x < 0
  ratio_max, ratio_arg      the same for error / budget over every x that is no NaN
  budget_rel, budget_tail   float64   tests/ref64.py's ERFC_REL and ERFC_TAIL the ratios were taken against
  recip_chunk0, recip_s1, recip_s2   the two sums of bits(1.0f / d) over the floats of [2, 9], for chunks recip_chunk0 .. + 17
  oracle_sha256             numerics_sums.oracle_sha256() of the oracle the sums come from

Generated from this project's oracle alone.  The file is written with fixed zip time stamps, so a second run on the same oracle and libm
reproduces it byte for byte.  Measured: 42 s for `all` with 8 threads on 8 CPUs (two runs: 42.8 s, 41.8 s).

    python tests/golden/make_numerics_sums.py [--check]       (--check: generate, compare with the committed file, write nothing)
"""
import io
import os
import sys
import tempfile
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import numerics_sums as ns  # noqa: E402
import ref64  # noqa: E402


def npz_bytes(arrays):
    """An .npz (deflated) whose bytes depend on the arrays alone: fixed member order and time stamps."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())
    return buf.getvalue()


def generate():
    with tempfile.TemporaryDirectory() as tmp:
        exe = ns.build_host(tmp)
        t0 = time.time()
        r = ns.run_host(exe, ["all"], timeout=3600)
        dt = time.time() - t0
    assert np.array_equal(r["chunk"], np.arange(ns.NCHUNKS))
    assert sorted(r["recip"]) == list(range(ns.RECIP_CHUNK0, ns.RECIP_CHUNK0 + ns.RECIP_NCHUNKS))
    rs = [r["recip"][c] for c in sorted(r["recip"])]
    arrays = {
        "erfc_s1": r["s1"], "erfc_s2": r["s2"], "erfc_min": r["min"], "erfc_max": r["max"],
        "rel_max": r["rel"], "rel_arg": r["rel_arg"], "abs_max": r["abs"], "abs_arg": r["abs_arg"],
        "ratio_max": r["ratio"], "ratio_arg": r["ratio_arg"],
        "budget_rel": np.float64(ref64.ERFC_REL), "budget_tail": np.float64(ref64.ERFC_TAIL),
        "recip_chunk0": np.int64(ns.RECIP_CHUNK0),
        "recip_s1": np.array([a for a, _ in rs], np.uint64), "recip_s2": np.array([b for _, b in rs], np.uint64),
        "oracle_sha256": np.array(ns.oracle_sha256()),
    }
    return npz_bytes(arrays), r, dt


def main():
    data, r, dt = generate()
    i, j, k = int(r["rel"].argmax()), int(r["abs"].argmax()), int(r["ratio"].argmax())
    print(f"all 2^32 inputs in {dt:.1f} s ({os.environ.get('OMP_NUM_THREADS', '8')} threads); {len(data)} bytes")
    print(f"largest relative error on [0, 7): {r['rel'][i]:.6g} at x = {ns.bits_to_float(r['rel_arg'][i])!r} (0x{int(r['rel_arg'][i]):08x})")
    print(f"largest absolute error below 0:   {r['abs'][j]:.6g} at x = {ns.bits_to_float(r['abs_arg'][j])!r} (0x{int(r['abs_arg'][j]):08x})")
    print(f"largest error / budget:           {r['ratio'][k]:.6g} at x = {ns.bits_to_float(r['ratio_arg'][k])!r} (0x{int(r['ratio_arg'][k]):08x})")
    if "--check" in sys.argv[1:]:
        same = open(ns.FIXTURE, "rb").read() == data
        print("committed fixture reproduced byte for byte" if same else "DIFFERS from the committed fixture")
        return 0 if same else 1
    with open(ns.FIXTURE, "wb") as f:
        f.write(data)
    print(ns.FIXTURE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
