"""The band CNN's tile loop re-derives no LDS address with vector adds beside its MFMAs.

A vector instruction takes the SIMD's vector issue port for 4 cycles -- the port the MFMAs issue through -- and with four waves per SIMD keeping
the matrix pipe busy nothing hides it.  hipcc's device assembly is the witness (no GPU needed); tools/cnn_valu_audit.py counts, per
band_params*_kernel instantiation, the vector instructions of the basic blocks that hold the tile's MFMAs and the literal adds that re-derive an
LDS address in front of a ds_read.  (It lists the params stores' address products and 64-bit adds too; they are not bounded here: a scalar-base
form of the stores was built and taken out again, its gain alone did not show beside the run-to-run spread -- DESIGN.md section 8, round 10.)
profiles/r10/cnn_valu_audit_parent.json and cnn_valu_audit.json hold the tables of the build before and the build that took the LDS adds out."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (config, band, tile rows, mixed sizes) -> non-MFMA vector instructions of the MFMA-holding blocks per wave and tile, as measured on the build that
# introduced this test; a ratchet, not a prediction.  (88 / 60 of them are the ReLU's v_med3_f32; the 4-row forms add as many v_accvgpr_read.)
VALU = {                                # before
    ('A', 0, 16, False): 121, # 138
    ('A', 1, 16, False): 122, # 131
    ('A', 2, 16, False): 122, # 221
    ('A', 0, 8, False): 121, # 134
    ('A', 1, 8, False): 122, # 130
    ('A', 2, 8, False): 122, # 166
    ('A', 0, 4, False): 209, # 222
    ('A', 1, 4, False): 210, # 219
    ('A', 2, 4, False): 211, # 253
    ('A', 0, 16, True): 119, # 136
    ('A', 1, 16, True): 120, # 129
    ('A', 2, 16, True): 120, # 216
    ('A', 0, 8, True): 119, # 132
    ('A', 1, 8, True): 120, # 128
    ('A', 2, 8, True): 120, # 164
    ('A', 0, 4, True): 207, # 220
    ('A', 1, 4, True): 208, # 217
    ('A', 2, 4, True): 209, # 251
    ('B', 0, 16, False): 78,  # 79
    ('B', 1, 16, False): 79,  # 82
    ('B', 2, 16, False): 79,  # 93
    ('B', 0, 8, False): 78,  # 81
    ('B', 1, 8, False): 79,  # 84
    ('B', 2, 8, False): 79,  # 91
    ('B', 0, 4, False): 140, # 142
    ('B', 1, 4, False): 141, # 144
    ('B', 2, 4, False): 141, # 151
    ('B', 0, 16, True): 76,  # 77
    ('B', 1, 16, True): 77,  # 80
    ('B', 2, 16, True): 77,  # 91
    ('B', 0, 8, True): 76,  # 79
    ('B', 1, 8, True): 77,  # 82
    ('B', 2, 8, True): 77,  # 89
    ('B', 0, 4, True): 138, # 140
    ('B', 1, 4, True): 139, # 142
    ('B', 2, 4, True): 139, # 149
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import cnn_valu_audit
        import cnn_wait_audit
        from kernel_resources import FLAGS, SRC
    finally:
        sys.path.pop(0)
    out = str(tmp_path_factory.mktemp("isa") / "llicti.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-S", "--cuda-device-only", "-o", out, SRC], stderr=subprocess.DEVNULL)
    return cnn_valu_audit.parse(cnn_wait_audit.kernels(out))


def _key(k):
    return (k["config"], k["band"], k["rows"], k["mixed"])


def test_every_instantiation_is_audited(table):
    assert sorted(_key(k) for k in table) == sorted(VALU), [k["kernel"] for k in table]
    for k in table:
        want = {("A", 0): 476, ("A", 1): 560, ("A", 2): 728, ("B", 0): 246, ("B", 1): 294, ("B", 2): 390}[(k["config"], k["band"])]
        assert k["mfma"] == want and k["stores"] == 8, k


def test_no_lds_address_beyond_the_offset_field(table):
    """no ds_read address is base + a literal of 64 KB or more anywhere in a kernel (before: 54 in config A's 16-row band 2), and at most 4 literal
    adds per tile feed LDS reads at all (before: 33 / 26 / 114 in config A's 16-row forms): re-basing once per phase is what is left"""
    for k in table:
        assert k["lit_add_ds_hi"] == 0, (k["kernel"], k["lit_add_ds_hi"])
        assert k["lit_add_ds"] <= 4, (k["kernel"], k["lit_add_ds"], k["lit_add_ds_by_block"])


def test_vector_instructions_beside_the_mfmas_do_not_grow(table):
    for k in table:
        assert k["valu"] <= VALU[_key(k)], (k["kernel"], k["valu"], VALU[_key(k)], k["valu_by_op"])
