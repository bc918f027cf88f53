"""The band CNN's tile loop may wait for vector memory at ONE place: the explicit drain in front of the tile's barrier.

The input staging is LDS-DMA (global_load_lds), tracked by vmcnt.  A second s_waitcnt with a vmcnt field inside the loop -- one the compiler
inserts in front of a ds_read because it cannot tell the buffer being filled from the one being read, or because a spilled register comes
back through scratch memory (an ordinary vector-memory load beside LDS-DMA in flight is waited for with vmcnt(0)) -- stalls a wavefront for
a memory round trip per tile and drains the DMA the kernel wants in flight.  hipcc's device assembly is the witness (no GPU needed);
tools/cnn_wait_audit.py parses it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def audit(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import cnn_wait_audit
        from kernel_resources import FLAGS, SRC
    finally:
        sys.path.pop(0)
    out = str(tmp_path_factory.mktemp("isa") / "llicti.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-S", "--cuda-device-only", "-o", out, SRC], stderr=subprocess.DEVNULL)
    return cnn_wait_audit, cnn_wait_audit.parse(out)


def test_every_instantiation_is_audited(audit):
    _, table = audit
    names = [k["kernel"] for k in table]
    assert len([n for n in names if "band_params_kernel" in n]) == 18, names         # 3 bands x {16, 8, 4} tile rows x {equal, mixed} sizes
    assert len([n for n in names if "band_params_h60_kernel" in n]) == 18, names
    for k in table:
        assert k["barriers"] == 1 and k["dma_in_loop"] >= 1, k


def test_one_vmcnt_wait_per_tile_in_front_of_the_barrier(audit):
    mod, table = audit
    for k in table:
        waits = mod.merged(k["waits"])
        assert len(waits) == 1, (k["kernel"], k["waits"])
        assert waits[0]["vmcnt"] == 0 and waits[0]["next"] == "s_barrier", (k["kernel"], k["waits"])
        # the drain is the first vector-memory event of a pass through the loop: every request and store of the pass before it is retired there
        assert waits[0]["dma_since"] == 0 and waits[0]["stores_since"] == 0, (k["kernel"], k["waits"])
