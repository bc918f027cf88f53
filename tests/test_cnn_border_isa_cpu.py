"""Staging a border tile of the band CNN must stay cheap: instructions per 64-float piece, counted from the device assembly (no GPU needed).

The parent of the build that introduced the unrolled border path staged every piece of a border tile through a rolled loop of 71 instructions
(27 vector, 43 scalar, 1 LDS-DMA) that re-derived the piece's plane, row group and phase with runtime divisions and redid both clamps per lane.
tools/cnn_border_isa.py counts the border path of a -DCNN_STAGE_FAST=0 build (every staging instruction of the tile loop is then the border
path's); profiles/r8/cnn_border_isa.json holds the figures of that parent and of the build that replaced the loop.  A regression guard: the
acceptance was the measured time (profiles/r8/ab_cnn_border.json)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_LOOP = 71


@pytest.fixture(scope="module")
def table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import cnn_border_isa
    finally:
        sys.path.pop(0)
    return cnn_border_isa.parse(cnn_border_isa.device_asm())


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(ROOT, "profiles", "r8", "cnn_border_isa.json")))


def test_every_instantiation_is_counted(table, recorded):
    names = sorted(k["kernel"] for k in table)
    assert len(names) == 36 and names == sorted(k["kernel"] for k in recorded["new"]), names
    for k in table:
        assert k["sites"] == 4, k                                   # CNN_STAGE_SITES staging sites in the tile loop
        assert k["pieces"] == k["wave_pieces"], k                   # every piece of a wave has its unrolled request
        assert k["loop"] is not None and k["loop"]["dma"] == 1, k   # and the general formula is ONE rolled loop behind them


def test_border_piece_no_dearer_than_recorded_and_cheaper_than_the_parents_loop(table, recorded):
    rec = {k["kernel"]: k for k in recorded["new"]}
    assert min(k["loop"]["total"] for k in recorded["parent"]) >= PARENT_LOOP - 3          # (the record's parent is the 71-instruction loop; 68 in the 4-row forms)
    for k in table:
        r = rec[k["kernel"]]
        assert k["per_piece"] <= r["per_piece"], (k["kernel"], k["per_piece"], r["per_piece"])
        assert k["per_piece"] < PARENT_LOOP, (k["kernel"], k["per_piece"])
        assert k["loop"]["total"] <= r["loop"]["total"], (k["kernel"], k["loop"], r["loop"])
