"""The tail census (tests/tail_census.py) over its fixed input list, on the CPU: every stream class of the rANS tail coders is held by at least
two streams of different inputs, every symbol class -- path of the decoder's coder -- by enough symbols, also with the anchors' error bound
doubled; the second reader accepts every container as canonical and the restated tail shape agrees with its facts.  tests/test_hip_tail_edges.py
runs exactly these inputs on the device, so a change of a fixture or a generator that empties a class fails HERE instead of silently turning
that file into a test of ordinary content.  No GPU.

Measured on the list as committed: 0 ambiguous symbols of 47,466 coded tail symbols at the bound, 0 at the doubled bound (the cap is
5 %); the largest spill reached is 352 bits; search13 is not reached (tail_census.SEARCH13_FOUND)."""
from collections import Counter

import tail_census as tc

MIN_STREAM_INPUTS = 2
MIN_SYMBOLS, MIN_EDGE = 16, 4
AMBIGUOUS_CAP = 0.05
REQUIRED_STREAM = tuple(tc.all_stream_classes())                # none dropped
REQUIRED_SYMBOL = tuple(c for c in tc.SYMBOL_CLASSES if c not in ("ambiguous", "search13")) + (("search13",) if tc.SEARCH13_FOUND else ())

_result = {}


def _run():
    if not _result:
        inputs_of = {c: set() for c in REQUIRED_STREAM}
        sym = [Counter(), Counter()]
        max_spill, gap = 0, 0.0
        for inp in tc.INPUTS:
            bl = tc.oracle_container(inp)
            # (census decodes with canonical=True and holds the image and the restated shape against the reader: it raises where they differ)
            streams, (s1, s2), extra = tc.census(bl, tc.oracle_weights(inp[4]), bound_scale=[1.0, 2.0], image=tc.image_of(*inp[:5]))
            assert (extra["header"]["L"], extra["header"]["M"]) == ((64, 128, 256)[inp[5]], inp[6]), inp
            for c in streams:
                inputs_of[c].add(inp)
            sym[0].update(s1)
            sym[1].update(s2)
            max_spill, gap = max(max_spill, extra["max_spill"]), max(gap, extra["anchor_gap"])
        _result.update(inputs_of=inputs_of, sym=sym, max_spill=max_spill, gap=gap)
    return _result


def test_input_list_is_fixed_and_small():
    assert len(set(tc.INPUTS)) == len(tc.INPUTS)
    big = [i for i in tc.INPUTS if i[1] > 70 or i[2] > 100]
    assert all(i[:3] == ("flat", 181, 181) for i in big), big      # the one larger image, flat: 90 x 91 = 8,190 >= 8,160 symbols on one stream
    assert all(32 <= i[1] and 32 <= i[2] for i in tc.INPUTS)
    assert (181 // 2) * ((181 + 1) // 2) >= 8160


def test_every_tail_class_is_held():
    r = _run()
    coded = r["sym"][0]["coded"]
    print("stream classes (inputs that hold one):")
    for c in REQUIRED_STREAM:
        print("  %-14s %3d" % (c, len(r["inputs_of"][c])))
    print("symbol classes of %d coded tail symbols (at the bound / at twice the bound):" % coded)
    for c in tc.SYMBOL_CLASSES:
        print("  %-14s %6d %6d" % (c, r["sym"][0][c], r["sym"][1][c]))
    print("ambiguous share %.4f %% (%.4f %% at twice the bound); largest spill %d bits; largest |float64 anchor - exact entry| / (bound + 1) = %.3f"
          % (100.0 * r["sym"][0]["ambiguous"] / coded, 100.0 * r["sym"][1]["ambiguous"] / coded, r["max_spill"], r["gap"]))
    short = [c for c in REQUIRED_STREAM if len(r["inputs_of"][c]) < MIN_STREAM_INPUTS]
    assert not short, short
    for k in (0, 1):                                       # the minimum counts hold with the bound doubled, too
        s = r["sym"][k]
        low = [c for c in REQUIRED_SYMBOL if s[c] < (MIN_EDGE if c.startswith("d=") else MIN_SYMBOLS)]
        assert not low, (k, low, dict(s))
    assert r["sym"][0]["ambiguous"] <= AMBIGUOUS_CAP * coded
    assert r["max_spill"] >= 32
    # the restated anchors are the exact entries up to the approximation: a wrong component or constant here would be off by hundreds of counts
    assert r["gap"] <= 1.0, r["gap"]
    # search13 joins the required set as soon as an input reaches it
    assert tc.SEARCH13_FOUND == (r["sym"][1]["search13"] > 0), r["sym"][1]["search13"]


def test_restated_shape_matches_the_library_rule():
    """tail_shape against hand-worked shapes (host_types.hpp's rule: n raw symbols per chain of two, the stream's last symbol for one chain)"""
    assert tc.tail_shape(100, 40, 2, 3) == (3, 6, 34)
    assert tc.tail_shape(100, 40, 1, 3) == (1, 1, 39)
    assert tc.tail_shape(1, 1, 1, 31) == (1, 1, 0)
    assert tc.tail_shape(0, 0, 1, 3) == (1, 0, 0)
    assert tc.tail_shape(100, 40, 1, 0, False) == (0, 0, 40)
    assert [tc.chain_count(7, 2, c) for c in (0, 1)] == [4, 3] and tc.chain_count(7, 1, 0) == 7
