"""The rANS tail coders on every tail shape and window edge (run with -m gpu on an MI355X): exactly tail_census.INPUTS, whose stream and symbol
classes tests/test_tail_census_cpu.py computes and asserts -- one or two chains, pooled preparing wavefronts, every residue of the last round,
seeds, spills across the payload's end, windows hit, missed by one on either side, clipped at entry 0 and at the top symbol.  Nothing in the
library is switched, forced or observed, and every input is a sound container.  Per input: the device's container is the oracle's byte for
byte and decodes, on a poisoned workspace, to the image with a clean status; the same in mixed-size batches with each input's own stream
count, under a per-image reduce list, and through the second reader of the format."""
import numpy as np
import pytest

import ref_rans as rr
import tail_census as tc

pytestmark = pytest.mark.gpu

GROUPS = {}
for _inp in tc.INPUTS:
    GROUPS.setdefault((_inp[1], _inp[2], _inp[4], _inp[5], _inp[6]), []).append(_inp)
GROUP_KEYS = sorted(GROUPS)

_codecs = {}


@pytest.fixture(scope="module")
def codec_of():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llicti_amd.codec import HipCodec

    def get(wname):
        if wname not in _codecs:
            c = HipCodec("cuda:0")
            c.load_state_dict(tc.state_dict(wname))
            _codecs[wname] = c
        return _codecs[wname]
    yield get
    for c in _codecs.values():
        c.close()
    _codecs.clear()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")          # (a writable copy: the census keeps its images read-only)


def _mode(inp):
    from llicti_amd.codec import MODE_RANS
    return MODE_RANS(inp[6], wide=inp[5])


def _image(inp):
    return tc.image_of(*inp[:5])


def _of_kind(wide):
    """the inputs of one lane kind under the weight set that has the most of them"""
    by = {}
    for inp in tc.INPUTS:
        if inp[5] == wide:
            by.setdefault(inp[4], []).append(inp)
    return max(sorted(by.items()), key=lambda kv: len(kv[1]))


@pytest.mark.parametrize("key", GROUP_KEYS, ids=lambda k: "%dx%d-%s-%s%d" % (k[0], k[1], k[2].replace(":", "_"), tc.KIND_NAME[k[3]], k[4]))
def test_tail_edges_input_group(codec_of, key):
    """one call per (size, weights, mode): encode == the oracle's bytes, poisoned decode == the pixels, clean"""
    import torch
    from llicti_amd.codec import container_to_bytestream_list
    H, W, wname = key[:3]
    group = GROUPS[key]
    c = codec_of(wname)
    mode = _mode(group[0])
    x = _dev(np.stack([_image(i) for i in group]))
    cont, seg = c.encode(x, mode=mode)
    c.check()
    cont_h, seg_h = cont.cpu().numpy(), seg.cpu().numpy()
    for b, inp in enumerate(group):
        assert container_to_bytestream_list(cont_h[b], seg_h[b]) == tc.oracle_container(inp), inp
    c.workspace(len(group), H, W, mode)
    c.poison_workspace(0xA5)
    rec = c.decode(cont, seg, H, W, mode=mode)
    c.check()
    assert torch.equal(rec, x), (key, int((rec != x).sum()))
    assert not c.image_status(len(group)).any(), key


def _batch(c, group):
    """the mixed-size batch of `group` in one encode_v call with each input's own mode -> (flat pixels, Hs, Ws, modes, containers, seg_len)"""
    Hs, Ws = [i[1] for i in group], [i[2] for i in group]
    modes = np.array([_mode(i) for i in group], dtype=np.int32)
    flat = _dev(np.concatenate([_image(i).reshape(-1) for i in group]))
    cont, seg = c.encode_v(flat, Hs, Ws, modes)
    c.check()
    return flat, Hs, Ws, modes, cont, seg


@pytest.mark.parametrize("wide", (2, 0, 1), ids=("xwide", "narrow", "wide"))
def test_tail_edges_mixed_batch(codec_of, wide):
    """all inputs of one lane kind and weight set in ONE call, each with its own stream count: every container is the solo one (the oracle's,
    which test_tail_edges_input_group holds the solo call to), the decode on a poisoned workspace is lossless and clean"""
    import torch
    from llicti_amd.codec import container_to_bytestream_list
    wname, group = _of_kind(wide)
    assert len(group) >= 2, (wide, group)
    c = codec_of(wname)
    flat, Hs, Ws, modes, cont, seg = _batch(c, group)
    cont_h, seg_h = cont.cpu().numpy(), seg.cpu().numpy()
    for b, inp in enumerate(group):
        assert container_to_bytestream_list(cont_h[b], seg_h[b]) == tc.oracle_container(inp), inp
    c.workspace_v(Hs, Ws, modes)
    c.poison_workspace(0xA5)
    rec = c.decode_v(cont, seg, Hs, Ws, modes)
    c.check()
    assert torch.equal(rec, flat), (wide, int((rec != flat).sum()))
    assert not c.image_status(len(group)).any()


def test_tail_edges_per_image_reduce(codec_of):
    """the xwide batch under a reduce list that mixes 0 with 1 and 2: the tail runs over the stream list of the r = 0 subset; those images are
    the originals, the others what the scalar call at their value gives, every status clean"""
    from llicti_amd.codec import reduced_dims
    wname, group = _of_kind(2)
    c = codec_of(wname)
    flat, Hs, Ws, modes, cont, seg = _batch(c, group)
    B = len(group)
    red = [(0, 1, 0, 2, 0)[b % 5] for b in range(B)]
    assert red.count(0) >= 2 and 0 < red.count(0) < B
    scalar = {}
    for r in sorted(set(red) - {0}):
        c.workspace_v(Hs, Ws, modes)
        c.poison_workspace(0xA5)
        scalar[r] = c.decode_v(cont, seg, Hs, Ws, modes, reduce=r).cpu().numpy()
        c.check()
    c.workspace_v(Hs, Ws, modes)
    c.poison_workspace(0xA5)
    got = c.decode_v(cont, seg, Hs, Ws, modes, reduce=red).cpu().numpy()
    c.check()
    assert not c.image_status(B).any()
    pos = 0
    spos = dict.fromkeys(scalar, 0)
    for b, inp in enumerate(group):
        h, w = reduced_dims(Hs[b], Ws[b], red[b])
        n = 3 * h * w
        if red[b] == 0:
            assert np.array_equal(got[pos:pos + n].reshape(3, h, w), _image(inp)), inp
        for r in scalar:
            hr, wr = reduced_dims(Hs[b], Ws[b], r)
            if r == red[b]:
                assert np.array_equal(got[pos:pos + n], scalar[r][spos[r]:spos[r] + n]), (inp, r)
            spos[r] += 3 * hr * wr
        pos += n
    assert pos == got.size


@pytest.mark.parametrize("wide", (0, 1, 2), ids=("narrow", "wide", "xwide"))
def test_tail_edges_second_reader(codec_of, wide):
    """one input per stream kind (xwide: a one-chain and a two-chain input): the DEVICE's container through the second reader, canonical"""
    from oracle import oracle as orc
    from llicti_amd.codec import container_to_bytestream_list
    picks = [next(i for i in tc.INPUTS if i[5] == wide and i[1] <= 70)]
    if wide == 2:
        picks = [("noise", 70, 100, 3, "trainedlike", 2, 7), ("smooth", 64, 96, 9, "trainedlike", 2, 1)]
        assert all(p in tc.INPUTS for p in picks)
    for inp in picks:
        c = codec_of(inp[4])
        cont, seg = c.encode(_dev(_image(inp)[None]), mode=_mode(inp))
        c.check()
        segs = rr.segments(container_to_bytestream_list(cont[0].cpu().numpy(), seg[0].cpu().numpy()))
        planes, info = rr.decode_image(segs, rr.OraclePlanes(segs, tc.oracle_weights(inp[4])), canonical=True)
        assert np.array_equal(orc.unlift(planes), _image(inp)), inp
        kinds = {tc.stream_kind(info["header"], f) for f in info["streams"] if f["share"]}
        assert kinds <= ({"N"}, {"W"}, {"X1", "X2"})[wide], (inp, kinds)
