"""Every entry point of the C-ABI on a CALLER'S stream, behind a gated queue (run with -m gpu on an MI355X).

include/llicti_hip.h promises that launches are asynchronous on `stream`.  On the null stream every wait the host side makes to keep that promise
does nothing, and a kernel, copy or event that went to stream 0 instead of `stream` gives the same bytes there.  Here every call runs on a
torch.cuda.Stream() -- non-blocking: the null stream does not synchronise with it -- and a GATE (helpers.StreamGate) makes ordering bugs
deterministic.  A gated run (class Run):
  1. the call's input buffers hold a DECOY, another valid input of the same shape and mode; the outputs a poison fill
  2. a spin kernel holds the gated stream busy for GATE_MS
  3. the real input is copied over the decoy on `s`, device to device
  4. the call under test is made on `s`
  5. its outputs are copied into fresh buffers on `s`
  6. PRECONDITION: the gate's end event has not fired -- the gate was still running when the last launch had been enqueued
  7. `s` is synchronised and the copies are compared with a yardstick that is never the code under test on another stream: the CPU oracle's
     containers, lifts, parameters, tables and coder output, the original pixels, tests/ref64.py and tests/ref_rans.py.
Variant "s" gates `s` itself: work of the call that is not ordered behind `s` runs early and sees the decoy (wrong but valid), work not joined back
onto `s` is missed by step 5 (poison).  Variant "null" gates the null stream and runs the call on an idle `s`: stray null-stream work is late.
No host synchronisation lies between steps 2 and 6, and the library never sees an invalid input (but for the one known-flagged header of case 5).

Two NEGATIVE CONTROLS make the same gated sequence but issue the call on the default stream: the result must be the decoy's.  HIP maps streams
onto 4 hardware queues; two streams that share one serialise, which can hide a misplaced launch (never invent one), so the module makes six
streams and takes as `s` the first on which the encode control detects.

GATE LENGTH.  Host wall time from the gate's launch to the last enqueue, measured on an MI355X host over the whole file (every run's time is
kept; the module prints the longest when it is done):
  warm context (plan hits, 73 runs):                          longest 3.1 ms  (the kernel-level chain: 2 levels x 3 bands x 3 colours x 2 images,
                                                              about 200 launches and copies; every whole-batch call is below 1.6 ms)
  first call of a new shape (plan build + upload, 28 runs):   longest 3.5 ms  (the eviction case: 36 encodes behind one gate, two of them new plans
                                                              that allocate a table block; a single first call is below 0.9 ms)
GATE_MS = 100 is 28 x the larger.  The first use of a kernel or a torch operator in a process loads its code (130 ms for the kernel-level chain):
the chain and the control make one ungated pass over the decoy first, so the gate times enqueues.  Step 6 fails any run whose enqueue outlasts it.

The eviction case of "one context, streams in turn" runs on a context of its own: it asserts what the block pool does, to the block, which needs a
pool whose history the test knows."""
import ctypes as C
import time

import numpy as np
import pytest

import ref64
import ref_rans as rr
from conftest import load_state_dict
from helpers import StreamGate, make_image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0xA5
GATE_MS = 100.0
VARIANTS = ["s", "null"]
ENQUEUE_MS = {"warm": [], "first": []}          # host time of every gated enqueue sequence (printed when the module is done)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def new_codec(torch, wname):
    """A context with its weights, WARM for gated calls: the first decode of a context allocates its per-image status words behind a device-wide
    synchronise (include/llicti_hip.h, "calls that BLOCK"), which a gated run must not meet."""
    from llicti_amd.codec import HipCodec
    c = HipCodec(DEV)
    if wname.startswith("b_"):
        c.set_model(60, 2)
    c.load_state_dict(load_state_dict(wname))
    rgb = _dev(torch, make_image("noise", 32, 32, 1)[None])
    cont, seg = c.encode(rgb)
    assert torch.equal(c.decode(cont, seg, 32, 32), rgb)
    c.check()
    return c


@pytest.fixture(scope="module")
def codecs(torch_mod):
    cache = {}

    def get(wname):
        if wname not in cache:
            cache[wname] = new_codec(torch_mod, wname)
        return cache[wname]
    yield get
    for c in cache.values():
        c.set_tuning("ac_anchor_min_batch", 96)
        c.set_tuning("enc_side_levels", 0)
        c.set_profiling(False)
        c.close()
    for k, v in ENQUEUE_MS.items():
        if v:
            print(f"\ngated enqueue sequences, {k}: {len(v)} runs, longest {', '.join('%.1f' % t for t in sorted(v)[-4:][::-1])} ms (gate {GATE_MS:.0f} ms)")


class Env:
    pass


@pytest.fixture(scope="module")
def env(torch_mod, codecs, oracle_weights):
    """The gate, and the streams: `s` is the first of six on which the encode negative control detects a call issued on the default stream."""
    torch = torch_mod
    e = Env()
    e.torch = torch
    e.gate = StreamGate(torch, DEV)
    e.streams = [torch.cuda.Stream(device=DEV) for _ in range(6)]
    e.s, e.tried = None, []
    # (the first use of a kernel or a torch operator loads its code: an ungated pass of what the control enqueues, so that the gate times enqueues)
    c = codecs("trainedlike")
    with torch.cuda.stream(e.streams[0]):
        cont, _ = c.encode(_dev(torch, batch(64, 96, (12, 13))), mode=_mode("xrans2"))
        cont.clone().copy_(torch.full_like(cont, POISON), non_blocking=True)
    torch.cuda.synchronize()
    c.check()
    for k, s in enumerate(e.streams):
        e.s = s
        seen = _control_encode(e, codecs("trainedlike"), oracle_weights("trainedlike"))
        e.tried.append((k, seen))
        if seen == "decoy":
            break
    e.index = k
    e.s2 = e.streams[(k + 1) % len(e.streams)]                     # the second stream of "streams in turn": always ordered against `s` by the caller
    print(f"\nnegative control (encode) per candidate stream: {e.tried}; `s` = stream {k} of {len(e.streams)}, against the null stream")
    return e


# ------------------------------------------------------------------------------------------------ the gated run
class Run:
    """One gated run (module docstring).  stage() / poison() before `with run:`, the call and keep() inside it; leaving the block checks the
    precondition and synchronises.  variant "s": the gate holds `stream`; "null": it holds the null stream and `stream` is idle."""

    def __init__(self, env, variant="s", stream=None, first=False, gate_ms=GATE_MS):
        self.env, self.torch = env, env.torch
        self.s = env.s if stream is None else stream
        self.gated = self.s if variant == "s" else self.torch.cuda.default_stream(DEV)
        self.first, self.gate_ms = first, gate_ms
        self.staged = []

    def stage(self, decoy, real):
        """-> the device buffer the call reads: it holds `decoy` now, `real` arrives on `s` behind the gate"""
        decoy, real = np.ascontiguousarray(decoy), np.ascontiguousarray(real)
        assert decoy.shape == real.shape and decoy.dtype == real.dtype and not np.array_equal(decoy, real)
        d, r = _dev(self.torch, decoy), _dev(self.torch, real)
        self.staged.append((d, r))
        return d

    def poison(self, shape, dtype=None, value=POISON):
        torch = self.torch
        return torch.full(tuple(shape), value, dtype=torch.uint8 if dtype is None else dtype, device=DEV)

    def __enter__(self):
        torch = self.torch
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()
        self.begin, self.end = self.env.gate.hold(self.gated, self.gate_ms)
        self.ctx = torch.cuda.stream(self.s)
        self.ctx.__enter__()
        for d, r in self.staged:
            d.copy_(r, non_blocking=True)
        return self

    def keep(self, t):
        """step 5: a copy of an output, enqueued on `s`"""
        out = self.torch.empty_like(t)
        out.copy_(t, non_blocking=True)
        return out

    def enqueued(self):
        """step 6, for a test that goes on with a blocking call of the library inside the block"""
        self.host_ms = (time.perf_counter() - self.t0) * 1e3
        self.open = not self.end.query()
        assert self.open, f"the gate ({self.gate_ms:.0f} ms) ended before the last launch was enqueued ({self.host_ms:.1f} ms of host time): the run proves nothing"

    def __exit__(self, et, ev, tb):
        self.ctx.__exit__(et, ev, tb)
        try:
            if et is None and not hasattr(self, "open"):
                self.enqueued()
        finally:
            self.torch.cuda.synchronize()
        if et is None:
            ENQUEUE_MS["first" if self.first else "warm"].append(self.host_ms)
            self.gate_measured_ms = self.begin.elapsed_time(self.end)
        return False


# ------------------------------------------------------------------------------------------------ images and yardsticks
_IMAGES, _ORACLE = {}, {}


def image(H, W, seed):
    """smooth (even seeds) and noise (odd seeds) images: cheap and expensive symbols"""
    key = (H, W, seed)
    if key not in _IMAGES:
        _IMAGES[key] = make_image("smooth" if seed % 2 == 0 else "noise", H, W, 4000 + seed)
    return _IMAGES[key]


def batch(H, W, seeds):
    return np.stack([image(H, W, s) for s in seeds])


def _mode(name):
    from llicti_amd.codec import mode_of_name
    return mode_of_name(name)


def oracle_list(W_o, rgb, name):
    """the CPU oracle's bytestream_list of an image in container `name`"""
    from oracle import oracle as orc
    if name == "ac":
        return orc.encode_image(rgb, W_o)
    if name.startswith("xauto"):
        return orc.encode_image_rans(rgb, W_o, int(name[5:]), wide=2, auto=True)
    wide = {"x": 2, "w": 1, "r": 0}[name[0]]
    return orc.encode_image_rans(rgb, W_o, int(name.lstrip("xwrans")), wide=wide)


def oracle_container(wname, W_o, rgb, name):
    """The yardstick of an encode and the input of a decode, computed once: (container bytes, its 49 segment lengths) from the CPU oracle."""
    from llicti_amd.codec import bytestream_list_to_container
    key = (wname, name, rgb.shape, rgb.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = bytestream_list_to_container(oracle_list(W_o, rgb, name))
    return _ORACLE[key]


def containers(c, wname, W_o, rgbs, names):
    """oracle containers of images (one container name, or one per image) as the arrays a decode takes: (uint8 [B, stride], int32 [B, 49])"""
    names = [names] * len(rgbs) if isinstance(names, str) else names
    stride = max(c.max_container_bytes(r.shape[1], r.shape[2]) for r in rgbs)
    cont, seg = np.zeros((len(rgbs), stride), np.uint8), np.zeros((len(rgbs), 49), np.int32)
    for b, (rgb, name) in enumerate(zip(rgbs, names)):
        buf, sl = oracle_container(wname, W_o, rgb, name)
        cont[b, :buf.size], seg[b] = buf, sl
    return cont, seg


def assert_containers(cont, seg, wname, W_o, rgbs, names, what):
    """device outputs of an encode / transcode against the oracle's containers of `rgbs`, to the byte"""
    names = [names] * len(rgbs) if isinstance(names, str) else names
    cont, seg = cont.cpu().numpy(), seg.cpu().numpy()
    for b, (rgb, name) in enumerate(zip(rgbs, names)):
        buf, sl = oracle_container(wname, W_o, rgb, name)
        assert np.array_equal(seg[b], sl), (what, b, "segment lengths", seg[b][:8], sl[:8])
        assert np.array_equal(cont[b, :buf.size], buf), (what, b, "container bytes")


def enc_outputs(run, c, sizes):
    stride = max(c.max_container_bytes(h, w) for h, w in sizes)
    return run.poison((len(sizes), stride)), run.poison((len(sizes), 49), run.torch.int32, -7)


def counters(c, *names):
    return {k: c.counter(k) for k in names}


# ------------------------------------------------------------------------------------------------ negative controls
def _control_encode(env, c, W_o):
    """The gated sequence of an encode with the CALL ISSUED ON THE DEFAULT STREAM while the real input's copy waits behind the gate on `s`
    -> "decoy" (the misplaced call was seen: the container is the decoy's), "real" (it hid: the two streams serialise) or "other"."""
    torch = env.torch
    H, W, name = 64, 96, "xrans2"
    real, decoy = batch(H, W, (10, 11)), batch(H, W, (12, 13))
    run = Run(env)
    x = run.stage(decoy, real)
    out, sl = enc_outputs(run, c, [(H, W)] * 2)
    c.workspace(2, H, W, _mode(name))
    with run:
        with torch.cuda.stream(torch.cuda.default_stream(DEV)):
            c.encode(x, mode=_mode(name), out=out, seg_len=sl)
            got = out.clone(), sl.clone()
    for tag, imgs in (("decoy", decoy), ("real", real)):
        try:
            assert_containers(*got, "trainedlike", W_o, list(imgs), name, tag)
            return tag
        except AssertionError:
            pass
    return "other"


def test_negative_control_encode(env):
    """The gate sees a misplaced launch: an encode issued on the default stream, while its real input waits behind the gate on `s`, codes the decoy."""
    assert env.tried[-1][1] == "decoy", f"no stream of {len(env.streams)} on which an encode on the default stream ran ahead of the gate: {env.tried}"
    assert all(seen in ("decoy", "real") for _, seen in env.tried), env.tried      # a stream that shares the null stream's queue hides the call, no more


def test_negative_control_decode(env, codecs, oracle_weights):
    """... and a decode issued on the default stream gives the decoy's pixels."""
    torch = env.torch
    wname, name, H, W = "trainedlike", "xrans2", 64, 96
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = batch(H, W, (10, 11)), batch(H, W, (12, 13))
    run = Run(env)
    cont = run.stage(containers(c, wname, W_o, list(decoy), name)[0], containers(c, wname, W_o, list(real), name)[0])
    seg = run.stage(containers(c, wname, W_o, list(decoy), name)[1], containers(c, wname, W_o, list(real), name)[1])
    out = run.poison((2, 3, H, W))
    c.workspace(2, H, W, _mode(name))
    c.poison_workspace(POISON)
    with run:
        with torch.cuda.stream(torch.cuda.default_stream(DEV)):
            c.decode(cont, seg, H, W, mode=_mode(name), out=out)
            got = out.clone()
    c.check()
    assert np.array_equal(got.cpu().numpy(), decoy), "a decode on the default stream did not run ahead of the gate on `s`"


# ------------------------------------------------------------------------------------------------ 1. the kernel-level chain
def _ac_encode_async(torch, c, cdf, sym, Lp):
    """HipCodec.ac_encode without its status check (which synchronises)"""
    from llicti_amd import _lib
    from llicti_amd.codec import _ptr, _stream_ptr
    S, N, stride = cdf.shape
    out_stride = (2 * N + 32 + 3) // 4 * 4
    out = torch.zeros((S, out_stride), dtype=torch.uint8, device=DEV)
    ln = torch.zeros((S,), dtype=torch.int32, device=DEV)
    _lib.check(c.L.llicti_ac_encode_u16cdf(c.ctx, _ptr(cdf), int(Lp), stride, _ptr(sym), S, N, _ptr(out), out_stride, _ptr(ln), _stream_ptr(c.device)))
    return out, ln


@pytest.mark.parametrize("wname", ["trainedlike", "rand1337"])
def test_kernel_level_chain_behind_one_gate(env, codecs, oracle_weights, wname):
    """lift -> band_params -> cdf_pairs and cdf_u16 -> ac_encode -> ac_decode -> unlift, and lift_train -> band_params -> selfinfo, B = 2 at
    67x93, levels 0 and 2, every band and colour, each step reading its predecessor's output with no host synchronisation, all behind ONE gate
    on `s`: every intermediate against the oracle (selfinfo: ref64.selfinfo64 and its tolerance), the unlifted decode against the pixels."""
    from llicti_amd._lib import level_geom
    from oracle import oracle as orc
    torch = env.torch
    c, W_o = codecs(wname), oracle_weights(wname)
    B, H, W, LEVELS = 2, 67, 93, (0, 2)
    real, decoy = batch(H, W, (0, 1)), batch(H, W, (2, 3))

    def host_side(rgbs):
        ref = {"lift": [orc.lift(r) for r in rgbs], "ftrain": [orc.lift_train(r) for r in rgbs]}
        for b in range(B):
            p, mm = ref["lift"][b]
            for lvl in LEVELS:
                for band in range(3):
                    par = orc.band_params(p, lvl, band, W_o)
                    ref[("par", b, lvl, band)] = par
                    for clr in range(3):
                        ref[("pairs", b, lvl, band, clr)] = orc.stream_pairs(p, mm, lvl, band, clr, par)
        return ref
    R, D = host_side(real), host_side(decoy)

    def syms(ref, lvl, band, clr):
        return np.stack([ref[("pairs", b, lvl, band, clr)][2] for b in range(B)])

    def minv(ref, b, clr):
        return -127 if clr == 0 else int(ref["lift"][b][1][clr])

    def lp(ref, b, clr):
        return (128 if clr == 0 else int(ref["lift"][b][1][3 + clr])) - minv(ref, b, clr) + 2

    def chain(ref, x, sym_in, minv_d, keep):
        """the two chains on the current stream, on the images `ref` describes (an image's Co / Cg tables have its own number of entries)"""
        K = {}
        planes, fplanes, mm = c.lift(x)
        K["planes"], K["fplanes"], K["mm"] = keep(planes), keep(fplanes), keep(mm)
        dec = planes.clone()                                        # the planes the decoded symbols go back into
        for lvl in LEVELS:
            for band in range(3):
                *_, hc, wc = level_geom(H, W, lvl, band)
                a, bb = ref64.TARGET[band]
                params = c.band_params(fplanes, lvl, band)
                K[("par", lvl, band)] = keep(params)
                K[("pairs", lvl, band)] = keep(c.cdf_pairs(planes, params, mm, lvl, band))
                for clr in range(3):
                    tab = c.cdf_tables(planes, params, mm, lvl, band, clr, row_stride=264 if clr == 0 else 512)
                    K[("tab", lvl, band, clr)] = keep(tab)
                    for b in range(B):
                        out, ln = _ac_encode_async(torch, c, tab[b:b + 1], sym_in[(lvl, band, clr)][b:b + 1], lp(ref, b, clr))
                        K[("bytes", lvl, band, clr, b)], K[("len", lvl, band, clr, b)] = keep(out), keep(ln)
                        got = c.ac_decode(tab[b:b + 1], lp(ref, b, clr), out, ln, hc * wc)
                        K[("sym", lvl, band, clr, b)] = keep(got)
                        dec[b, clr, a << lvl::2 << lvl, bb << lvl::2 << lvl] = got.view(hc, wc) + minv_d[b, clr]
        K["rgb"] = keep(c.unlift(dec))
        ftrain = c.lift_train(x)
        K["ftrain"] = keep(ftrain)
        for lvl in LEVELS:
            for band in range(3):
                pt = c.band_params(ftrain, lvl, band)
                K[("tpar", lvl, band)] = keep(pt)
                K[("bits", lvl, band)] = keep(c.selfinfo(ftrain, pt, lvl, band))
        return K

    stages = [(lvl, band, clr) for lvl in LEVELS for band in range(3) for clr in range(3)]
    minv_of = {id(ref): _dev(torch, np.array([[minv(ref, b, clr) for clr in range(3)] for b in range(B)], np.int16)) for ref in (R, D)}
    # an ungated pass over the DECOY first: the first use of a kernel or a torch operator loads its code (130 ms of host time in a new process),
    # and whatever memory the gated pass is handed back holds the decoy's results, not the real image's
    with torch.cuda.stream(env.s):
        Kw = chain(D, _dev(torch, decoy), {k: _dev(torch, syms(D, *k)) for k in stages}, minv_of[id(D)], lambda t: t.clone())
    torch.cuda.synchronize()
    assert np.array_equal(Kw["rgb"].cpu().numpy(), decoy)
    del Kw
    run = Run(env)
    x = run.stage(decoy, real)
    sym_in = {k: run.stage(syms(D, *k), syms(R, *k)) for k in stages}
    with run:
        K = chain(R, x, sym_in, minv_of[id(R)], run.keep)

    def minv_r(b, clr):
        return minv(R, b, clr)

    def lp_r(b, clr):
        return lp(R, b, clr)
    K = {k: v.cpu() for k, v in K.items()}
    for b in range(B):
        p_ref, mm_ref = R["lift"][b]
        assert np.array_equal(K["planes"][b].numpy(), p_ref), "lift: planes"
        assert np.array_equal(K["mm"][b].numpy(), [mm_ref[1], mm_ref[2], mm_ref[4], mm_ref[5]]), "lift: min / max"
        assert np.array_equal(K["fplanes"][b].numpy(), p_ref.astype(np.float32) / np.float32(255)), "lift: float planes"
        assert np.array_equal(K["ftrain"][b].numpy(), R["ftrain"][b]), "lift_train"
    assert np.array_equal(K["rgb"].numpy(), real), "lift -> ... -> ac_decode -> unlift does not give the pixels back"
    worst = 0.0
    for lvl in LEVELS:
        for band in range(3):
            *_, hc, wc = level_geom(H, W, lvl, band)
            a, bb = ref64.TARGET[band]
            rows_, cols_ = np.arange(a << lvl, H, 2 << lvl), np.arange(bb << lvl, W, 2 << lvl)
            p60 = c.params60(K[("par", lvl, band)]).numpy()
            t60 = c.params60(K[("tpar", lvl, band)]).numpy()
            pairs = K[("pairs", lvl, band)].numpy().view(np.uint32)
            for b in range(B):
                par = R[("par", b, lvl, band)]
                assert np.array_equal(np.ascontiguousarray(p60[b]).view(np.uint32), par.view(np.uint32)), ("band_params", lvl, band, b)
                want_t = orc.band_params_f(R["ftrain"][b], lvl, band, W_o)
                assert np.array_equal(np.ascontiguousarray(t60[b]).view(np.uint32), want_t.view(np.uint32)), ("band_params (training path)", lvl, band, b)
                ref, tol = ref64.selfinfo64(R["ftrain"][b], lvl, band, np.ascontiguousarray(t60[b]))
                q = float((np.abs(K[("bits", lvl, band)][b].numpy() - ref) / tol).max())
                assert q <= 1.0, ("selfinfo", lvl, band, b, q)
                worst = max(worst, q)
                p_ref, mm_ref = R["lift"][b]
                P = par[:hc, :wc].reshape(-1, 60)
                tg = p_ref[:, rows_][:, :, cols_].reshape(3, -1).astype(np.float32) / np.float32(255)
                for clr in range(3):
                    clow, chigh, sym = R[("pairs", b, lvl, band, clr)]
                    assert np.array_equal(pairs[clr, b] & 0xFFFF, clow) and np.array_equal(pairs[clr, b] >> 16, chigh & 0xFFFF), ("cdf_pairs", lvl, band, clr, b)
                    Lp = lp_r(b, clr)
                    tab = K[("tab", lvl, band, clr)][b].numpy().view(np.uint16)
                    assert np.array_equal(tab[:, :Lp], orc.cdf_rows(P, clr, tg[0], tg[1], minv_r(b, clr), minv_r(b, clr) + Lp - 2)), ("cdf_u16", lvl, band, clr, b)
                    assert (tab[:, Lp:] == 0xFFFF).all()
                    n = int(K[("len", lvl, band, clr, b)][0])
                    assert bytes(K[("bytes", lvl, band, clr, b)][0, :n].numpy()) == orc.ac_encode_pairs(clow, chigh), ("ac_encode", lvl, band, clr, b)
                    assert np.array_equal(K[("sym", lvl, band, clr, b)][0].numpy(), sym), ("ac_decode", lvl, band, clr, b)
    print(f"{wname}: largest |selfinfo - float64| / tolerance behind the gate: {worst:.3g}; enqueue {run.host_ms:.1f} ms")


# ------------------------------------------------------------------------------------------------ 2. encodes
ENC_CASES = [("ac", 67, 93, "rand1337"), ("ac", 96, 128, "trainedlike"), ("rans8", 67, 93, "trainedlike"), ("rans8", 96, 128, "rand1337"),
             ("wrans4", 67, 93, "rand1337"), ("wrans4", 96, 128, "trainedlike"), ("xrans2", 67, 93, "trainedlike"), ("xrans2", 96, 128, "rand1337"),
             ("xauto", 67, 93, "rand1337"), ("xauto", 96, 128, "trainedlike")]


def _encode_first_then_warm(env, c, wname, W_o, variant, sizes, names, call, stage_input, what, expect_miss=True):
    """The gated encode twice: the first call of the shape (plan miss: the tables are built and uploaded on `s`), then warm (plan hit), with
    other images.  call(x, out, seg_len); stage_input(run, seeds) -> (the staged input, the real images)."""
    for first in (True, False):
        run = Run(env, variant, first=first)
        x, real = stage_input(run, (4, 5, 6) if first else (6, 7, 4))
        out, sl = enc_outputs(run, c, sizes)
        c.poison_workspace(POISON)
        before = counters(c, "plan_builds", "plan_hits", "device_syncs")
        with run:
            call(x, out, sl)
            got = run.keep(out), run.keep(sl)
        after = counters(c, *before)
        if first and expect_miss:
            assert after["plan_builds"] == before["plan_builds"] + 1, (what, "the first call was to build its plan", before, after)
        if not first:
            assert (after["plan_builds"], after["plan_hits"]) == (before["plan_builds"], before["plan_hits"] + 1), (what, before, after)
        assert after["device_syncs"] == before["device_syncs"], (what, before, after)
        assert_containers(*got, wname, W_o, real, names, (what, variant, "first" if first else "warm"))
    c.check()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,H,W,wname", ENC_CASES)
def test_encode_first_call_and_warm(env, codecs, oracle_weights, name, H, W, wname, variant):
    """llicti_encode_images in every container kind, at an odd and an even shape: the oracle's containers to the byte.  xauto: MODE_RANS_AUTO of
    the size's count (codec.image_streams; both shapes are too small for one xwide stream by that rule, so the count is 1).  The batch holds 2
    images under variant "s" and 3 under "null", so that each variant's first call builds a plan."""
    from llicti_amd.codec import image_streams
    c, W_o = codecs(wname), oracle_weights(wname)
    if name == "xauto":
        name = "xauto%d" % max(1, image_streams(H, W))
    B = 2 if variant == "s" else 3
    c.workspace(B, H, W, _mode(name))

    def stage_input(run, seeds):
        real = batch(H, W, seeds[:B])
        return run.stage(batch(H, W, [s + 20 for s in seeds[:B]]), real), list(real)
    _encode_first_then_warm(env, c, wname, W_o, variant, [(H, W)] * B, name, lambda x, out, sl: c.encode(x, mode=_mode(name), out=out, seg_len=sl),
                            stage_input, name)


@pytest.mark.parametrize("variant", VARIANTS)
def test_encode_mixed_sizes_mode_per_image(env, codecs, oracle_weights, variant):
    """llicti_encode_images_vm: 64x96 with 67x93 (and 96x128 under "null"), a stream count per image."""
    wname = "trainedlike"
    c, W_o = codecs(wname), oracle_weights(wname)
    sizes = [(64, 96), (67, 93), (96, 128)][:2 if variant == "s" else 3]
    names = ["xrans2", "xrans3", "xrans1"][:len(sizes)]
    Hs, Ws, modes = [h for h, _ in sizes], [w for _, w in sizes], [_mode(n) for n in names]
    c.workspace_v(Hs, Ws, modes)

    def stage_input(run, seeds):
        real = [image(h, w, s) for (h, w), s in zip(sizes, seeds)]
        decoy = [image(h, w, s + 20) for (h, w), s in zip(sizes, seeds)]
        return run.stage(np.concatenate([d.reshape(-1) for d in decoy]), np.concatenate([r.reshape(-1) for r in real])), real
    _encode_first_then_warm(env, c, wname, W_o, variant, sizes, names, lambda x, out, sl: c.encode_v(x, Hs, Ws, modes, out=out, seg_len=sl),
                            stage_input, "encode_vm")


@pytest.mark.parametrize("variant", VARIANTS)
def test_encode_px_bgra_crop_at_odd_offset(env, codecs, oracle_weights, variant):
    """llicti_encode_images_px: 67x93 windows of BGRA frames, the first byte of each at an ODD offset (the byte-wise path), the frame's pitch."""
    wname, name = "rand1337", "xrans2"
    c, W_o = codecs(wname), oracle_weights(wname)
    H, W, FH, FW, y0, x0 = 67, 93, 80, 120, 5, 11
    B = 2 if variant == "s" else 3
    frame_bytes = FH * FW * 4 + 4
    px_off = [b * frame_bytes + 1 + (y0 * FW + x0) * 4 for b in range(B)]
    assert all(o % 2 == 1 for o in px_off)

    def frames(imgs, seed):
        buf = np.random.default_rng(seed).integers(0, 256, B * frame_bytes, dtype=np.uint8)
        for b, im in enumerate(imgs):
            fr = buf[b * frame_bytes + 1:b * frame_bytes + 1 + FH * FW * 4].reshape(FH, FW, 4)
            fr[y0:y0 + H, x0:x0 + W, :3] = im[::-1].transpose(1, 2, 0)         # B, G, R; the fourth byte stays random: alpha is not coded
        return buf

    def stage_input(run, seeds):
        real = [image(H, W, s) for s in seeds[:B]]
        return run.stage(frames([image(H, W, s + 20) for s in seeds[:B]], 1), frames(real, 2)), real
    c.workspace_v([H] * B, [W] * B, _mode(name))
    _encode_first_then_warm(env, c, wname, W_o, variant, [(H, W)] * B, name,
                            lambda x, out, sl: c.encode_px(x, [H] * B, [W] * B, _mode(name), "bgra", px_off=px_off, pitch=[FW * 4] * B, out=out, seg_len=sl),
                            stage_input, "encode_px")


@pytest.mark.parametrize("variant", VARIANTS)
def test_encode_f32(env, codecs, oracle_weights, variant):
    """llicti_encode_images_f32 on k / 255: the containers of the uint8 pixels."""
    wname, name, H, W = "trainedlike", "xrans2", 67, 93
    c, W_o = codecs(wname), oracle_weights(wname)
    B = 2 if variant == "s" else 3
    c.workspace_v([H] * B, [W] * B, _mode(name))

    def f32(imgs):
        return (np.stack(imgs).astype(np.float32) / np.float32(255)).reshape(-1)

    def stage_input(run, seeds):
        real = [image(H, W, s) for s in seeds[:B]]
        return run.stage(f32([image(H, W, s + 20) for s in seeds[:B]]), f32(real)), real
    # (the plan is the uint8 call's on the same sizes and mode with this placement: test_encode_first_call_and_warm may have built it)
    _encode_first_then_warm(env, c, wname, W_o, variant, [(H, W)] * B, name,
                            lambda x, out, sl: c.encode_f32(x, [H] * B, [W] * B, _mode(name), out=out, seg_len=sl), stage_input, "encode_f32",
                            expect_miss=False)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["ac", "xrans2"])
def test_encode_side_levels_fork_and_join(env, codecs, oracle_weights, name, variant):
    """enc_side_levels = 1: levels 4..1 fork onto the context's internal stream behind an event recorded on `s` and join back before the coder."""
    wname, H, W = "trainedlike", 96, 128
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = batch(H, W, (8, 9)), batch(H, W, (28, 29))
    run = Run(env, variant)
    x = run.stage(decoy, real)
    out, sl = enc_outputs(run, c, [(H, W)] * 2)
    c.workspace(2, H, W, _mode(name))
    c.poison_workspace(POISON)
    c.set_tuning("enc_side_levels", 1)
    try:
        with run:
            c.encode(x, mode=_mode(name), out=out, seg_len=sl)
            got = run.keep(out), run.keep(sl)
    finally:
        c.set_tuning("enc_side_levels", 0)
    assert_containers(*got, wname, W_o, list(real), name, ("enc_side_levels", name, variant))
    c.check()


# ------------------------------------------------------------------------------------------------ 3. decodes
def _staged_containers(run, c, wname, W_o, real, decoy, names):
    cr, sr = containers(c, wname, W_o, real, names)
    cd, sd = containers(c, wname, W_o, decoy, names)
    return run.stage(cd, cr), run.stage(sd, sr)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("anchors", [False, True])
@pytest.mark.parametrize("B,H,W", [(2, 96, 128), (1, 192, 256)])
def test_decode_reference_format_pipeline(env, codecs, oracle_weights, B, H, W, anchors, variant):
    """The reference-format decoder with 4 and 8 chunks at level 0: every band forks onto the context's two internal streams behind an event
    recorded on `s` and joins back; with full table rows, and over anchor rows (ac_anchor_min_batch = 1)."""
    wname = "trainedlike"
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = [image(H, W, s) for s in range(B)], [image(H, W, 20 + s) for s in range(B)]
    run = Run(env, variant)
    cont, seg = _staged_containers(run, c, wname, W_o, real, decoy, "ac")
    out = run.poison((B, 3, H, W))
    c.workspace(B, H, W, 0)
    c.poison_workspace(POISON)
    c.set_tuning("ac_anchor_min_batch", 1 if anchors else 96)
    try:
        with run:
            c.decode(cont, seg, H, W, mode=0, out=out)
            got = run.keep(out)
    finally:
        c.set_tuning("ac_anchor_min_batch", 96)
    assert np.array_equal(got.cpu().numpy(), np.stack(real))
    c.check()
    assert not c.image_status(B).any()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,wname", [("rans8", "trainedlike"), ("wrans4", "rand1337"), ("xrans10", "trainedlike")])
def test_decode_rans_containers(env, codecs, oracle_weights, name, wname, variant):
    c, W_o = codecs(wname), oracle_weights(wname)
    B, H, W = 2, 67, 93
    real, decoy = [image(H, W, s) for s in (0, 1)], [image(H, W, s) for s in (2, 3)]
    run = Run(env, variant)
    cont, seg = _staged_containers(run, c, wname, W_o, real, decoy, name)
    out = run.poison((B, 3, H, W))
    c.workspace(B, H, W, _mode(name))
    c.poison_workspace(POISON)
    with run:
        c.decode(cont, seg, H, W, mode=_mode(name), out=out)
        got = run.keep(out)
    assert np.array_equal(got.cpu().numpy(), np.stack(real))
    c.check()
    assert not c.image_status(B).any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_decode_mixed_sizes_mode_per_image(env, codecs, oracle_weights, variant):
    """llicti_decode_images_vm"""
    wname = "trainedlike"
    c, W_o = codecs(wname), oracle_weights(wname)
    sizes, names = [(64, 96), (67, 93)], ["xrans2", "xrans3"]
    Hs, Ws, modes = [h for h, _ in sizes], [w for _, w in sizes], [_mode(n) for n in names]
    real = [image(h, w, s) for (h, w), s in zip(sizes, (0, 1))]
    decoy = [image(h, w, s) for (h, w), s in zip(sizes, (2, 3))]
    run = Run(env, variant)
    cont, seg = _staged_containers(run, c, wname, W_o, real, decoy, names)
    out = run.poison((sum(r.size for r in real),))
    c.workspace_v(Hs, Ws, modes)
    c.poison_workspace(POISON)
    with run:
        c.decode_v(cont, seg, Hs, Ws, modes, out=out)
        got = run.keep(out)
    assert np.array_equal(got.cpu().numpy(), np.concatenate([r.reshape(-1) for r in real]))
    c.check()


@pytest.mark.parametrize("variant", VARIANTS)
def test_decode_reduced(env, codecs, oracle_weights, variant):
    """llicti_decode_images_reduced at r = 2: full[:, ::4, ::4] of the original"""
    wname, name, B, H, W, r = "rand1337", "xrans2", 2, 67, 93, 2
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = [image(H, W, s) for s in (0, 1)], [image(H, W, s) for s in (2, 3)]
    run = Run(env, variant)
    cont, seg = _staged_containers(run, c, wname, W_o, real, decoy, name)
    out = run.poison((B, 3, -(-H // 4), -(-W // 4)))
    c.workspace_v([H] * B, [W] * B, _mode(name))
    c.poison_workspace(POISON)
    with run:
        c.decode(cont, seg, H, W, mode=_mode(name), out=out, reduce=r)
        got = run.keep(out)
    assert np.array_equal(got.cpu().numpy(), np.stack(real)[:, :, ::4, ::4])
    c.check()


@pytest.mark.parametrize("variant", VARIANTS)
def test_decode_px_into_poisoned_canvas(env, codecs, oracle_weights, variant):
    """llicti_decode_images_px: RGB windows at an odd offset of a canvas; every byte outside the windows' rows keeps its poison."""
    wname, name, B, H, W = "trainedlike", "xrans2", 2, 67, 93
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = [image(H, W, s) for s in (0, 1)], [image(H, W, s) for s in (2, 3)]
    pitch, span = 3 * W + 7, (H - 1) * (3 * W + 7) + 3 * W
    px_off = [5, 5 + span + 12]
    run = Run(env, variant)
    cont, seg = _staged_containers(run, c, wname, W_o, real, decoy, name)
    canvas = run.poison((px_off[1] + span + 9,))
    c.workspace_v([H] * B, [W] * B, _mode(name))
    c.poison_workspace(POISON)
    with run:
        c.decode_px(cont, seg, [H] * B, [W] * B, _mode(name), "rgb", out=canvas, px_off=px_off, pitch=[pitch] * B)
        got = run.keep(canvas)
    want = np.full(canvas.numel(), POISON, np.uint8)
    for b, im in enumerate(real):
        for i in range(H):
            want[px_off[b] + i * pitch:px_off[b] + i * pitch + 3 * W] = im[:, i].T.reshape(-1)
    assert np.array_equal(got.cpu().numpy(), want)
    c.check()


@pytest.mark.parametrize("variant", VARIANTS)
def test_decode_tensor_f16_crop_flip_normalise(env, codecs, oracle_weights, variant):
    """llicti_decode_images_tensor: float16, a window per image, one mirrored, mean / std -- torch on the CPU on the original pixels, bit for bit."""
    torch = env.torch
    wname, name, B, H, W = "rand1337", "xrans2", 2, 67, 93
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = [image(H, W, s) for s in (0, 1)], [image(H, W, s) for s in (2, 3)]
    Ho, Wo, y0, x0, flip = 33, 50, [3, 34], [43, 0], [0, 1]
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    run = Run(env, variant)
    cont, seg = _staged_containers(run, c, wname, W_o, real, decoy, name)
    out = torch.full((B, 3, Ho, Wo), float("nan"), dtype=torch.float16, device=DEV)
    c.workspace_v([H] * B, [W] * B, _mode(name))
    c.poison_workspace(POISON)
    with run:
        c.decode_tensor(cont, seg, [H] * B, [W] * B, _mode(name), (Ho, Wo), dtype=torch.float16, origin=(y0, x0), flip=flip, mean=mean, std=std, out=out)
        got = run.keep(out)
    wins = [torch.from_numpy(im[:, y0[b]:y0[b] + Ho, x0[b]:x0[b] + Wo].copy()) for b, im in enumerate(real)]
    u8 = torch.stack([torch.flip(w, dims=[-1]) if flip[b] else w for b, w in enumerate(wins)])
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    want = ((u8.float() / 255 - m[:, None, None]) / s[:, None, None]).to(torch.float16)
    assert torch.equal(got.cpu(), want)
    c.check()


class _HipRows(rr.Planes):
    """ref_rans' CDF rows from the kernel-level entry points (as tests/test_hip_ref_rans.py): config B has no encoder in the CPU oracle"""

    def __init__(self, segs, codec, torch):
        super().__init__(segs)
        self.c, self.torch, self._par = codec, torch, (None, None)

    def table(self, lvl, band, clr, R, Cc, minv, maxv):
        torch = self.torch
        if self._par[0] != (lvl, band):
            self._par = ((lvl, band), self.c.band_params(_dev(torch, (self.planes.astype(np.float32) / np.float32(255))[None]), lvl, band))
        mm = _dev(torch, np.array([[self.mm[1], self.mm[2], self.mm[4], self.mm[5]]], np.int32))
        tab = self.c.cdf_tables(_dev(torch, self.planes[None]), self._par[1], mm, lvl, band, clr)[0].cpu().numpy().view(np.uint16)
        return np.ascontiguousarray(tab[:, :maxv - minv + 2])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["ac", "xrans2"])
def test_config_b_encode_and_decode(env, codecs, name, variant):
    """Config B (60-wide heads, 2 levels) at 64x48: the gated encode, then the gated decode of what it wrote.  The CPU oracle has no config-B
    encoder, so the encode's yardsticks are the suite's config-B ones: every stream of the reference format is the oracle's range coder on the
    oracle's pairs (from the kernel-level CNN outputs, made on the default stream after the run), the xwide container is read by ref_rans in
    canonical mode; both must give the original pixels, and so must the gated decode."""
    from llicti_amd.codec import container_to_bytestream_list
    from oracle import oracle as orc
    torch = env.torch
    wname, B, H, W = "b_rand1337", 2, 64, 48
    c = codecs(wname)
    real, decoy = batch(H, W, (0, 1)), batch(H, W, (2, 3))
    run = Run(env, variant)
    x = run.stage(decoy, real)
    out, sl = enc_outputs(run, c, [(H, W)] * B)
    c.workspace(B, H, W, _mode(name))
    c.poison_workspace(POISON)
    with run:
        c.encode(x, mode=_mode(name), out=out, seg_len=sl)
        cont, seg = run.keep(out), run.keep(sl)
    c.check()
    cont_h, seg_h = cont.cpu().numpy(), seg.cpu().numpy()
    for b in range(B):
        bl = container_to_bytestream_list(cont_h[b], seg_h[b])
        assert len(bl) == 3 and (seg_h[b, 22:] == 0).all()
        if name == "ac":
            p_host, mm_ref = orc.lift(real[b])
            assert bl[0][3] == real[b][:, ::4, ::4].tobytes()
            fpl = _dev(torch, (p_host.astype(np.float32) / np.float32(255))[None])
            for si, lvl in enumerate((1, 0)):
                for band in range(3):
                    P3 = c.params60(c.band_params(fpl, lvl, band))[0].cpu().numpy()
                    for clr in range(3):
                        clow, chigh, _ = orc.stream_pairs(p_host, mm_ref, lvl, band, clr, P3)
                        assert bl[1 + si][3 * band + clr] == orc.ac_encode_pairs(clow, chigh), (b, lvl, band, clr)
        else:
            segs = rr.segments(bl)
            planes, info = rr.decode_image(segs, _HipRows(segs, c, torch), canonical=True)
            assert info["header"]["nlevels"] == 2 and info["header"]["M"] == 2
            assert np.array_equal(orc.unlift(planes), real[b]), b
    # the decode: the containers just checked are the real input, those of the decoy images (an ungated encode) the decoy
    dcont, dseg = c.encode(_dev(torch, decoy), mode=_mode(name))
    c.check()
    run = Run(env, variant)
    cin, sin = run.stage(dcont.cpu().numpy(), cont_h), run.stage(dseg.cpu().numpy(), seg_h)
    rec = run.poison((B, 3, H, W))
    c.poison_workspace(POISON)
    with run:
        c.decode(cin, sin, H, W, mode=_mode(name), out=rec)
        got = run.keep(rec)
    assert np.array_equal(got.cpu().numpy(), real)
    c.check()


# ------------------------------------------------------------------------------------------------ 4. transcodes
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("src,dst", [("ac", "xrans2"), ("xrans2", "ac")])
def test_transcode(env, codecs, oracle_weights, src, dst, variant):
    """llicti_transcode_images, B = 2 at 96x128: the oracle's container of the ORIGINAL image in the target mode.  (The reference format as the
    source runs the decoder's three-queue pipeline with the pairs kernel of the target behind every band's join.)"""
    wname, B, H, W = "trainedlike", 2, 96, 128
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = [image(H, W, s) for s in (0, 1)], [image(H, W, s) for s in (20, 21)]
    run = Run(env, variant)
    cont, seg = _staged_containers(run, c, wname, W_o, real, decoy, src)
    out, sl = enc_outputs(run, c, [(H, W)] * B)
    c.transcode_workspace([H] * B, [W] * B, _mode(src), _mode(dst))
    c.poison_workspace(POISON)
    with run:
        c.transcode(cont, seg, [H] * B, [W] * B, _mode(src), _mode(dst), out=out, seg_len_out=sl)
        got = run.keep(out), run.keep(sl)
    assert_containers(*got, wname, W_o, real, dst, ("transcode", src, dst, variant))
    c.check()
    assert not c.image_status(B).any()


# ------------------------------------------------------------------------------------------------ 5. status calls and timing
def test_status_calls_synchronise_the_stream_they_are_given(env, codecs, oracle_weights):
    """A batch of three with image 0's header damaged (h4 ^ 1: the corruption of test_malformed_header_is_deterministic_and_per_image, flagged by
    the header kernel, never a fault) decoded on gated `s`, with no torch synchronisation: llicti_check_status(ctx, s) must wait for `s` -- the
    gate, the copy of the containers, the decode -- and return LLICTI_EFORMAT, llicti_image_status(ctx, .., s) the words bad, good, good.  A
    call that synchronised another stream would read the zeros of a decode that has not run."""
    from llicti_amd._lib import EFORMAT
    from llicti_amd.codec import _ptr
    wname, name, B, H, W = "trainedlike", "xrans2", 3, 64, 96
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = [image(H, W, s) for s in (0, 1, 2)], [image(H, W, s) for s in (20, 21, 22)]
    for mode_name in ("ac", name):
        cr, sr = containers(c, wname, W_o, real, mode_name)
        cr = cr.copy()
        cr[0, 1] ^= 0x01                                             # h4 of image 0
        cd, sd = containers(c, wname, W_o, decoy, mode_name)
        run = Run(env)
        cont, seg = run.stage(cd, cr), run.stage(sd, sr)
        out = run.poison((B, 3, H, W))
        c.workspace(B, H, W, _mode(mode_name))
        c.poison_workspace(POISON)
        sp = C.c_void_p(env.s.cuda_stream)
        st = np.full(B, 77, np.int32)
        with run:
            c.decode(cont, seg, H, W, mode=_mode(mode_name), out=out)
            got = run.keep(out)
            run.enqueued()
            rc = c.L.llicti_check_status(c.ctx, sp)
            done_after_check = got.clone()                           # (on `s`, which the library has just synchronised)
            rc_img = c.L.llicti_image_status(c.ctx, _ptr(st), B, sp)
        assert rc == EFORMAT, (mode_name, rc)
        assert rc_img == 0 and list(st) == [EFORMAT, 0, 0], (mode_name, rc_img, st)
        rec = done_after_check.cpu().numpy()
        assert np.array_equal(rec[1], real[1]) and np.array_equal(rec[2], real[2]), mode_name
        assert c.L.llicti_check_status(c.ctx, sp) == 0               # (the latched word was cleared by the first check)


def test_status_calls_touch_no_other_stream(env, codecs, oracle_weights):
    """... and ONLY that stream.  The mirrored run: the null stream is held by the gate, the same damaged batch is decoded on an idle `s`, and
    llicti_check_status(ctx, s) / llicti_image_status(ctx, .., s) return their results while the gate on the null stream is STILL running.  A
    status call that reads or clears its words with a synchronous copy on the null stream waits for whatever the caller has in flight there --
    a training step on the default stream, for a caller that keeps the codec on a side stream.  (The decode takes about a millisecond, the gate
    GATE_MS.)"""
    from llicti_amd._lib import EFORMAT
    from llicti_amd.codec import _ptr
    wname, name, B, H, W = "trainedlike", "xrans2", 3, 64, 96
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = [image(H, W, s) for s in (0, 1, 2)], [image(H, W, s) for s in (20, 21, 22)]
    cr, sr = containers(c, wname, W_o, real, name)
    cr = cr.copy()
    cr[0, 1] ^= 0x01                                                 # h4 of image 0
    cd, sd = containers(c, wname, W_o, decoy, name)
    run = Run(env, "null")
    cont, seg = run.stage(cd, cr), run.stage(sd, sr)
    out = run.poison((B, 3, H, W))
    c.workspace(B, H, W, _mode(name))
    c.poison_workspace(POISON)
    sp = C.c_void_p(env.s.cuda_stream)
    st = np.full(B, 77, np.int32)
    with run:
        c.decode(cont, seg, H, W, mode=_mode(name), out=out)
        got = run.keep(out)
        run.enqueued()
        rc = c.L.llicti_check_status(c.ctx, sp)
        open_after_check = not run.end.query()
        rc_img = c.L.llicti_image_status(c.ctx, _ptr(st), B, sp)
        open_after_image = not run.end.query()
        rc_again = c.L.llicti_check_status(c.ctx, sp)
    assert rc == EFORMAT and rc_img == 0 and list(st) == [EFORMAT, 0, 0] and rc_again == 0, (rc, rc_img, st, rc_again)
    assert open_after_check, "llicti_check_status(ctx, s) waited for the null stream"
    assert open_after_image, "llicti_image_status(ctx, .., s) waited for the null stream"
    rec = got.cpu().numpy()
    assert np.array_equal(rec[1], real[1]) and np.array_equal(rec[2], real[2])


def test_last_timing_extent_lies_behind_the_gate(env, codecs, oracle_weights):
    """Profiling on: the extent of a gated call on `s` is recorded on `s`, behind the gate -- llicti_last_timing succeeds, ms[0] is positive and
    smaller than the gate as the gate's own events measure it."""
    wname, name, B, H, W = "trainedlike", "xrans2", 2, 67, 93
    c, W_o = codecs(wname), oracle_weights(wname)
    real, decoy = batch(H, W, (0, 1)), batch(H, W, (2, 3))
    c.workspace(B, H, W, _mode(name))
    c.set_profiling(True)
    try:
        run = Run(env)
        x = run.stage(decoy, real)
        out, sl = enc_outputs(run, c, [(H, W)] * B)
        with run:
            c.encode(x, mode=_mode(name), out=out, seg_len=sl)
            got = run.keep(out), run.keep(sl)
            run.enqueued()
            ms, n_launch = c.last_timing()                           # (waits for the call's closing event, on `s`)
    finally:
        c.set_profiling(False)
    assert_containers(*got, wname, W_o, list(real), name, "profiled encode")
    assert n_launch >= 15 and 0.0 < ms[0] < run.gate_measured_ms, (ms, n_launch, run.gate_measured_ms)
    assert run.gate_measured_ms > 0.8 * GATE_MS, run.gate_measured_ms


# ------------------------------------------------------------------------------------------------ 6. one context, streams in turn
def test_one_context_streams_in_turn_and_block_pool(env, oracle_weights):
    """Calls of one context on different streams, ordered by the caller (B.wait_stream(A) ...), on a context of its own (module docstring).
    (a) call 1 of a new shape on gated A, call 2 of the shape on B (a plan hit on another stream: get_plan waits for the upload and for the
    last use), call 3 back on A: three right containers, no device synchronisation or allocation after the first call, two plan hits.
    (b) the cache is full (32 plans) and the pool empty; behind the gate on A every cached plan is used, oldest first, then two new plans are
    requested on B.  The first takes a new block (the pool is empty) and evicts the oldest plan, whose last user is still gated: its block goes
    to the pool BUSY.  acquire_block's rule for the second: a block whose `done` event has not fired is not reused, and with fewer than 16 blocks
    pooled it does not wait either -- one more allocation, no block wait, two blocks pooled.  Once the streams are idle a third new plan
    REUSES a pooled block: no allocation."""
    from llicti_amd.codec import MODE_RANS
    torch = env.torch
    wname = "trainedlike"
    W_o = oracle_weights(wname)
    A, Bs = env.s, env.s2
    c = new_codec(torch, wname)
    try:
        # (a)
        H, W, name = 72, 104, "xrans2"
        imgs = [image(H, W, s)[None] for s in (0, 1, 2)]
        run = Run(env, first=True)
        xs = [run.stage(image(H, W, 20 + k)[None], imgs[k]) for k in range(3)]
        outs = [enc_outputs(run, c, [(H, W)]) for _ in range(3)]
        c.workspace(1, H, W, _mode(name))
        c.poison_workspace(POISON)
        base = counters(c, "plan_builds", "plan_hits")
        with run:
            c.encode(xs[0], mode=_mode(name), out=outs[0][0], seg_len=outs[0][1])
            after1 = counters(c, "device_syncs", "device_allocs")
            Bs.wait_stream(A)
            with torch.cuda.stream(Bs):
                c.encode(xs[1], mode=_mode(name), out=outs[1][0], seg_len=outs[1][1])
            A.wait_stream(Bs)
            c.encode(xs[2], mode=_mode(name), out=outs[2][0], seg_len=outs[2][1])
            got = [(run.keep(o), run.keep(s)) for o, s in outs]
        assert counters(c, "device_syncs", "device_allocs") == after1
        assert counters(c, "plan_builds", "plan_hits") == {"plan_builds": base["plan_builds"] + 1, "plan_hits": base["plan_hits"] + 2}
        for k in range(3):
            assert_containers(*got[k], wname, W_o, list(imgs[k]), name, ("streams in turn, call", k + 1))
        c.check()

        # (b) fill the cache: 32 plans, every block held by a cached plan, none pooled
        mode = MODE_RANS(2)
        shapes = [(32 + 8 * i, 40 + 4 * i) for i in range(35)]
        warm = _dev(torch, make_image("noise", 32, 32, 1)[None])    # new_codec's own warm-up calls, whose plan(s) the cache still holds
        wcont, wseg = c.encode(warm)
        c.check()
        n_fill = 32 - c.counter("plans_cached")
        fill, (new1, new2, new3) = shapes[:n_fill], shapes[n_fill:n_fill + 3]
        dev_imgs = {hw: _dev(torch, image(*hw, 1)[None]) for hw in shapes[:n_fill + 3]}
        for hw in fill:
            c.encode(dev_imgs[hw], mode=mode)
        c.check()
        assert c.counter("plans_cached") == 32 and c.counter("blocks_pooled") == 0
        h0, w0 = fill[0]
        run = Run(env, first=True)
        x_old = run.stage(image(h0, w0, 3)[None], image(h0, w0, 1)[None])
        x_new = [run.stage(image(*hw, 3)[None], image(*hw, 1)[None]) for hw in (new1, new2)]
        o_old = enc_outputs(run, c, [(h0, w0)])
        o_new = [enc_outputs(run, c, [hw]) for hw in (new1, new2)]
        c.workspace(1, *new3, mode)
        c.poison_workspace(POISON)
        before = counters(c, "device_allocs", "block_waits", "device_syncs", "plan_builds")
        with run:
            c.encode(x_old, mode=mode, out=o_old[0], seg_len=o_old[1])      # used first: the least recently used plan once all have been used
            c.encode(warm)
            c.decode(wcont, wseg, 32, 32)
            c.encode(xs[0], mode=_mode(name))
            for hw in fill[1:]:
                c.encode(dev_imgs[hw], mode=mode)
            all_hits = counters(c, "plan_builds")["plan_builds"] == before["plan_builds"]
            Bs.wait_stream(A)
            with torch.cuda.stream(Bs):
                for k in range(2):
                    c.encode(x_new[k], mode=mode, out=o_new[k][0], seg_len=o_new[k][1])
            A.wait_stream(Bs)
            got_old = run.keep(o_old[0]), run.keep(o_old[1])
            got_new = [(run.keep(o), run.keep(s)) for o, s in o_new]
        after = counters(c, *before)
        assert all_hits and after["plan_builds"] == before["plan_builds"] + 2, (before, after)
        assert after["device_allocs"] == before["device_allocs"] + 2, ("a block whose last user had not finished was reused", before, after)
        assert after["block_waits"] == before["block_waits"] and after["device_syncs"] == before["device_syncs"], (before, after)
        assert c.counter("plans_cached") == 32 and c.counter("blocks_pooled") == 2
        assert_containers(*got_old, wname, W_o, [image(h0, w0, 1)], "rans2", "the evicted plan's last user")
        for k, hw in enumerate((new1, new2)):
            assert_containers(*got_new[k], wname, W_o, [image(*hw, 1)], "rans2", ("new plan", k))
        c.check()
        cont, seg = c.encode(dev_imgs[new3], mode=mode)             # idle streams: the pooled blocks' events have fired
        c.check()
        assert c.counter("device_allocs") == after["device_allocs"] and c.counter("blocks_pooled") == 2
        assert_containers(cont, seg, wname, W_o, [image(*new3, 1)], "rans2", "a plan on a reused block")
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 7. the model layer
def test_model_layer_batches_in_flight_on_a_gated_stream(env):
    """LLICTI_nets.py under `with torch.cuda.stream(s)`, `s` gated: its upload and download streams order themselves against the CURRENT stream
    (wait_stream / record_stream) and recycle pinned staging buffers per slot.  Two encode_batch_async calls in flight (slot 0: a list of host
    arrays of mixed sizes, slot 1: a host tensor), then two decode_batch_async calls, all enqueued while the gate holds `s`: lists() are the
    oracle's bytestream lists, the decodes the original pixels.  transcode_batch (synchronous by design) follows behind them on `s`, and
    codec().check() is clean.  The model's context, copy streams and staging buffers are made by an ungated pass over other images of the same
    sizes first: creating a context and loading weights synchronise the device."""
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.weights import pack_state_dict
    from oracle import oracle as orc
    torch = env.torch
    dev = torch.device(DEV)
    torch.manual_seed(1337)
    model = LLICTI(default_config(container="xrans2")).to(DEV).eval()
    W_o = orc.Weights(pack_state_dict(model.state_dict()))
    sizes = [(64, 96), (67, 93), (96, 128)]
    mixed = [image(h, w, k) for k, (h, w) in enumerate(sizes)]
    same = batch(67, 93, (4, 5))
    want_mixed = [oracle_list(W_o, im, "xrans2") for im in mixed]
    want_same = [oracle_list(W_o, im, "xrans2") for im in same]
    try:
        with torch.cuda.stream(env.s):
            w0 = model.encode_batch_async([image(h, w, 20 + k) for k, (h, w) in enumerate(sizes)], slot=0).lists()
            w1 = model.encode_batch_async(torch.from_numpy(batch(67, 93, (24, 25))), slot=1).lists()
            model.decode_batch_async(w0, dev, slot=0)
            model.decode_batch_async(w1, dev, slot=1)
            model.transcode_batch(w1, container="ac")
            model.codec().check()
        run = Run(env)
        with run:
            e0 = model.encode_batch_async(mixed, slot=0)
            e1 = model.encode_batch_async(torch.from_numpy(same), slot=1)
            flat, Hs, Ws = model.decode_batch_async(want_mixed, dev, slot=0)
            rec = model.decode_batch_async(want_same, dev, slot=1)
            got_flat, got_rec = run.keep(flat), run.keep(rec)
            run.enqueued()
            l0, l1 = e0.lists(), e1.lists()                          # (each waits for its own download, behind the gate)
            ac = model.transcode_batch(want_same, container="ac")
            model.codec().check()
        assert l0 == want_mixed and l1 == want_same
        assert (list(Hs), list(Ws)) == ([h for h, _ in sizes], [w for _, w in sizes])
        assert np.array_equal(got_flat.cpu().numpy(), np.concatenate([im.reshape(-1) for im in mixed]))
        assert np.array_equal(got_rec.cpu().numpy(), same)
        assert ac == [orc.encode_image(im, W_o) for im in same]
    finally:
        torch.cuda.synchronize()
        if model._codec is not None:
            model._codec.close()
