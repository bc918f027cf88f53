"""Census of the rANS tail coders' paths, computed from the INPUTS (numpy, the CPU oracle and tests/ref_rans.py only; shared by
tests/test_tail_census_cpu.py, which asserts minimum counts, and tests/test_hip_tail_edges.py, which runs exactly INPUTS on the device).

The tail (llicti_amd/csrc/rans_tail.hpp, the encoder's side in rans_encode.hpp, the shape both share in host_types.hpp) is the most
branchy code of the coder.  census(bl, weights) runs the oracle's container `bl` through the second reader (ref_rans.decode, canonical=True,
its on_tail hook) and returns two counters: which STREAM classes the container's streams hold and which SYMBOL classes -- paths of the
decoder's coder in tail_decode_rounds -- its coded tail symbols take.  Nothing here imports the library's code or the oracle's rANS entry
points; seeded_tail_shape is restated below (tail_shape) and held against the reader's facts.

Stream classes (stream_classes; `cnt` the stream's symbols of the last stage, T its tail symbols, E the spill, n the seeds per chain)
  kind:N / kind:W / kind:X1 / kind:X2     64 lanes, 128 lanes, xwide with one chain, xwide with two
  cnt=0                                   no symbol of the last stage (M larger than the stage's chunk count)
  T=cnt, T<cnt, T=cap:NW, T=cap:X         the whole share in the tail; a main part in front; T at 2,047 / 8,160
  ncod=0                                  T >= 1 and no coded symbol: X1 with T = 1, X2 with T = 2 n
  one_round                               0 < chain_count(0) <= SA (SA = 4; 8 on X1, whose idle chain's preparing wavefronts are pooled)
  NW:T%4=r                                r = 0 .. 3, T >= 1
  X2:A%4=r, X2:B%4=r, X2:ncod odd / even  the chains' coded counts (> 0) modulo the round; chain A one ahead or level
  X1:ncod%8=r                             r = 0 .. 7, ncod >= 1
  X1:E=0, X1:E=1..31, X1:E>=32, X2:...    the spill; X2:E=1..31 is chain B's final state across the payload / spill boundary
  X2:gap>0, X2:gap=0                      zero bits left between the chains or none
  chunk_jump                              M > 1 and the tail reaches back over a chunk boundary of its stream (positions jump by L M)
  partial_chunk                           cnt % L != 0 and T >= 1: the partial last chunk lies inside the tail
  X2:n=3, X2:n=31, X2:n odd, X2:n even    seeds per chain (odd / even: 3 < n < 31);  A=1: a one-symbol alphabet (flat, grey)

Symbol classes (one coded tail symbol each; classify)
  none            no window offered                      hit    the slot proves inside the offered window (1 <= np <= 11)
  miss            offered, then the bucket search
  d=0, d=10       hit at the first / last provable entry (d = symbol - wbs)
  d=-1, d=11      the first misses on either side
  wbs=0           an offered window at entry 0, the floor of the search, "counted whatever it holds"
  clip_top        wbs + 11 > max_symbol: the window's entries past the top symbol are 2^16
  bucket_clipped  the bucket search behind a miss or behind `none` has wb == 0
  search13        the bucket's 12 entries do not bracket the slot (np == 0 or 12): the exact 13-ary search
  ambiguous       the class depends on an anchor value inside the bound below
No class has left the required set (test_tail_census_cpu.REQUIRED_*) except search13, see SEARCH13 below.

The anchors and their bound.  The window and the bucket come from the APPROXIMATE table entries e1 at the 64 anchors i1 = min(8 l,
max_symbol): term_fast's formula (Abramowitz-Stegun 7.1.26 with the folded constants c1 = fl(K rsig), c0 = fl(-mu c1), both formed here in
fp32 exactly as comp_fast forms them) evaluated in float64, e1 = rint(sum * scale) + i1.  The device evaluates the same formula in fp32 with
v_rcp_f32 / v_exp_f32 (1 ulp each).  Per component k, with a = |x|:
  x = fma(pt, c1, c0): c0's rounding is |mu c1| 2^-24, the fma's |x| 2^-24; both are covered by dx = |c1| (|pt| + |mu|) 2^-23 -- NOT a
      fixed number of counts: at the sigma floor |c1| = 1,968 and dx = 4.7e-4 for |pt| + |mu| = 2, which the term's slope turns into up
      to 14 counts.  |d term / d x| = wh * 2 / (sqrt(pi) * 1.2011) * exp2(-x^2) <= 0.94 wh exp2(-max(a - dx, 0)^2).
  E = p(u) u exp2(-a^2) wh: u = rcp(1 + q a) (1 ulp + the fma), four fma of the polynomial, three multiplies, exp2 (1 ulp) of an argument a^2
      rounded to 2^-24 relative, i.e. ln 2 * a^2 * 2^-24 relative on E: together below (16 + a^2) 2^-23 relative.
  wn - E: wn 2^-24.   The five terms' sum (<= 1): 4 additions, 2^-22 together.   sum * scale (< 2^16): 2^-8 counts.
  bound = scale * (sum_k [0.94 wh_k exp2(-max(a_k - dx_k, 0)^2) dx_k + E_k (16 + a_k^2) 2^-23 + wn_k 2^-24] + 2^-22) + 2^-8   counts,
and the device's e1 lies in [rint(v - bound), rint(v + bound)].  The window's refinement fr = 8 (0x8000 - eL) rcp(eH - eL) (ints below
2^24 are exact in fp32; rcp and two multiplies: 2^-21 relative) is taken at both ends of that too.  A symbol gets a class only if every
combination of anchor values inside the bound gives the same set of classes; census(..., bound_scale=2) doubles the bound.
"""
import os
from collections import Counter

import numpy as np

import ref_rans as rr
from helpers import bw_image, flat_image, make_image, two_valued_image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_f = np.float32
SA_OF = {"N": 4, "W": 4, "X2": 4, "X1": 8}          # symbols of a chain per round (kTailAhead; pooled on X1)
SYMBOL_CLASSES = ("none", "hit", "miss", "d=0", "d=10", "d=-1", "d=11", "wbs=0", "clip_top", "bucket_clipped", "search13", "ambiguous")
EDGE_D = {0: "d=0", 10: "d=10", -1: "d=-1", 11: "d=11"}


# ------------------------------------------------------------------------------------------------------------- stream classes
def tail_shape(cnt, tall, nch, ns, seeded=True):
    """host_types.hpp's seeded_tail_shape, restated: -> (sn raw symbols per start state, NS seed symbols, ncod coded symbols)"""
    sn = 0 if not seeded else ns if nch == 2 else 1
    NS = min(nch * sn, cnt)
    return sn, NS, max(tall - NS, 0)


def chain_count(ncod, nch, c):
    return (ncod + nch - 1 - c) // nch


def stream_kind(hdr, facts):
    if hdr["L"] != 256:
        return "N" if hdr["L"] == 64 else "W"
    return "X1" if facts["one_chain"] else "X2"


def stream_classes(hdr, facts, m):
    """The classes of stream m (facts: ref_rans' per-stream dict after a canonical decode) -> (set of class names, the restated shape)"""
    L, M = hdr["L"], hdr["M"]
    kind = stream_kind(hdr, facts)
    cnt, T = facts["share"], facts["T"]
    out = set()
    if cnt == 0:
        return {"cnt=0"}, (kind, 0, 0, 0)
    out.add("kind:" + kind)
    X = kind[0] == "X"
    nch = 2 if kind == "X2" else 1
    ns = facts["n_seed"] if X else 0
    sn, NS, ncod = tail_shape(cnt, T, nch, ns, X)
    out.add("T=cnt" if T == cnt else "T<cnt")
    if T == (rr.V4_TAIL_MAX if X else rr.V3_TAIL_MAX):
        out.add("T=cap:X" if X else "T=cap:NW")
    if T >= 1 and ncod == 0:
        out.add("ncod=0")
    cA, cB = chain_count(ncod, nch, 0), (chain_count(ncod, nch, 1) if nch == 2 else 0)
    if 0 < cA <= SA_OF[kind]:
        out.add("one_round")
    if not X and T >= 1:
        out.add("NW:T%%4=%d" % (T % 4))
    if kind == "X1" and ncod >= 1:
        out.add("X1:ncod%%8=%d" % (ncod % 8))
    if kind == "X2":
        if cA:
            out.add("X2:A%%4=%d" % (cA % 4))
        if cB:
            out.add("X2:B%%4=%d" % (cB % 4))
        if ncod:
            out.add("X2:ncod odd" if ncod & 1 else "X2:ncod even")
        out.add("X2:gap>0" if facts["gap"] > 0 else "X2:gap=0")
        out.add("X2:n=3" if ns == 3 else "X2:n=31" if ns == 31 else "X2:n odd" if ns & 1 else "X2:n even")
    if X:
        E = facts["spill"]
        out.add(kind + (":E=0" if E == 0 else ":E=1..31" if E < 32 else ":E>=32"))
        if facts["A"] == 1:
            out.add("A=1")
    last = cnt % L or L                                   # symbols of the stream's last chunk
    if M > 1 and T > last:
        out.add("chunk_jump")
    if cnt % L and T >= 1:
        out.add("partial_chunk")
    return out, (kind, sn, NS, ncod)


def all_stream_classes():
    out = ["kind:N", "kind:W", "kind:X1", "kind:X2", "cnt=0", "T=cnt", "T<cnt", "T=cap:NW", "T=cap:X", "ncod=0", "one_round"]
    out += ["NW:T%%4=%d" % r for r in range(4)] + ["X2:A%%4=%d" % r for r in range(4)] + ["X2:B%%4=%d" % r for r in range(4)]
    out += ["X2:ncod odd", "X2:ncod even"] + ["X1:ncod%%8=%d" % r for r in range(8)]
    out += [k + e for k in ("X1", "X2") for e in (":E=0", ":E=1..31", ":E>=32")]
    out += ["X2:gap>0", "X2:gap=0", "chunk_jump", "partial_chunk", "X2:n=3", "X2:n=31", "X2:n odd", "X2:n even", "A=1"]
    return out


# ------------------------------------------------------------------------------------------------------------- symbol classes
_K1 = _f(_f(-0.70710678118654752440) * _f(1.2011224087864498))           # comp_fast's folded constant, as the compiler folds it (fp32)
_Q = float(_f(_f(0.3275911) / _f(1.2011224087864498)))
_P = [float(_f(v)) for v in (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)]
_SCALE_BOUND = _f(0.11 / 255.0)
_WEIGHT_BOUND = _f(1e-6)


def components(par60, yv, cov):
    """The Cg channel's five prepared components of n positions (par60 [n, 60]: the CNN's outputs; yv, cov fp32 [n]): mix_component<2> and
    mix_weight_den in fp32, operation for operation (numerics spec) -> (mu, rsig, wn), fp32 [n, 5] each"""
    par60 = np.asarray(par60, np.float32)
    y, co = np.asarray(yv, np.float32)[:, None], np.asarray(cov, np.float32)[:, None]
    sg, mu0, wk = par60[:, 10:15], par60[:, 25:30], par60[:, 40:45]
    bb, dd = par60[:, 50:55], par60[:, 55:60]
    mu = mu0 + (bb * y + dd * co)
    rsig = _f(1) / np.where(sg > _SCALE_BOUND, sg, _SCALE_BOUND)
    w = np.where(wk > _WEIGHT_BOUND, wk, _WEIGHT_BOUND)
    den = _f(1e-9) + ((((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]) + w[:, 4])
    return mu.astype(np.float32), rsig.astype(np.float32), (w / den[:, None]).astype(np.float32)


def anchors(mu, rsig, wn, minv, maxv, bound_scale=1.0):
    """-> (v float64 [n, 64]: sum * scale at the anchors; bound float64 [n, 64] in counts; i1 int [64]) -- module docstring"""
    Lp = maxv - minv + 2
    max_symbol = Lp - 2
    scale = float(_f(65536 - (Lp - 1)))
    i1 = np.minimum(8 * np.arange(64), max_symbol)
    pt = (_f(minv) - _f(0.5) + i1.astype(np.float32)) / _f(255)                     # div255_exact is the fp32 division, bit for bit
    pt = np.where(i1 == 0, _f((minv - 0.5 - 20.0) / 255.0), pt).astype(np.float64)   # sample_pt(gr, 0) = p_first
    c1 = (_K1 * rsig).astype(np.float32)
    c0 = (-mu * c1).astype(np.float32)
    c1d, c0d, wnd, mud = c1.astype(np.float64)[:, None, :], c0.astype(np.float64)[:, None, :], wn.astype(np.float64)[:, None, :], mu.astype(np.float64)[:, None, :]
    whd = 0.5 * wnd
    x = pt[None, :, None] * c1d + c0d
    a = np.abs(x)
    u = 1.0 / (1.0 + _Q * a)
    p = _P[0] * u + _P[1]
    for cf in _P[2:]:
        p = p * u + cf
    E = p * u * np.exp2(-(a * a)) * whd
    term = np.where(x < 0, wnd - E, E)
    v = term.sum(axis=2) * scale
    dx = np.abs(c1d) * (np.abs(pt)[None, :, None] + np.abs(mud)) * 2.0 ** -23
    per = 0.94 * whd * np.exp2(-np.maximum(a - dx, 0.0) ** 2) * dx + E * (16.0 + a * a) * 2.0 ** -23 + wnd * 2.0 ** -24
    bound = scale * (per.sum(axis=2) + 2.0 ** -22) + 2.0 ** -8
    return v, bound * bound_scale, i1


def _tags(row, slot, symbol, max_symbol, wbs, wb):
    """The classes of one symbol on one outcome of the preparing wavefront (wbs: the offered window's first index, None: no window) and of
    the anchors' bucket (wb), tail_decode_rounds read literally against the exact row"""
    tags = set()
    if wbs is not None:
        npop = sum(1 for k in range(12) if wbs + k <= max_symbol and row[wbs + k] <= slot)
        if wbs == 0 and not (row[0] <= slot):
            npop += 1                                      # entry 0 is counted whatever it holds
        if wbs == 0:
            tags.add("wbs=0")
        if wbs + 11 > max_symbol:
            tags.add("clip_top")
        d = symbol - wbs
        if d in EDGE_D:
            tags.add(EDGE_D[d])
        if 1 <= npop <= 11:
            assert wbs + npop - 1 == symbol, "the window proves another symbol than the exact search"
            tags.add("hit")
            return frozenset(tags)
        tags.add("miss")
    else:
        tags.add("none")
    npop = sum(1 for k in range(12) if wb + k <= max_symbol and (row[wb + k] <= slot or wb + k == 0))
    if wb == 0:
        tags.add("bucket_clipped")
    if npop == 0 or npop == 12:
        tags.add("search13")
    else:
        assert wb + npop - 1 == symbol, "the bucket proves another symbol than the exact search"
    return frozenset(tags)


def _rint_range(v, b):
    return int(np.rint(v - b)), int(np.rint(v + b))


def classify(row, slot, symbol, v, bound, i1, max_symbol):
    """One coded tail symbol -> frozenset of SYMBOL_CLASSES (the single class "ambiguous" if the anchors' bound leaves more than one answer).
    v, bound: the symbol's 64 anchors (anchors()).  tail_prepare_role's window rule and tail_decode_rounds' bucket rule, restated."""
    lo = np.rint(v - bound).astype(np.int64) + i1
    hi = np.rint(v + bound).astype(np.int64) + i1
    valid = 8 * np.arange(64) <= max_symbol
    valid[0] = True
    # the window: lst = the last anchor at or below 2^15 (a count, as the ballot's), eL / eH the entries around the crossing
    sure = int((valid[1:] & (hi[1:] <= 0x8000)).sum()) + 1
    maybe = int((valid[1:] & (lo[1:] <= 0x8000) & (hi[1:] > 0x8000)).sum())
    wins = set()
    for lst in range(sure - 1, sure + maybe):
        top = lst < 63 and 8 * (lst + 1) <= max_symbol
        eHr = (int(lo[lst + 1]), int(hi[lst + 1])) if top else (0x10000, 0x10000)
        eLr = (int(lo[lst]), int(hi[lst]))
        if eHr[0] - eLr[1] < 0x2000:
            wins.add(None)
            if eHr[1] - eLr[0] < 0x2000:
                continue
        ws = []
        for eL in eLr:
            for eH in eHr:
                if eH - eL >= 0x2000:
                    for rel in (1 - 2.0 ** -21, 1 + 2.0 ** -21):
                        fr = 8.0 * (0x8000 - eL) / (eH - eL) * rel
                        ws.append(max(8 * lst + int(min(max(fr, 0.0), 8.0)) - 5, 0))
        wins.update(range(min(ws), max(ws) + 1))
    # the bucket: the anchors at or below the slot, counted
    psure = int((valid[1:] & (hi[1:] <= slot)).sum()) + 1
    pmaybe = int((valid[1:] & (lo[1:] <= slot) & (hi[1:] > slot)).sum())
    answers = {_tags(row, slot, symbol, max_symbol, wbs, max(8 * (p - 1) - 2, 0)) for wbs in wins for p in range(psure, psure + pmaybe + 1)}
    return next(iter(answers)) if len(answers) == 1 else frozenset(("ambiguous",))


# ------------------------------------------------------------------------------------------------------------- the census
class _TailPlanes(rr.OraclePlanes):
    """OraclePlanes that keeps what the last stage's rows were made from: the CNN's outputs and the prior channels of every position"""

    def table(self, lvl, band, clr, R, C, minv, maxv):
        t = super().table(lvl, band, clr, R, C, minv, maxv)
        if (lvl, band, clr) == (0, 2, 2):
            np_ = self.np
            par = self._par[1][:len(R), :len(C)].reshape(-1, 60)
            yv = (self.planes[0][np_.ix_(R, C)].astype(np_.float32) / np_.float32(255)).ravel()
            cov = (self.planes[1][np_.ix_(R, C)].astype(np_.float32) / np_.float32(255)).ravel()
            self.last = (par, yv, cov, minv, maxv)
        return t


def census(bl, weights, bound_scale=1.0, image=None):
    """bl: the oracle's rANS container (bytestream_list) of one image under `weights` -> (streams, symbols, extra): Counter of stream classes
    (one count per stream), Counter of symbol classes (one count per coded tail symbol and class; "coded" counts them all), and
    extra = dict(max_spill, anchor_gap: the largest |float64 anchor - exact entry| in units of the anchor's bound + 1, shapes_ok).
    bound_scale may be a sequence: the symbol counter then becomes a list, one per scale (one decode).
    The reader must accept the container as canonical; `image` (uint8 [3, H, W]), if given, must be what it decodes to."""
    from oracle import oracle as orc
    scales = list(bound_scale) if isinstance(bound_scale, (list, tuple)) else [bound_scale]
    segs = rr.segments(bl)
    pm = _TailPlanes(segs, weights)
    coded = []
    decoded, info = rr.decode(segs, pm.rows, canonical=True, on_tail=lambda m, j, row, slot, sym: coded.append((m, j, row, slot, sym)))
    pm.place(decoded)
    if image is not None:
        assert np.array_equal(orc.unlift(pm.planes), image), "the second reader decodes another image"
    hdr = info["header"]
    L, M = hdr["L"], hdr["M"]
    par, yv, cov, minv, maxv = pm.last
    nc = par.shape[0]
    max_symbol = maxv - minv
    streams = Counter()
    ncod_of = {}
    max_spill = 0
    for m, facts in enumerate(info["streams"]):
        cls, (kind, sn, NS, ncod) = stream_classes(hdr, facts, m)
        streams.update(cls)
        ncod_of[m] = ncod
        if facts["share"] and kind[0] == "X":
            max_spill = max(max_spill, facts["spill"])
            # the restated shape against the reader's facts: two chains iff the flag says so, their seeds, the coded count
            assert sn == (facts["n_seed"] if kind == "X2" else 1) and (kind == "X2") == ("gap" in facts)
    got = Counter(m for m, *_ in coded)
    assert all(got.get(m, 0) == n for m, n in ncod_of.items()), "the restated shape's coded count is not the number of symbols the reader decoded"
    symbols = [Counter() for _ in scales]
    gap = 0.0
    if coded:
        seqs = {m: [n for step in rr.stream_positions(nc, m, M, L) for n in step] for m in got}
        pos = np.array([seqs[m][len(seqs[m]) - 1 - j] for m, j, *_ in coded])
        mu, rsig, wn = components(par[pos], yv[pos], cov[pos])
        for si, sc in enumerate(scales):
            v, bound, i1 = anchors(mu, rsig, wn, minv, maxv, sc)
            for k, (m, j, row, slot, sym) in enumerate(coded):
                symbols[si].update(classify(row, slot, sym, v[k], bound[k], i1, max_symbol))
            symbols[si]["coded"] = len(coded)
            if si == 0:
                exact = np.array([[row[i] for i in i1] for _, _, row, _, _ in coded], np.float64)
                # (an entry is kept modulo 2^16; the anchors are not)
                diff = np.abs(((np.rint(v) + i1 - exact + 0x8000) % 0x10000) - 0x8000)
                gap = float((diff / (bound + 1.0)).max())
    extra = dict(max_spill=max_spill, anchor_gap=gap, header=hdr)
    return streams, (symbols if isinstance(bound_scale, (list, tuple)) else symbols[0]), extra


# ------------------------------------------------------------------------------------------------------------- inputs
def k_valued_image(H, W, k, seed=5):
    """R = B = 100, G in 100 .. 100 + k - 1 (helpers.two_valued_image for k = 2): the Cg channel has exactly k values, A = k"""
    img = np.full((3, H, W), 100, np.uint8)
    img[1] += np.random.default_rng(seed).integers(0, k, (H, W)).astype(np.uint8)
    return img


def grey_image(H, W, seed=13):
    g = np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    return np.stack([g, g, g])


def state_dict(wname):
    """A weight set by name: the two fixture sets ("rand1337", "trainedlike"), the cheap-source models of tests/test_oracle_golden.py's
    _cheap_case ("sharp", "single": same edits of the trained-like set) and the mixture regimes ("regime:<name>", tests/mixture_regimes.py)"""
    if wname.startswith("regime:"):
        import mixture_regimes as mr
        return mr.regime_state_dict(wname[7:])
    if wname in ("rand1337", "trainedlike"):
        return dict(np.load(os.path.join(GOLDEN, "weights_%s.npz" % wname)))
    assert wname in ("sharp", "single"), wname
    sd = dict(np.load(os.path.join(GOLDEN, "weights_trainedlike.npz")))
    for k in list(sd):
        if k.endswith("layers1toL.2.bias"):
            b = sd[k].copy()
            if wname == "sharp":
                b[0:15] *= 0.15
            else:
                b[0:15] = 0.6 / 255.0
                b[30:45] = np.tile(np.array([1.0, 1e-7, 1e-7, 1e-7, 1e-7], np.float32), 3)
            sd[k] = b
        if k.endswith("layers1toL.2.weight") and wname == "single":
            w = sd[k].copy()
            w[0:15] = 0.0
            w[30:45] = 0.0
            sd[k] = w
    return sd


_weights, _images, _containers = {}, {}, {}


def oracle_weights(wname):
    from llicti_amd.weights import pack_state_dict
    from oracle import oracle as orc
    if wname not in _weights:
        _weights[wname] = orc.Weights(pack_state_dict(state_dict(wname)))
    return _weights[wname]


def image_of(gen, H, W, seed, wname):
    """gen: "noise" | "smooth" (helpers.make_image), "flat", "grey", "bw", "k<k>" (k_valued_image), "sampled" (drawn from the weight set's own
    model: the reference-format decoder fed seeded random bytes behind the smooth image's header, helpers.make_sampled_image's method)"""
    from oracle import oracle as orc
    key = (gen, H, W, seed, wname if gen == "sampled" else None)
    if key not in _images:
        if gen in ("noise", "smooth"):
            img = make_image(gen, H, W, seed)
        elif gen == "flat":
            img = flat_image(H, W)
        elif gen == "grey":
            img = grey_image(H, W, seed)
        elif gen == "bw":
            img = bw_image(H, W, seed)
        elif gen[0] == "k":
            img = two_valued_image(H, W, seed) if gen == "k2" else k_valued_image(H, W, int(gen[1:]), seed)
        else:
            assert gen == "sampled", gen
            W_o = oracle_weights(wname)
            bl = orc.encode_image(make_image("smooth", H, W, 11), W_o)
            rng = np.random.default_rng(seed)
            bl = [list(bl[0])] + [[rng.integers(0, 256, len(s), dtype=np.uint8).tobytes() for s in row] for row in bl[1:]]
            img = orc.decode_image(bl, W_o)
        img = np.ascontiguousarray(img)
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def oracle_container(inp):
    """The oracle's container of one entry of INPUTS, once per process"""
    from oracle import oracle as orc
    if inp not in _containers:
        gen, H, W, seed, wname, wide, M = inp
        _containers[inp] = orc.encode_image_rans(image_of(gen, H, W, seed, wname), oracle_weights(wname), M, wide)
    return _containers[inp]


KIND_NAME = {0: "rans", 1: "wrans", 2: "xrans"}


def mode_name(inp):
    return "%s%d" % (KIND_NAME[inp[5]], inp[6])


# (image generator, H, W, seed, weight set, lane kind 0 = 64 / 1 = 128 / 2 = xwide lanes, M streams).  Found by a greedy search on the CPU over
# the generators, sizes 32 x 32 .. 70 x 100, seeds, weight sets, kinds and M = 1 .. 8 (the search is not committed, the list is): each entry
# was kept for a class it added.  The 181 x 181 flat image is the one larger input: its last stage holds 90 x 91 = 8,190 symbols on one stream.
INPUTS = (
    ('noise', 70, 100, 3, 'trainedlike', 2, 7),
    ('sampled', 34, 50, 8, 'regime:off_hi', 2, 6),
    ('smooth', 41, 44, 3, 'trainedlike', 2, 4),
    ('flat', 55, 60, 3, 'regime:floor', 2, 3),
    ('noise', 68, 87, 6, 'regime:off_lo', 0, 8),
    ('smooth', 64, 96, 5, 'single', 2, 1),
    ('k8', 66, 38, 5, 'rand1337', 2, 3),
    ('noise', 46, 83, 6, 'single', 0, 8),
    ('flat', 45, 79, 8, 'regime:off_lo', 2, 1),
    ('k3', 45, 74, 6, 'trainedlike', 2, 7),
    ('k2', 44, 70, 5, 'rand1337', 2, 4),
    ('k5', 67, 93, 4, 'trainedlike', 2, 8),
    ('flat', 181, 181, 0, 'single', 1, 1),
    ('flat', 181, 181, 0, 'trainedlike', 1, 1),
    ('grey', 37, 35, 3, 'trainedlike', 2, 2),
    ('flat', 35, 53, 4, 'trainedlike', 2, 3),
    ('k2', 38, 58, 7, 'regime:off_lo', 2, 5),
    ('flat', 46, 46, 2, 'rand1337', 2, 7),
    ('flat', 59, 40, 6, 'trainedlike', 2, 1),
    ('k2', 59, 41, 7, 'sharp', 2, 2),
    ('smooth', 51, 58, 9, 'trainedlike', 2, 3),
    ('flat', 62, 38, 9, 'regime:floor', 2, 6),
    ('flat', 46, 57, 7, 'single', 2, 3),
    ('grey', 70, 100, 9, 'sharp', 2, 2),
    ('flat', 43, 75, 3, 'regime:floor', 2, 3),
    ('k3', 64, 96, 7, 'single', 2, 1),
    ('noise', 64, 96, 7, 'single', 2, 2),
    ('smooth', 70, 100, 3, 'sharp', 2, 1),
    ('flat', 181, 181, 0, 'sharp', 2, 1),
    ('flat', 181, 181, 0, 'trainedlike', 2, 1),
    # no coded symbol (a share of ONE symbol behind a partial last chunk: 19 x 27 = 2 * 256 + 1, 25 x 41 = 4 * 256 + 1 positions)
    ('noise', 38, 54, 2, 'rand1337', 2, 3),
    ('smooth', 50, 82, 4, 'trainedlike', 2, 5),
    # one-chain xwide streams that spill: 1 .. 31 bits and more
    ('smooth', 64, 96, 9, 'trainedlike', 2, 1),
    ('smooth', 64, 96, 7, 'trainedlike', 2, 1),
    ('smooth', 67, 93, 5, 'trainedlike', 2, 1),
    # a second 64-lane and a second 128-lane input under the weight set of another one: the device test's mixed-size batches of those kinds
    ('smooth', 67, 93, 3, 'single', 0, 3),
    ('smooth', 33, 64, 4, 'single', 1, 2),
)

# search13 -- the bucket's twelve entries do not bracket the slot -- was NOT FOUND and is not in the required set.  Searched: 1,350 inputs
# (the generators above at 32 x 32 .. 70 x 100, seeds 1 .. 9, all three lane kinds, M = 1 .. 8) under the two fixture weight sets (rand1337 IS
# the sigma-floor model: its sigmas sit at the floor), "sharp", "single" and the regimes off_hi, off_lo and floor: 1.1 million coded tail symbols,
# none of them search13 with certainty or within the bound.  Reason: the bucket comes from the anchors' approximate entries, which differ from
# the exact ones by the bound above -- a few counts at most -- while the window reaches 2 entries below and 3 above the bucket's eight; an
# entry moves by at least one count per index (entry_from_sum adds the index).  It takes an approximation error of at least two entries'
# worth of counts, which term_fast does not have on any finite mixture tried.  The test reports it if an input ever reaches it.
SEARCH13_FOUND = False
