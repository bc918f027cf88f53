"""Float64 reference of the interpolator CNN, the mixture CDF tables and the self-information, with rigorous per-output error
bounds.  TEST INFRASTRUCTURE (CPU only, torch float64).

Written from the model definition, from the state dict with its reference key names: it does NOT go through
llicti_amd.weights.pack_state_dict (the K order, the transposes, the pre-summed layer-0 bias), so that a packing error is not cancelled
by the same error on both sides.  The oracle and the HIP kernels share the numerics spec (erfc_spec, the fmaf chains); this module
shares nothing with them but the fp32 inputs (the float planes the kernels read, the fp32 CNN outputs the table kernels read), cast up.

Every comparison is "fp32 result within a bound of the float64 value", the bound computed per output:
  * band_params64 / cnn_error_bound   -- the CNN;
  * cdf_entries64 (entries, tolerance) -- the 16-bit table entries;
  * selfinfo64 (values, tolerance)     -- -log2 of the mixture likelihood.
MUTANTS names deliberately wrong variants (a missing odd-edge pad, a shifted layer-0 tap, a dropped Co term in Cg's mean
update, no +-20-level push of the grid ends): tests/test_ref64_cpu.py asserts that each breaks its bound somewhere on the sweep shapes,
which is what shows the bounds tight enough to catch a subtle error.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

PREFIX = "entropymodel.entmdls_scale_band.0."
# band -> layer-0 convs (name, polyphase source (a, b), replicate pad (left, right, top, bottom)) (LLICTI_nets.py:651-675)
LAYER0 = {
    0: [("layer0_00_11", (0, 0), (1, 2, 1, 2))],
    1: [("layer0_00_01", (0, 0), (1, 2, 1, 1)), ("layer0_11_01", (1, 1), (1, 1, 2, 1))],
    2: [("layer0_00_10", (0, 0), (1, 1, 1, 2)), ("layer0_11_10", (1, 1), (2, 1, 1, 1)), ("layer0_01_10", (0, 1), (2, 1, 1, 2))],
}
TARGET = {0: (1, 1), 1: (0, 1), 2: (1, 0)}          # band -> polyphase component it codes (x11, x01, x10)
U = 2.0 ** -24                                      # unit roundoff of fp32
SCALE_BOUND = float(np.float32(0.11 / 255.0))      # compressai's bounds are fp32 buffers
WEIGHT_BOUND = float(np.float32(1e-6))
NORM_EPS = float(np.float32(1e-9))
LIK_BOUND = float(np.float32(1e-9))
HALF = 0.5 / 255.0
# erfc_spec's error budget (oracle/llicti_oracle.c, numerics.hpp):
# |erfc_spec(x) - erfc(x)| <= ERFC_REL * erfc(|x|) + ERFC_TAIL (+ U for x < 0: the rounding of 2 - v); ERFC_TAIL: erfc_spec is 0 from x = 7.
# Held for EVERY fp32 input by tests/test_numerics_cpu.py::test_erfc_budget_holds_for_every_float (the oracle, through
# tests/golden/numerics_sums.npz) with tests/test_hip_numerics.py::test_device_erfc_sums_equal_oracle (the device function has the oracle's
# bits on all 2^32 inputs); tests/test_ref64_cpu.py::test_erfc_spec_error_budget is the sampled check kept beside them.  The exhaustive
# maximum is 5.97 u relative (x = 2.0307915), so 6 u; the sampled 2.74e-7 (4.6 u) this constant once rested on, as 5 u, was too small.
ERFC_REL = 6.0 * U
ERFC_TAIL = math.erfc(7.0)
MUTANTS = ("no_odd_pad", "tap_shift", "cg_no_co", "no_grid_push")


def gamma(k):
    return k * U / (1.0 - k * U)


def level_geom(H, W, lvl):
    """(Hl, Wl, h, w): the level's grid and its band grid (the odd edge rounds up)."""
    st = 1 << lvl
    Hl, Wl = -(-H // st), -(-W // st)
    return Hl, Wl, (Hl + 1) // 2, (Wl + 1) // 2


def _t64(sd, key):
    v = sd[key]
    v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    return torch.from_numpy(np.asarray(v, dtype=np.float32).astype(np.float64))


def component(fp, lvl, a, b, h, w, mutant=None):
    """Polyphase component (a, b) of level lvl of float planes [3, H, W] (torch float64), on the band grid h x w.  lazyDWT pads the odd
    edge by replicating the component's own last row / column (LLICTI_nets.py:226-240).  mutant "no_odd_pad": the missing row / column is
    taken from the level grid's last row / column instead (the other phase) -- a clamp to the grid in place of the pad."""
    st = 1 << lvl
    Hl, Wl = fp.shape[1] // st + (fp.shape[1] % st > 0), fp.shape[2] // st + (fp.shape[2] % st > 0)
    rows = [min(2 * i + a, Hl - 1) if mutant == "no_odd_pad" else (2 * i + a if 2 * i + a < Hl else 2 * i + a - 2) for i in range(h)]
    cols = [min(2 * j + b, Wl - 1) if mutant == "no_odd_pad" else (2 * j + b if 2 * j + b < Wl else 2 * j + b - 2) for j in range(w)]
    lv = fp[:, ::st, ::st]
    return lv[:, rows][:, :, cols]


def _layer0_weight(sd, band, c, mutant):
    name = LAYER0[band][c][0]
    wt = _t64(sd, f"{PREFIX}{band}.{name}.weight").clone()
    if mutant == "tap_shift" and c == 0:            # tap (ky = 1, kx = 1) of the first conv reads one column to the right
        wt[:, :, 1, 2] += wt[:, :, 1, 1]
        wt[:, :, 1, 1] = 0.0
    return wt


def _cnn(fp, lvl, band, sd, absolute=False, mutant=None):
    """The CNN on float64 planes.  absolute: the same network on |W|, |b| and the given (non-negative) planes, without the ReLUs --
    what the error bound is built from."""
    H, W = fp.shape[1:]
    _, _, h, w = level_geom(H, W, lvl)
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    acc = None
    for c, (name, (a, b), pad) in enumerate(LAYER0[band]):
        x = F.pad(component(fp, lvl, a, b, h, w, mutant).unsqueeze(0), pad, mode="replicate")
        y = F.conv2d(x, f(_layer0_weight(sd, band, c, mutant)), f(_t64(sd, f"{PREFIX}{band}.{name}.bias")))
        acc = y if acc is None else acc + y
    return acc


def band_params64(fplanes, lvl, band, sd, mutant=None):
    """fplanes: fp32 [3, H, W] (what the kernels read), cast up.  -> float64 [h, w, 60] (sigma | mu | weight (Y, Co, Cg x 5) | a, b, d x 5)."""
    fp = torch.from_numpy(np.asarray(fplanes, dtype=np.float32).astype(np.float64))
    with torch.no_grad():
        y = F.relu(_cnn(fp, lvl, band, sd, mutant=mutant))
        y = F.relu(F.conv2d(y, _t64(sd, f"{PREFIX}{band}.layers1toL.0.weight"), _t64(sd, f"{PREFIX}{band}.layers1toL.0.bias"), groups=4))
        y = F.conv2d(y, _t64(sd, f"{PREFIX}{band}.layers1toL.2.weight"), _t64(sd, f"{PREFIX}{band}.layers1toL.2.bias"), groups=4)
    return y[0].permute(1, 2, 0).numpy()


def cnn_error_bound(fplanes, lvl, band, sd):
    """-> float64 [h, w, 60]: a rigorous bound of |fp32 CNN - band_params64| per output, for ANY summation order (the oracle's fmaf chains,
    MFMA's blocked sums alike).  The inputs are exact (the same fp32 planes); per layer, with a the exact pre-activation input and e_in its
    error bound (ReLU is 1-Lipschitz, so e passes through it),

        e_out = |W| e_in + gamma_K (|W| (|a| + e_in) + |b|),   gamma_K = K u / (1 - K u),  u = 2^-24,

    where K bounds the roundings on any path of the sum: the K0 products and the pre-summed biases of layer 0 (at most 3 convs: K0 + 3),
    the 88 products of a group plus one of layers 1 and 2.  |W| (|a| + e_in) + |b| is the same float64 network run on |W|, |b| and |a| + e_in
    (a bound of |computed input|): the rounding of those float64 sums (~1e-16 relative) is far below the bound's own slack."""
    fp = torch.from_numpy(np.abs(np.asarray(fplanes, dtype=np.float32)).astype(np.float64))
    K0 = {0: 48, 1: 72, 2: 120}[band] + 3
    fps = torch.from_numpy(np.asarray(fplanes, dtype=np.float32).astype(np.float64))
    with torch.no_grad():
        a0 = _cnn(fps, lvl, band, sd)                                        # exact layer-0 output (its float64 rounding: negligible)
        e0 = gamma(K0) * _cnn(fp, lvl, band, sd, absolute=True)
        h0 = F.relu(a0)
        W1, b1 = _t64(sd, f"{PREFIX}{band}.layers1toL.0.weight"), _t64(sd, f"{PREFIX}{band}.layers1toL.0.bias")
        W2, b2 = _t64(sd, f"{PREFIX}{band}.layers1toL.2.weight"), _t64(sd, f"{PREFIX}{band}.layers1toL.2.bias")
        a1 = F.conv2d(h0, W1, b1, groups=4)
        e1 = F.conv2d(e0, W1.abs(), groups=4) + gamma(89) * F.conv2d(h0 + e0, W1.abs(), b1.abs(), groups=4)
        h1 = F.relu(a1)
        e2 = F.conv2d(e1, W2.abs(), groups=4) + gamma(89) * F.conv2d(h1 + e1, W2.abs(), b2.abs(), groups=4)
    # (float64 slack of the reference itself: a relative 1e-13 of the absolute-value network)
    return (e2 * (1.0 + 1e-12))[0].permute(1, 2, 0).numpy()


# ------------------------------------------------------------------------------------------------ mixture CDF tables
def _erfc(x):
    return torch.special.erfc(x)


def _phi_min(z, dz):
    """max of the standard normal density over [z - dz, z + dz]."""
    zz = torch.clamp(z.abs() - dz, min=0.0)
    return torch.exp(-0.5 * zz * zz) / math.sqrt(2.0 * math.pi)


def _mixture(par60, clr, yv, cov, mutant=None):
    """fp32 parameters [N, 60] and prior-channel targets -> float64 (sigma, mu, wn, |dmu| bound), each [N, 5]."""
    p = torch.from_numpy(np.asarray(par60, dtype=np.float32).astype(np.float64))
    y = torch.from_numpy(np.asarray(yv, dtype=np.float32).astype(np.float64))[:, None]
    co = torch.from_numpy(np.asarray(cov, dtype=np.float32).astype(np.float64))[:, None]
    sg = torch.clamp(p[:, 5 * clr:5 * clr + 5], min=SCALE_BOUND)
    mu0 = p[:, 15 + 5 * clr:15 + 5 * clr + 5]
    if clr == 0:
        mu, dmu = mu0, U * mu0.abs()
    elif clr == 1:
        t = p[:, 45:50] * y
        mu = mu0 + t
        dmu = 2 * U * (mu0.abs() + t.abs())                     # the product's and the sum's rounding
    else:
        t1, t2 = p[:, 50:55] * y, p[:, 55:60] * co
        mu = mu0 + t1 + (0.0 if mutant == "cg_no_co" else t2)
        dmu = 3 * U * (mu0.abs() + t1.abs() + t2.abs())         # two products, two sums
    wk = torch.clamp(p[:, 30 + 5 * clr:30 + 5 * clr + 5], min=WEIGHT_BOUND)
    wn = wk / (NORM_EPS + wk.sum(1, keepdim=True))
    return sg, mu, wn, dmu


def grid64(Lp, minv, maxv, mutant=None):
    """Sample points of the Lp table entries (LLICTI_nets.py:941-942): half-integers / 255, the two ends pushed out by 20 levels."""
    g = (minv - 0.5 + torch.arange(Lp, dtype=torch.float64)) / 255.0
    if mutant != "no_grid_push":
        g[0] = (minv - 0.5 - 20.0) / 255.0
        g[-1] = (maxv + 0.5 + 20.0) / 255.0
    return g


def cdf_entries64(par60, clr, yv, cov, minv, maxv, mutant=None, with_tolerance=True):
    """The 16-bit table rows of N positions in float64: par60 fp32 [N, 60] (CNN outputs), yv / cov fp32 [N] (Y, Co targets / 255).
    -> (entries uint16 [N, Lp], tolerance int64 [N, Lp]) (tolerance None if not with_tolerance).

    entry_i = (round(C(pt_i) * S) + i) & 0xFFFF,  S = 65536 - (Lp - 1),  C(pt) = sum_k wn_k Phi((pt - mu_k) / sigma_k).

    Tolerance of entry i (in units of the entry, modulo 2^16): 1 + ceil(S dC), the 1 for the rounding to an integer when S C lies near a
    half-integer, and dC a first-order bound of the fp32 evaluation's error in C:
      * arguments: z_k = (pt - mu_k) / sigma_k.  fp32 computes pt (one rounding of the division; the end points one conversion), mu_k
        (dmu: each product and sum of the mean update rounds once), 1/sigma (one division), pt - mu, the product by 1/sigma and by the
        rounded -1/sqrt(2): |dz_k| <= (u |pt| + |dmu_k|) / sigma_k + 5 u |z_k|, and the term moves by at most
        phi(z_k') |dz_k| with phi's largest value on [z_k - dz_k, z_k + dz_k];
      * erfc_spec: 0.5 (ERFC_REL erfc(|x|) + ERFC_TAIL + u [x < 0]) per component (ERFC_REL = 6 u, held for every float: see ERFC_REL);
      * normalisation and sum: wn_k = w_k / (1e-9 + sum w) carries 7 u (four additions, the constant's, the division's), the products wn_k c_k
        and the four additions gamma_5, the final product by S one u:  (7 u + gamma_5 + u) C.
    Per entry, not one global constant: it is large only where a component is narrow and the grid point sits on its slope."""
    sg, mu, wn, dmu = _mixture(par60, clr, yv, cov, mutant)
    Lp = maxv - minv + 2
    S = float(65536 - (Lp - 1))
    pt = grid64(Lp, minv, maxv, mutant)
    N = sg.shape[0]
    ent = np.empty((N, Lp), np.uint16)
    tol = np.empty((N, Lp), np.int64) if with_tolerance else None
    idx = np.arange(Lp, dtype=np.int64)
    chunk = max(1, 2_000_000 // (5 * Lp))
    with torch.no_grad():
        for s in range(0, N, chunk):
            sl = slice(s, s + chunk)
            z = (pt[None, None, :] - mu[sl, :, None]) / sg[sl, :, None]          # [n, 5, Lp]
            x = z * (-1.0 / math.sqrt(2.0))
            c = 0.5 * _erfc(x)
            C = (wn[sl, :, None] * c).sum(1)
            q = torch.round(C * S).numpy().astype(np.int64)
            ent[sl] = ((q + idx[None, :]) & 0xFFFF).astype(np.uint16)
            if with_tolerance:
                dz = (U * pt.abs()[None, None, :] + dmu[sl, :, None]) / sg[sl, :, None] + 5 * U * z.abs()
                d_arg = (wn[sl, :, None] * _phi_min(z, dz) * dz).sum(1)
                d_erfc = (wn[sl, :, None] * 0.5 * (ERFC_REL * _erfc(x.abs()) + ERFC_TAIL + U * (x < 0))).sum(1)
                dC = d_arg + d_erfc + (8 * U + gamma(5)) * C
                tol[sl] = 1 + np.ceil(S * dC.numpy()).astype(np.int64)
    return ent, tol


def wrap_diff(a, b):
    """Signed difference of 16-bit table entries modulo 2^16."""
    d = (np.asarray(a, np.int64) - np.asarray(b, np.int64)) & 0xFFFF
    return np.where(d >= 0x8000, d - 0x10000, d)


# ------------------------------------------------------------------------------------------------ self-information
def selfinfo64(fplanes, lvl, band, par, with_tolerance=True):
    """-> (float64 [3, h, w] self-information in bits (Y, Co, Cg), tolerance [3, h, w] or None) of band `band` at level lvl; par fp32 [h, w, 60].

    s = -log2(max(L, 1e-9)),  L = sum_m wn_m (Phi((h - d_m) / s_m) - Phi((-h - d_m) / s_m)),  d_m = |v - mu_m|,  h = 0.5 / 255,
    wn_m = w_m / sum w.  Not bit-exact to anything (the kernel uses the hardware log2 and up - lo cancels), so the tolerance is built like the
    tables': each of up / lo moves by phi(z') |dz| (|dz| <= (u h + u |v| + |dmu| + u d) / s + 5 u |z|) plus erfc_spec's error, lik = up - lo
    rounds once (u |lik|), the normalisation 7 u and the sum gamma_5:  dL.  s then lies in [-log2(max(L + dL, 1e-9)), -log2(max(L - dL, 1e-9))],
    widened by the log2's own error (2^-20 absolute + 4 u relative)."""
    fp = np.asarray(fplanes, dtype=np.float32)
    H, W = fp.shape[1:]
    _, _, h, w = level_geom(H, W, lvl)
    a, b = TARGET[band]
    comp = component(torch.from_numpy(fp.astype(np.float64)), lvl, a, b, h, w)     # [3, h, w]: the targets (odd-edge pad included)
    v = comp.reshape(3, -1).T                                                       # [n, 3]
    P = par.reshape(-1, 60)
    out = np.empty((3, h * w))
    tol = np.empty((3, h * w)) if with_tolerance else None
    for clr in range(3):
        sg, mu, _, dmu = _mixture(P, clr, v[:, 0].numpy(), v[:, 1].numpy())
        p = torch.from_numpy(np.asarray(P, dtype=np.float32).astype(np.float64))
        wk = torch.clamp(p[:, 30 + 5 * clr:30 + 5 * clr + 5], min=WEIGHT_BOUND)
        wn = wk / wk.sum(1, keepdim=True)
        vv = v[:, clr:clr + 1]
        d = (vv - mu).abs()
        zu, zl = (HALF - d) / sg, (-HALF - d) / sg
        k = -1.0 / math.sqrt(2.0)
        up, lo = 0.5 * _erfc(k * zu), 0.5 * _erfc(k * zl)
        lik = up - lo
        L = (wn * lik).sum(1)
        out[clr] = -np.log2(np.maximum(L.numpy(), LIK_BOUND))
        if with_tolerance:
            dd = U * HALF + U * vv.abs() + dmu + U * d
            dzu, dzl = dd / sg + 5 * U * zu.abs(), dd / sg + 5 * U * zl.abs()
            e = lambda z, dz: _phi_min(z, dz) * dz + 0.5 * (ERFC_REL * _erfc((k * z).abs()) + ERFC_TAIL + U * (k * z < 0))
            dL = (wn * (e(zu, dzu) + e(zl, dzl) + U * lik.abs())).sum(1) + (7 * U + gamma(5)) * L
            Ln, dLn = L.numpy(), dL.numpy()
            hi = -np.log2(np.maximum(Ln - dLn, LIK_BOUND))
            lo_ = -np.log2(np.maximum(Ln + dLn, LIK_BOUND))
            tol[clr] = np.maximum(hi - out[clr], out[clr] - lo_) + 2.0 ** -20 + 4 * U * np.abs(out[clr])
    out = out.reshape(3, h, w)
    return out, (tol.reshape(3, h, w) if with_tolerance else None)
