"""Drop-in for the reference's `graphs.models.LLICTI_nets.LLICTI` on the encode/decode path.

Same constructor, `nn.Module` surface (33 `state_dict` entries with the reference's key names, so
`load_state_dict(ckpt['state_dict'])` works -- agents/base.py:51-76), `compress(x)` and `decompres(...)`
(sic: the missing "s" is part of the reference API, LLICTI_nets.py:161) with the reference's
`bytestream_list` container.  All computation is done by the gfx950 HIP library through
`llicti_amd.codec.HipCodec`; the torch modules below only hold parameters.  There is no CPU path:
calling compress/decompres without a GPU raises.

Differences from the reference, by design:
  * fp32 arithmetic follows the numerics spec (same bits on every launch shape / device), so
    decode(encode(x)) == x by construction, where the reference relies on PyTorch determinism;
  * `compress` accepts B >= 1 only through `compress_batch` (the reference's decoder assumes B == 1,
    LLICTI_nets.py:429, :443); `compress` itself keeps the B == 1 contract.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from ...codec import (MODE_AC, MODE_RANS, NSEG, HipCodec, auto_modes, bytestream_list_to_container, container_to_bytestream_list, header_dims, mode_of_header, mode_of_name, pixel_bytes, pixel_format, reduced_dims)
from ...archive import Batch
from ...progressive import ProgressiveBatch
from ...config import check_supported, model_shape


class _LowerBound(nn.Module):
    """Parameter-less stand-in that only carries compressai's `bound` buffer name (state_dict parity)."""

    def __init__(self, bound):
        super().__init__()
        self.register_buffer("bound", torch.Tensor([float(bound)]))


class _CondProbModel(nn.Module):
    """Buffer names of GaussianConditionalLosslessGMM (entropy_layer_nets.py:145-158)."""

    def __init__(self):
        super().__init__()
        self.likelihood_lower_bound = _LowerBound(1e-9)
        self.lower_bound_scale = _LowerBound(0.11 / 255.0)
        self.lower_bound_weights = _LowerBound(1e-6)


class LLICTIEntropyModel4(nn.Module):
    """Parameter container of one band interpolator (LLICTI_nets.py:585-712, config A branch).
    Construction order matches the reference so a seeded default init gives the same weights."""

    def __init__(self, scale, band, config, Ev, Od, Ch, Ly):
        super().__init__()
        self.band = band
        self.num_mixtures = config.num_mixtures
        self.conditional_prob_model = _CondProbModel()
        grps = 4
        Ch = grps * Ch
        Co = (3 * self.num_mixtures) * 3 + (1 + 2) * self.num_mixtures
        c = 3
        if band == 0:
            self.layer0_00_11 = nn.Conv2d(c, Ch, kernel_size=(Ev, Ev))
        if band == 1:
            self.layer0_00_01 = nn.Conv2d(c, Ch, kernel_size=(Od, Ev))
            self.layer0_11_01 = nn.Conv2d(c, Ch, kernel_size=(Ev, Od))
        if band == 2:
            self.layer0_00_10 = nn.Conv2d(c, Ch, kernel_size=(Ev, Od))
            self.layer0_11_10 = nn.Conv2d(c, Ch, kernel_size=(Od, Ev))
            self.layer0_01_10 = nn.Conv2d(c, Ch, kernel_size=(Ev, Ev))
        layers = []
        for _ in range((Ly - 1) - 1):
            layers.append(nn.Conv2d(Ch, Ch, kernel_size=1, groups=grps))
            layers.append(nn.ReLU(inplace=True))
        layers.append(nn.Conv2d(Ch, Co, kernel_size=1, groups=grps))
        self.layers1toL = nn.Sequential(*layers)


class LLICTIEntropyLayer(nn.Module):
    """LLICTI_nets.py:255-316 with useprevlevNN=[F,T,T,T,T]: one scale entry of three band models,
    shared by all five levels."""

    def __init__(self, config):
        super().__init__()
        self.list_scales = config.dwtlevels
        self.num_scales = len(self.list_scales)
        bands = nn.ModuleList()
        for b in range(3):
            bands.append(LLICTIEntropyModel4(scale=0, band=b, config=config, Ev=config.Evens[0], Od=config.Odds[0],
                                             Ch=config.chs[0], Ly=config.conv_layers))
        self.entmdls_scale_band = nn.ModuleList([bands])


class LLICTI(nn.Module):
    """(L)earned (L)ossless (I)mage (C)ompression (T)hrough (I)nterpolation -- MI355X hot path."""

    def __init__(self, config):
        super().__init__()
        check_supported(config)
        self.config = config
        self.ycocg = config.ycocg
        self.clrchs = config.clrchs
        self.clrjnt = config.clr_joint_mode
        self.list_scales = config.dwtlevels
        self.num_scales = len(self.list_scales)
        self.entropymodel = LLICTIEntropyLayer(config)
        self._codec = None
        self._weights_version = None
        # container written by compress().  config.container: "ac" = the reference's (torchac-compatible) format -- what compress() returns when the
        # config does not say; "xrans<M>" / "wrans<M>" / "rans<M>" = a rANS container with M streams per image; "auto" = xwide rANS streams (v4), their
        # number a function of the IMAGE'S SIZE alone (llicti_amd.codec.image_streams: 16 for 768x512 -- inside the north star's 0.001 bpp of the
        # reference format), so that an image's bytes do not depend on what it is coded with, next to or after.  LLICTIAgent.eval_model switches a
        # model whose config has NO container key -- the reference's own llicti_A.json -- to "auto" (set_container): there the north star's
        # "torchac replaced by a HIP rANS coder" is the default and the reference's byte format the opt-in.
        self.container_defaulted = "container" not in config
        self.set_container(str(config["container"]) if "container" in config else "ac")
        self._stage = {}                # pinned host staging buffers of the batched path, by (tag, slot): [buffer, event behind its last copy]
        self._xfer = {}                 # (upload, download) copy streams of the batched path, by device index
        self._last_decode = None        # (codec, full sizes, mode, reduce) of the last decode_batch_async: what last_digests() digests

    def set_container(self, name):
        """Container of the following compress() / encode_batch_async() calls: "ac", "rans<M>", "wrans<M>", "xrans<M>" or "auto"."""
        self.container = str(name)
        self.mode = None if self.container == "auto" else mode_of_name(self.container)

    # ------------------------------------------------------------------ plumbing
    def _weights_key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def codec(self, device=None) -> HipCodec:
        if self._codec is None:
            dev = device
            if dev is None:
                p = next(self.parameters())
                dev = p.device if p.is_cuda else None
            self._codec = HipCodec(dev)
            self._codec.set_model(*model_shape(self.config))       # (config B: 60-wide heads, 2 levels; a new context is config A)
        key = self._weights_key()
        if key != self._weights_version:
            self._codec.load_state_dict({k: v for k, v in self.state_dict().items()})
            self._weights_version = key
        return self._codec

    @torch.no_grad()
    def forward(self, x):
        """Validation likelihood (LLICTI_nets.py:101-123): x float32 [B,3,H,W] in {k/255} (or uint8), H and W
        multiples of 32 (lazyDWT(pad=False) needs equal sub-band sizes; the reference's validate() pads first,
        llicti_agent.py:105-113) -> list of L tensors (5: config A, 2: config B) [B, 9, h, w] of -log2 pmf in bits, scale 0 first,
        channel = 3 * band + colour.  Inference only: the kernels do not produce gradients (training stays
        outside this package)."""
        assert x.dim() == 4 and x.shape[1] == 3
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError("forward() needs H and W to be multiples of 32 (pad first, as llicti_agent.py:105-113 does)")
        codec = self.codec(x.device if x.is_cuda else None)
        return codec.forward_selfinfo(self._to_u8(x).to(codec.device).contiguous())

    @staticmethod
    def _to_u8(x):
        # dataloader tensors are uint8/255 as float32 (image_dl.py ToTensor); round(x*255) is the
        # reference's own first step (LLICTI_nets.py:65)
        if x.dtype == torch.uint8:
            return x
        return (x * 255).round().clamp_(0, 255).to(torch.uint8)

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def compress(self, x):
        """x: float32 [1,3,H,W] in {k/255} (or uint8) -> (bytestream_list, x_ycocg)  (LLICTI_nets.py:125-159)."""
        assert x.dim() == 4 and x.shape[1] == 3     # ensure x has 3 colour channels (LLICTI_nets.py:63)
        if x.shape[0] != 1:
            raise ValueError("compress() codes one image (the reference's decoder assumes B == 1); use compress_batch()")
        lists, x_ycocg = self.compress_batch(x)
        return lists[0], x_ycocg

    def mode_for_batch(self, B, device=None, sizes=None):
        """Container mode(s) of a call with B images of `sizes` [(H, W), ...] (one entry: all alike): the configured one, or for "auto" each image's
        own -- a function of its size (llicti_amd.codec.auto_modes), not of the batch, the device or anything coded before.  One int where all images
        get the same mode, else one per image (llicti_encode_images_vm)."""
        if self.mode is not None:
            return self.mode
        if not sizes:
            raise ValueError('container "auto" needs the image sizes')
        sz = list(sizes) if len(sizes) == B else [sizes[0]] * B
        modes = auto_modes(sz, self.num_scales)
        return modes[0] if all(m == modes[0] for m in modes) else modes

    def _pinned(self, key, nbytes):
        """Pinned host staging buffer (flat uint8, at least nbytes, grown to the running maximum) of `key` = (tag, slot).  The buffer's last
        asynchronous copy -- _pinned_mark() records an event behind it -- has finished when this returns: the host may rewrite it."""
        ent = self._stage.get(key)
        if ent is not None and ent[1] is not None:
            ent[1].synchronize()
            ent[1] = None
        if ent is None or ent[0].numel() < nbytes:
            ent = self._stage[key] = [torch.empty((int(nbytes * (1.25 if ent is not None else 1.0)),), dtype=torch.uint8).pin_memory(), None]
        return ent[0]

    def _pinned_mark(self, key, stream):
        """An asynchronous copy from / into the buffer of `key` has just been enqueued on `stream`."""
        ev = torch.cuda.Event()
        ev.record(stream)
        self._stage[key][1] = ev

    @torch.no_grad()
    def compress_batch(self, x):
        """x: [B,3,H,W] float32 in {k/255} or uint8 -> (list of B bytestream_lists, x_ycocg).  Synchronous."""
        enc = self.encode_batch_async(x, want_ycocg=True)
        return enc.lists(), enc.x_ycocg

    @torch.no_grad()
    def encode_batch_async(self, x, want_ycocg=False, slot=0, pixels=None, digests=False):
        """Enqueue the encode of a batch and the download of its containers (pinned host buffers); returns an EncodedBatch whose lists() waits
        for the download and cuts the containers into the reference's bytestream_lists.  Nothing here blocks the host: a caller can enqueue
        the next batch before it converts this one (LLICTIAgent.eval_model with eval_batch > 1).  `slot` selects one of the staging buffer
        sets (two batches in flight need two).
        x: a tensor [B,3,H,W] (float32 in {k/255} or uint8; host or device), or a LIST of B uint8 host arrays [3,H_b,W_b] whose sizes may
        differ (the reference's test loader yields arbitrary sizes, dataloaders/image_dl.py:40-45): one call, one upload, one download.
        pixels = "rgb" | "bgr" | "rgba" | "bgra": x is a LIST of uint8 host arrays [H_b, W_b, 3 | 4], interleaved as image files, PIL and OpenCV
        hold them -- uploaded as they are and lifted from that layout on the device (HipCodec.encode_px; alpha is ignored): the same containers
        as the planar list, without a transpose on the host.  EncodedBatch.rgb is then the flat INTERLEAVED device buffer.
        pixels = "f32": x is a float32 DEVICE tensor [B,3,H,W] in {k/255}, or a list of such tensors [3,H_b,W_b] (or [1,3,H_b,W_b]) whose sizes may
        differ; the encode's first kernel reads the floats (HipCodec.encode_f32: round(x * 255) half to even, clamped, as _to_u8) -- no conversion
        pass, the same containers.  EncodedBatch.rgb is then the flat float32 device buffer.
        digests=True: the pixel digests of the batch (HipCodec.digests: zlib.crc32 of every image's planar uint8 [3][H][W] bytes) are computed
        directly behind the encode, from the planes it left in its workspace, and downloaded under the handle's event: EncodedBatch.digests().
        Without the flag the call is exactly the call it was."""
        if pixels == "f32":
            return self._encode_f32_async(x, slot, digests)
        if pixels is not None and not isinstance(x, (list, tuple)):
            raise ValueError("pixels=...: the batch is a list of uint8 [H, W, C] arrays")
        if isinstance(x, (list, tuple)):
            imgs = [np.ascontiguousarray(a) for a in x]
            if pixels is not None:
                fmt = pixel_format(pixels)
                bpp = pixel_bytes(fmt)
                if any(a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != bpp for a in imgs):
                    raise ValueError(f"a pixels={pixels!r} batch holds uint8 [H, W, {bpp}] arrays")
                Hs, Ws = [int(a.shape[0]) for a in imgs], [int(a.shape[1]) for a in imgs]
            else:
                if any(a.dtype != np.uint8 or a.ndim != 3 or a.shape[0] != 3 for a in imgs):
                    raise ValueError("a list batch holds uint8 [3, H, W] arrays")
                Hs, Ws = [int(a.shape[1]) for a in imgs], [int(a.shape[2]) for a in imgs]
            codec = self.codec(None)
            total = sum(a.size for a in imgs)            # the images back to back, tightly packed: flat_offsets() / encode_px's default placement
            host = self._pinned(("rgb_in", slot), total)
            hv, o = host.numpy(), 0
            for a in imgs:
                hv[o:o + a.size] = a.reshape(-1)
                o += a.size
            cur = torch.cuda.current_stream(codec.device)
            up, down = self._copy_streams(codec.device)
            with torch.cuda.stream(up):
                rgb = host[:total].to(codec.device, non_blocking=True)
            self._pinned_mark(("rgb_in", slot), up)
            cur.wait_stream(up)
            rgb.record_stream(cur)
            t0 = torch.cuda.Event(enable_timing=True)              # the compute stream has the batch: what follows is encode time, not upload wait
            t0.record(cur)
            B = len(imgs)
            mode = self.mode_for_batch(B, codec.device, sizes=list(zip(Hs, Ws)))
            cont, seg = codec.encode_v(rgb, Hs, Ws, mode) if pixels is None else codec.encode_px(rgb, Hs, Ws, mode, fmt)
            crc = codec.digests(Hs, Ws, mode)[0] if digests else None      # (before anything else can use the workspace)
            x_ycocg = None
        else:
            t0 = None
            codec = self.codec(x.device if x.is_cuda else None)
            cur = torch.cuda.current_stream(codec.device)
            up, down = self._copy_streams(codec.device)
            xu = self._to_u8(x)
            if xu.is_cuda:
                rgb = xu.to(codec.device).contiguous()
            else:
                # host input (pinned by the caller for a true async copy): uploaded on the copy stream, so that it runs under whatever the
                # compute stream is doing (the previous batch's decode); the compute stream waits for it, nothing else does
                with torch.cuda.stream(up):
                    rgb = xu.to(codec.device, non_blocking=True).contiguous()
                cur.wait_stream(up)
                rgb.record_stream(cur)
            B, _, H, W = rgb.shape
            Hs, Ws = [H] * B, [W] * B
            mode = self.mode_for_batch(B, codec.device, sizes=[(H, W)])
            cont, seg = codec.encode(rgb, mode=mode)
            crc = codec.digests(Hs, Ws, mode)[0] if digests else None
            # x_ycocg = (YCoCg - [127,0,0]) / 255 (LLICTI_nets.py:143-144): the float planes the reference hands back beside the streams -- the encode
            # has just computed them: copied out of its workspace, not lifted a second time
            x_ycocg = codec.encoded_fplanes(B, H, W, mode) if want_ycocg else None
        nb = cont.numel()
        seg_h = self._pinned(("seg", slot), B * NSEG * 4)[:B * NSEG * 4].view(torch.int32).view(B, NSEG)
        cont_h = self._pinned(("cont_out", slot), nb)[:nb].view(tuple(cont.shape))
        crc_h = None if crc is None else self._pinned(("crc", slot), B * 8)[:B * 8].view(torch.int64)
        # the download runs on its own stream behind the encode: the compute stream goes straight on to the next enqueued call
        down.wait_stream(cur)
        with torch.cuda.stream(down):
            seg_h.copy_(seg, non_blocking=True)
            cont_h.copy_(cont, non_blocking=True)                  # one contiguous copy of the container strides (bytes past a container's own length: undefined)
            self._download_crc(crc, crc_h, slot, down)
            ev = torch.cuda.Event()
            ev.record(down)
        self._pinned_mark(("seg", slot), down)
        self._pinned_mark(("cont_out", slot), down)
        cont.record_stream(down)
        seg.record_stream(down)
        enc = EncodedBatch(codec, rgb, cont_h, seg_h, ev, x_ycocg, mode, Hs, Ws)
        enc.t0 = t0
        enc.crc_h = crc_h
        return self._with_records(enc, cont, seg, slot)

    def _download_crc(self, crc, crc_h, slot, down):
        """the digests of an encode into their pinned buffer, on the download stream (the caller has it current); nothing without digests"""
        if crc is None:
            return
        crc_h.copy_(crc, non_blocking=True)
        self._pinned_mark(("crc", slot), down)
        crc.record_stream(down)

    def _encode_f32_async(self, x, slot, digests=False):
        """encode_batch_async(pixels="f32"): float32 device tensors in, EncodedBatch out."""
        imgs = list(x) if isinstance(x, (list, tuple)) else [x]
        if any(not isinstance(a, torch.Tensor) or not a.is_cuda or a.dtype != torch.float32 for a in imgs):
            raise ValueError('a pixels="f32" batch holds float32 device tensors')
        if isinstance(x, torch.Tensor):
            if x.dim() != 4 or x.shape[1] != 3:
                raise ValueError('a pixels="f32" tensor is [B, 3, H, W]')
            B, _, H, W = x.shape
            Hs, Ws = [H] * B, [W] * B
            flat = x.contiguous().view(-1)
        else:
            imgs = [a[0] if a.dim() == 4 and a.shape[0] == 1 else a for a in imgs]
            if any(a.dim() != 3 or a.shape[0] != 3 for a in imgs):
                raise ValueError('a pixels="f32" list holds tensors [3, H, W]')
            Hs, Ws = [int(a.shape[1]) for a in imgs], [int(a.shape[2]) for a in imgs]
            flat = torch.cat([a.reshape(-1) for a in imgs])
            B = len(imgs)
        codec = self.codec(flat.device)
        cur = torch.cuda.current_stream(codec.device)
        _, down = self._copy_streams(codec.device)
        mode = self.mode_for_batch(B, codec.device, sizes=list(zip(Hs, Ws)))
        cont, seg = codec.encode_f32(flat, Hs, Ws, mode)
        crc = codec.digests(Hs, Ws, mode)[0] if digests else None
        nb = cont.numel()
        seg_h = self._pinned(("seg", slot), B * NSEG * 4)[:B * NSEG * 4].view(torch.int32).view(B, NSEG)
        cont_h = self._pinned(("cont_out", slot), nb)[:nb].view(tuple(cont.shape))
        crc_h = None if crc is None else self._pinned(("crc", slot), B * 8)[:B * 8].view(torch.int64)
        down.wait_stream(cur)
        with torch.cuda.stream(down):
            seg_h.copy_(seg, non_blocking=True)
            cont_h.copy_(cont, non_blocking=True)
            self._download_crc(crc, crc_h, slot, down)
            ev = torch.cuda.Event()
            ev.record(down)
        self._pinned_mark(("seg", slot), down)
        self._pinned_mark(("cont_out", slot), down)
        cont.record_stream(down)
        seg.record_stream(down)
        enc = EncodedBatch(codec, flat, cont_h, seg_h, ev, None, mode, Hs, Ws)
        enc.crc_h = crc_h
        return self._with_records(enc, cont, seg, slot)

    def _with_records(self, enc, cont, seg, slot):
        """What EncodedBatch.records() needs: the device containers and segment lengths of the encode (kept alive by the handle) and the pinned
        staging buffer of the dense download."""
        enc.cont_d, enc.seg_d = cont, seg
        enc._rec_stage = lambda nbytes: self._pinned(("rec_out", slot), nbytes)
        return enc

    def _copy_streams(self, device):
        """(upload, download) HIP streams of a device for the batched calls' transfers (created once): PCIe copies next to the kernels, not
        between them -- on one stream they cost a 24-image encode + decode 2.6 ms of a compute queue that is otherwise never idle."""
        key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
        if key not in self._xfer:
            self._xfer[key] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
        return self._xfer[key]

    @torch.no_grad()
    def decompres(self, bytestream_list, devc=None, xorg=None, reduce=0):
        """bytestream_list -> float32 [1,3,H,W] (LLICTI_nets.py:161-179).  xorg: the reference's diagnostic (:167-171) -- the float planes
        compress() returned; the decoded planes are compared with them on the device and a difference of a grey level or more is reported.
        reduce = r (0 .. the model's levels; not in the reference): float32 [1,3,ceil(H/2^r),ceil(W/2^r)] = the full result's [..., ::2^r, ::2^r],
        decoded from the levels >= r alone (3 (levels - r) of the band-CNN launches).  A decimation, not a low-pass: fine texture aliases.  For
        r >= 1 a rANS container's end-of-stream check is not run (it belongs to the last stage); xorg is compared at [..., ::2^r, ::2^r]."""
        rgb = self.decode_batch_async([bytestream_list], devc, reduce=reduce)
        codec = self.codec()
        codec.check()
        if xorg is not None:
            if reduce:
                # (a reduced image may be smaller than the 32 pixels the lift kernel takes: this diagnostic's few integer ops run in torch)
                R, G, Bl = (rgb[:, k].to(torch.int32) for k in range(3))
                Co = R - Bl
                t = Bl + (Co >> 1)
                Cg = G - t
                planes = torch.stack((t + (Cg >> 1) - 127, Co, Cg), dim=1).to(torch.float32) / 255
                xorg = xorg[..., ::1 << reduce, ::1 << reduce]
            else:
                planes = codec.lift(rgb)[1]                        # (YCoCg - [127,0,0]) / 255 of the decoded image, as compress() returns it
            maxx_abserr = float((xorg.to(planes.device) - planes).abs().max()) * 255
            if maxx_abserr >= 1.0:                                 # LLICTI_nets.py:169-171
                print("Error: Decoded YCoCg img does NOT match original YCoCg image perfectly! The maximum of absolute error is {:.4f}".format(maxx_abserr))
        return rgb.to(torch.float32) / 255           # LLICTI_nets.py:87

    @torch.no_grad()
    def decompres_batch(self, lists, devc=None, reduce=0):
        """bytestream_lists of B images -> float32 [B,3,H,W] (equal sizes), or -- images of different sizes, rANS containers -- a LIST of B tensors
        [1,3,H_b,W_b], each what decompres() returns for that image.  reduce: as for decompres() -- one value for the call, or one per image
        (rANS containers): then always the list, image b at its own reduced size."""
        res = self.decode_batch_async(lists, devc, reduce=reduce)
        self.codec().check()
        if isinstance(res, tuple):
            flat, Hs, Ws = res
            offs, _ = self.codec().flat_offsets(Hs, Ws)
            return [flat[int(o):int(o) + 3 * h * w].view(1, 3, h, w).to(torch.float32) / 255 for o, h, w in zip(offs, Hs, Ws)]
        return res.to(torch.float32) / 255           # LLICTI_nets.py:87

    def _upload_lists(self, lists, devc=None, slot=0):
        """bytestream_lists of B images -> their containers and segment lengths on the device (one upload from the pinned staging buffers, on the copy
        stream; the compute stream waits for it): (codec, containers [B, stride], seg_len [B, 49], Hs, Ws, mode -- one int or one per image, read from
        the headers --, mixed)."""
        codec = self.codec(devc if (devc is not None and torch.device(devc).type == "cuda") else None)
        Hs, Ws, modes = [], [], []
        for bl in lists:
            if len(bl) != 1 + self.num_scales or any(len(r) != 9 for r in bl):
                raise ValueError(f"bytestream_list must be {1 + self.num_scales} lists of 9 byte strings (1 + the model's {self.num_scales} levels)")
            if len(bl[0][0]) != 3 or len(bl[0][1]) != 12 or len(bl[0][2]) != 2:
                raise ValueError("malformed header streams")
            hdr = bytes(bl[0][0]) + bytes(bl[0][1]) + bytes(bl[0][2])
            modes.append(mode_of_header(hdr))           # AC container: hdr[0] == num_scales (LLICTI_nets.py:424); rANS: its lane kind and stream count
            H, W = header_dims(hdr)
            Hs.append(H)
            Ws.append(W)
        if any((m & ~0xFF) != (modes[0] & ~0xFF) for m in modes):
            raise ValueError("all images of one decompres_batch call must be in the same kind of container (their stream counts may differ)")
        mode = modes[0] if all(m == modes[0] for m in modes) else modes
        B = len(lists)
        mixed = any(h != Hs[0] or w != Ws[0] for h, w in zip(Hs, Ws)) or isinstance(mode, list)
        if mixed and modes[0] == MODE_AC:
            raise ValueError("images of different sizes in the reference-format container decode one size per call")
        stride = max(codec.max_container_bytes(h, w) for h, w in set(zip(Hs, Ws)))
        cont_h = self._pinned(("cont_in", slot), B * stride)[:B * stride].view(B, stride)
        seg_h = self._pinned(("seg_in", slot), B * NSEG * 4)[:B * NSEG * 4].view(torch.int32).view(B, NSEG)
        cont_np, seg_np = cont_h.numpy(), seg_h.numpy()
        for i, bl in enumerate(lists):
            pos, k = 0, 0
            for r, row in enumerate(bl):
                for s in (row[:4] if r == 0 else row):
                    n = len(s)
                    if pos + n > stride:
                        raise ValueError("container larger than any valid stream set for this image size")
                    if n:
                        cont_np[i, pos:pos + n] = np.frombuffer(s, dtype=np.uint8)
                    seg_np[i, k] = n
                    pos += n
                    k += 1
            seg_np[i, k:] = 0                            # (config B: 22 segments; the pinned buffer is reused)
        cur = torch.cuda.current_stream(codec.device)
        up, _ = self._copy_streams(codec.device)
        with torch.cuda.stream(up):
            cont_d = cont_h.to(codec.device, non_blocking=True)  # one contiguous copy; bytes past a container's own length are never read (validated lengths)
            seg_d = seg_h.to(codec.device, non_blocking=True)
        self._pinned_mark(("cont_in", slot), up)
        self._pinned_mark(("seg_in", slot), up)
        cur.wait_stream(up)
        cont_d.record_stream(cur)
        seg_d.record_stream(cur)
        return codec, cont_d, seg_d, Hs, Ws, mode, mixed

    def _upload_batch(self, batch, devc=None):
        """_upload_lists for an archive.Batch (ArchiveReader.read_batch): ONE copy of the dense blob and its offsets on the copy stream, then
        HipCodec.unpack_records on the compute stream cuts it into containers of the batch's tight stride -- no per-image host work, no padding
        over PCIe.  Sizes and modes are the index's; a record the device refuses (or whose header contradicts the index) is flagged per image
        by the decode that follows."""
        codec = self.codec(devc if (devc is not None and torch.device(devc).type == "cuda") else None)
        Hs, Ws, modes = [int(h) for h in batch.Hs], [int(w) for w in batch.Ws], [int(m) for m in batch.modes]
        B = len(Hs)
        if B < 1 or len(batch.rec_off) != B + 1:
            raise ValueError("an archive batch holds B >= 1 images and B + 1 record offsets")
        if any((m & ~0xFF) != (modes[0] & ~0xFF) for m in modes):
            raise ValueError("all images of one decompres_batch call must be in the same kind of container (their stream counts may differ)")
        mode = modes[0] if all(m == modes[0] for m in modes) else modes
        mixed = any(h != Hs[0] or w != Ws[0] for h, w in zip(Hs, Ws)) or isinstance(mode, list)
        if mixed and modes[0] == MODE_AC:
            raise ValueError("images of different sizes in the reference-format container decode one size per call")
        blob_h = batch.blob if isinstance(batch.blob, torch.Tensor) else torch.from_numpy(np.frombuffer(batch.blob, dtype=np.uint8).copy())
        ro_h = torch.from_numpy(np.ascontiguousarray(batch.rec_off, dtype=np.int64))
        cur = torch.cuda.current_stream(codec.device)
        up, _ = self._copy_streams(codec.device)
        with torch.cuda.stream(up):
            blob_d = blob_h.to(codec.device, non_blocking=True)
            ro_d = ro_h.to(codec.device, non_blocking=True)
        cur.wait_stream(up)
        blob_d.record_stream(cur)
        ro_d.record_stream(cur)
        with torch.cuda.device(codec.device):
            if isinstance(batch, ProgressiveBatch):      # prefixes of progressive records: the levels >= batch.reduce[b] of image b, nothing else
                cont_d, seg_d = codec.unpack_progressive(blob_d, ro_d, reduce=[int(r) for r in batch.reduce], stride=int(batch.stride))
            else:
                cont_d, seg_d = codec.unpack_records(blob_d, ro_d, stride=int(batch.stride))
        return codec, cont_d, seg_d, Hs, Ws, mode, mixed

    @torch.no_grad()
    def transcode_batch(self, lists, container=None, devc=None, slot=0):
        """bytestream_lists of B images -> their bytestream_lists in `container` ("ac", "rans<M>", "wrans<M>", "xrans<M>", "auto"; default: the
        model's set_container value), each what compress() of the decoded image gives in that container -- without decoding to pixels and coding
        again: one pass of the band CNN instead of two (HipCodec.transcode).  The source containers' kinds and the sizes are read from the
        headers as decode_batch_async does; "auto" gives every image the mode of its size (auto_modes).  Synchronous; device-side failures
        (a malformed source container) raise through codec().check()."""
        codec, cont_d, seg_d, Hs, Ws, src_mode, _ = self._upload_lists(lists, devc, slot)
        name = self.container if container is None else str(container)
        B = len(lists)
        if name == "auto":
            modes = auto_modes(list(zip(Hs, Ws)), self.num_scales)
            dst_mode = modes[0] if all(m == modes[0] for m in modes) else modes
        else:
            dst_mode = mode_of_name(name)
        cur = torch.cuda.current_stream(codec.device)
        _, down = self._copy_streams(codec.device)
        cont, seg = codec.transcode(cont_d, seg_d, Hs, Ws, src_mode, dst_mode)
        nb = cont.numel()
        seg_h = self._pinned(("seg", slot), B * NSEG * 4)[:B * NSEG * 4].view(torch.int32).view(B, NSEG)
        cont_h = self._pinned(("cont_out", slot), nb)[:nb].view(tuple(cont.shape))
        down.wait_stream(cur)
        with torch.cuda.stream(down):
            seg_h.copy_(seg, non_blocking=True)
            cont_h.copy_(cont, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(down)
        self._pinned_mark(("seg", slot), down)
        self._pinned_mark(("cont_out", slot), down)
        cont.record_stream(down)
        seg.record_stream(down)
        return EncodedBatch(codec, None, cont_h, seg_h, ev, None, dst_mode, Hs, Ws).lists()

    @torch.no_grad()
    def decode_batch_async(self, lists, devc=None, slot=0, flat=False, reduce=None, pixels=None, tensor=None):
        """bytestream_lists of B images -> uint8 [B,3,H,W] on the device, enqueued (upload from a pinned buffer + decode); device-side
        failures are reported by codec().check() / image_status().  The images of a call share a container kind; in a rANS container their
        SIZES may differ -- then (or with flat=True) the result is (flat uint8 device tensor, Hs, Ws): the images back to back, [3][H][W] each.
        reduce = r: every image at 1 / 2^r (decompres()); H, W, Hs, Ws of the result are the REDUCED sizes.  reduce = [r_0, ...], one per image
        (rANS containers): image b stops at its own level -- exactly what the call at r_b gives for it -- and the finer levels run for the images
        that need them alone; the result is the flat form, Hs, Ws each image's own reduced size; with tensor= the origins, boxes and views are
        in the coordinates of each image's own decimated grid (codec.resized_crop_plan / multi_crop_plan with per_image=True).  (The pinned staging buffers hold the
        call's INPUT -- containers and segment lengths, sized by the full image -- so a reduced and a full decode share them safely.)
        pixels = "rgb" | "bgr" | "rgba" | "bgra": the result is a LIST of B uint8 device tensors [H_b, W_b, 3 | 4], interleaved (alpha 255), written
        in that layout by the decode's last kernel (HipCodec.decode_px) -- views of one flat buffer, the images back to back; with flat=True
        (that flat buffer, Hs, Ws) instead.
        tensor = dict(size=(Ho, Wo), dtype=, origin=, flip=, mean=, std=) (only size is required): the result is ONE device tensor [B,3,Ho,Wo] of
        dtype (float32 by default), every image's window cropped, flipped and normalised by the decode's last kernel (HipCodec.decode_tensor) --
        the images' sizes may differ.  Not together with pixels= or flat=.
        tensor = dict(size=(Ho, Wo), boxes=[(y0, x0, hs, ws), ...], antialias=, dtype=, flip=, mean=, std=): with `boxes` every image's source box
        (decoded coordinates: the reduced ones for reduce >= 1; codec.resized_crop_plan maps full-resolution boxes and picks reduce) is RESAMPLED
        to size by that kernel (HipCodec.decode_tensor_resized) -- a random resized crop per image; `origin` does not go with it.
        tensor = dict(views=[group, ...], mean=, std=): SEVERAL crops per image from one decode (HipCodec.decode_tensor_views, which describes a
        group: size, image, boxes, flip, dtype, antialias, out) -> a list of one tensor [n, 3, Ho, Wo] per group; codec.multi_crop_plan picks
        reduce.  `views` goes with neither `boxes`, `origin` nor `size` at the top level.
        Every form takes channels_last=True: the tensor(s) come out as [n, 3, Ho, Wo] in torch.channels_last, interleaved by the same kernel.
        The `origin` form also takes pad=dict(mode="constant" | "edge" | "reflect" | "symmetric", fill=, space="pixel" | "output"): windows may
        then leave their images and origins be negative (HipCodec.decode_tensor states the modes); codec.center_crop_origins gives
        torchvision's CenterCrop windows, the images smaller than the crop included.
        lists may be an archive.Batch (ArchiveReader.read_batch) instead: the records of B images in one host buffer -- one dense upload and
        HipCodec.unpack_records in place of the per-image staging (`slot` is not used: the batch owns its buffer, which must stay untouched until
        the upload has run); sizes and modes are the archive index's, everything behind the containers is the same path.
        lists may be a progressive.ProgressiveBatch (ProgressiveReader.read_batch(reduce=...)): the PREFIXES of the images' progressive records,
        holding the levels >= batch.reduce[b] of image b alone -- HipCodec.unpack_progressive in place of unpack_records.  reduce= then defaults to
        the batch's; a requested r_b BELOW what the batch holds for its image is a ValueError (those bytes were never read).  Otherwise reduce
        defaults to 0."""
        if tensor is not None and (pixels is not None or flat):
            raise ValueError("tensor=... gives one dense float tensor: it goes with neither pixels= nor flat=")
        if isinstance(lists, ProgressiveBatch):
            held = [int(r) for r in lists.reduce]
            if reduce is None:
                reduce = held[0] if all(r == held[0] for r in held) else held
            want = [int(reduce)] * len(held) if isinstance(reduce, (int, np.integer)) else [int(r) for r in reduce]
            if len(want) == len(held) and any(w < h for w, h in zip(want, held)):
                raise ValueError(f"reduce {want} asks for finer levels than the batch holds ({held}): read the batch at the reduce it is decoded at")
        elif reduce is None:
            reduce = 0
        if isinstance(lists, (Batch, ProgressiveBatch)):        # an archive's records: one dense upload, cut into containers on the device
            codec, cont_d, seg_d, Hs, Ws, mode, mixed = self._upload_batch(lists, devc)
        else:
            codec, cont_d, seg_d, Hs, Ws, mode, mixed = self._upload_lists(lists, devc, slot)
        per_image = not isinstance(reduce, (int, np.integer))
        if per_image:
            reduce = [int(r) for r in reduce]
            if len(reduce) != len(Hs):
                raise ValueError(f"reduce: {len(reduce)} values for a batch of {len(Hs)} images (one int, or one per image)")
        self._last_decode = (codec, list(Hs), list(Ws), mode, reduce)      # (last_digests: the FULL sizes, whatever the form of the result)
        # the images' decoded sizes (a value the library refuses: it says so in the decode call)
        red_sizes = lambda: (list(v) for v in zip(*(reduced_dims(h, w, r) for h, w, r in zip(Hs, Ws, reduce if per_image else [reduce] * len(Hs)))))
        if tensor is not None and "views" in tensor:
            if any(k in tensor for k in ("boxes", "origin", "size")):
                raise ValueError("tensor=dict(views=...): every group has its own size and boxes; boxes=, origin= and size= do not go beside it")
            rest = {k: v for k, v in tensor.items() if k != "views"}
            return codec.decode_tensor_views(cont_d, seg_d, Hs, Ws, mode, tensor["views"], reduce=reduce, **rest)
        if tensor is not None and "boxes" in tensor:
            return codec.decode_tensor_resized(cont_d, seg_d, Hs, Ws, mode, reduce=reduce, **tensor)      # (an `origin` beside boxes: a TypeError)
        if tensor is not None:
            return codec.decode_tensor(cont_d, seg_d, Hs, Ws, mode, reduce=reduce, **tensor)
        if pixels is not None:
            bpp = pixel_bytes(pixels)
            out = codec.decode_px(cont_d, seg_d, Hs, Ws, mode, pixels, reduce=reduce)
            if per_image or reduce:
                Hs, Ws = red_sizes()
            if flat:
                return out, Hs, Ws
            offs = np.concatenate(([0], np.cumsum([h * w * bpp for h, w in zip(Hs, Ws)])))
            return [out[int(o):int(o) + h * w * bpp].view(h, w, bpp) for o, h, w in zip(offs, Hs, Ws)]
        if mixed or flat or per_image:
            out = codec.decode_v(cont_d, seg_d, Hs, Ws, mode, reduce=reduce)
            if per_image or reduce:
                Hs, Ws = red_sizes()
            return out, Hs, Ws
        return codec.decode(cont_d, seg_d, Hs[0], Ws[0], mode=mode, reduce=reduce)

    def last_digests(self):
        """The pixel digests of the images of the model's last decode_batch_async, whatever its form (planar, pixels=, tensor= with a window,
        boxes or views) -> (crc, have): HipCodec.digests' int64 and int32 device tensors [B], enqueued on the current stream without a
        synchronisation -- crc[b] = zlib.crc32 of image b's pixels as planar uint8 [3][H][W] bytes where have[b] = 1 (an image decoded at
        reduce >= 1 has have = 0).  A loader compares against its manifest with one device `!=`.  Call it before another whole-batch call of
        this model's codec reuses the workspace."""
        if self._last_decode is None:
            raise ValueError("last_digests: no decode_batch_async has run on this model")
        codec, Hs, Ws, mode, reduce = self._last_decode
        with torch.cuda.device(codec.device):
            return codec.digests(Hs, Ws, mode, reduce=reduce if (isinstance(reduce, list) or reduce) else None)


class EncodedBatch:
    """Handle of one enqueued batch encode (LLICTI.encode_batch_async): the device input, the pinned host copies of the containers and
    their segment lengths, and the event recorded behind the download."""

    def __init__(self, codec, rgb, cont_h, seg_h, ev, x_ycocg, mode, Hs=None, Ws=None):
        self.codec, self.rgb, self.cont_h, self.seg_h, self.ev = codec, rgb, cont_h, seg_h, ev
        self.x_ycocg, self.mode = x_ycocg, mode
        self.Hs, self.Ws = Hs, Ws           # per image (a list batch: rgb is the flat device buffer, the images back to back)
        self.t0 = None                      # list batches: timing event on the compute stream behind the wait for the upload
        self._lists = None
        self.cont_d = self.seg_d = None     # the device containers / segment lengths of the encode (records())
        self._rec_stage = None              # pinned staging buffer of records(): nbytes -> flat uint8 host tensor
        self._records = None
        self._records_prog = None
        self.crc_h = None                   # encode_batch_async(digests=True): the pinned int64 [B] digests, valid behind ev
        self._crc_decoded = None            # ... and those of records(progressive=True)'s decode of the batch (digests(verify=True))

    def digests(self, verify=False):
        """The pixel digests of the batch, a list of B ints: zlib.crc32 of every image's pixels as planar uint8 [3][H][W] bytes, computed on the
        device behind the encode (encode_batch_async(digests=True)).  Waits for the handle's download.  verify=True: records(progressive=True)
        pays a full decode of the batch's containers; the digests of THAT decode are held against the encode's, and a difference raises
        ValueError naming the images -- a round-trip check at pack time for the price of two small kernels."""
        if self.crc_h is None:
            raise ValueError("this handle holds no digests: encode_batch_async(..., digests=True)")
        self.ev.synchronize()
        crc = [int(v) for v in self.crc_h.numpy()]
        if verify:
            self.records(progressive=True)
            bad = [b for b, (a, d) in enumerate(zip(crc, self._crc_decoded)) if a != d]
            if bad:
                raise ValueError("images %s decode to other pixels than were encoded (crc32 %s, encoded %s)" % (
                    bad, ["%08x" % self._crc_decoded[b] for b in bad], ["%08x" % crc[b] for b in bad]))
        return crc

    def records(self, check=True, progressive=False):
        """progressive=True: the batch as one dense blob of PROGRESSIVE records (llicti_amd/progressive.py) -> (blob, rec_off, prefix): as below,
        plus prefix int64 [B, 6], every image's P_0 .. P_L; what progressive.ProgressiveWriter.append_records takes.  xwide containers only
        ("auto", "xrans<M>").  HipCodec.level_cuts + pack_progressive behind the encode: this costs ONE DECODE of the batch (the cuts are the
        decoder's cursors) -- archives are built once.
        Otherwise: the batch as ONE dense blob of .llic records -> (blob, rec_off): blob a uint8 numpy view of the pinned staging buffer (valid until
        the next records() of the same slot), rec_off int64 [B + 1]; blob[rec_off[b]:rec_off[b + 1]] is image b's .llic file, the whole blob what
        archive.ArchiveWriter.append_records takes.  Made on the device (HipCodec.pack_records) behind the encode and downloaded as one dense
        copy of rec_off[B] bytes -- the real bytes, not B container strides.  Synchronous; check as for lists()."""
        if progressive:
            return self._records_progressive(check)
        if self._records is None:
            if self.cont_d is None:
                raise ValueError("this handle does not hold its device containers")
            codec = self.codec
            cur = torch.cuda.current_stream(codec.device)
            cur.wait_event(self.ev)
            with torch.cuda.device(codec.device):
                blob, ro = codec.pack_records(self.cont_d, self.seg_d)
                ro_h = ro.cpu()                                      # (waits for the scan: the total decides the size of the copy)
                total = int(ro_h[-1])
                host = self._rec_stage(max(total, 1)) if self._rec_stage is not None else torch.empty((max(total, 1),), dtype=torch.uint8).pin_memory()
                host[:total].copy_(blob[:total], non_blocking=True)
                cur.synchronize()
            if check:
                codec.check()
            self._records = (host[:total].numpy(), ro_h.numpy())
        return self._records

    def _records_progressive(self, check):
        if self._records_prog is None:
            if self.cont_d is None:
                raise ValueError("this handle does not hold its device containers")
            codec = self.codec
            cur = torch.cuda.current_stream(codec.device)
            cur.wait_event(self.ev)
            with torch.cuda.device(codec.device):
                hdr = self.cont_d[:, :17].contiguous().cpu().numpy()          # (what the encoder wrote: an "auto" encode picks the stream counts)
                modes = [mode_of_header(hdr[b]) for b in range(hdr.shape[0])]
                if any((m >> 8) != 5 for m in modes):
                    raise ValueError("progressive records hold xwide containers: encode with container \"auto\" or \"xrans<M>\"")
                dims = [header_dims(bytes(hdr[b])) for b in range(hdr.shape[0])]
                cuts = codec.level_cuts(self.cont_d, self.seg_d, [d[0] for d in dims], [d[1] for d in dims], modes)
                # (level_cuts is a full decode: its planes are in the workspace; a handle with digests has them digested for digests(verify=True))
                crc_dec = codec.digests([d[0] for d in dims], [d[1] for d in dims], modes)[0] if self.crc_h is not None else None
                blob, ro, pre = codec.pack_progressive(self.cont_d, self.seg_d, cuts)
                ro_h, pre_h = ro.cpu(), pre.cpu()
                if crc_dec is not None:
                    self._crc_decoded = [int(v) for v in crc_dec.cpu().numpy()]
                total = int(ro_h[-1])
                host = torch.empty((max(total, 1),), dtype=torch.uint8).pin_memory()
                host[:total].copy_(blob[:total], non_blocking=True)
                cur.synchronize()
            if check:
                codec.check()
            self._records_prog = (host[:total].numpy(), ro_h.numpy(), pre_h.numpy())
        return self._records_prog

    def lists(self, check=True):
        """Wait for the download (NOT for anything enqueued after it) and cut the containers into bytestream_lists (1 + L lists x 9 `bytes`).
        check=False leaves the device-side status to a later codec.check() (which synchronises the whole stream)."""
        if self._lists is None:
            self.ev.synchronize()
            if check:
                self.codec.check()
            seg_np, cont_np = self.seg_h.numpy(), self.cont_h.numpy()
            self._lists = [container_to_bytestream_list(cont_np[b], seg_np[b]) for b in range(seg_np.shape[0])]
        return self._lists
